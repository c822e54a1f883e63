#!/usr/bin/env python3
"""rc_stream_decode_rows / rc_stream_encode_rows (a table per symbol out of rows in device memory)
in one process: HIP-event times, warm-up first, every run listed.  Run by hand, not by a test.

  python3 tools/kbench_rows.py --streams 4096 --n-symbols 256 --route-b --out FILE

Input: --rows mixed rows (about 70% live symbols, counts below 2^19), --symbols symbols per
stream, row_of uniform random, every symbol one of its row's live ones; numpy / torch generators
seeded with 1.  Measured, each as --pairs alternated pairs with fresh states before every call:
  new      the two new calls on the random rows (Gsym/s)
  one_row  every row_of = 0: rc_stream_encode (on the gathered triples) and rc_stream_decode (on
           row 0), alternated with the new calls on the same input; ratio = one-table time /
           new time (above 1: the new call is faster)
  route_b  (--route-b) a row sequence shared by all streams, in runs of 1 and of 64 symbols: one
           rc_stream_decode launch per run (the only batch route before these calls; its symbols
           land run-major), alternated with one rc_stream_decode_rows call on the same streams.
  decoders (--compare-decoders) rc_stream_decode_rows's two kernels, the wave-per-stream and the
           lane-per-stream one, each forced through the library's hook and alternated on the
           random rows; lane_speedup = wave time / lane time
--decoder auto | wave | lane sets the kernel of every other rc_stream_decode_rows call (auto: the
library's rule; a library without the hook, such as an earlier revision's, takes auto only).
--sweep-streams 64,4096,... runs everything once per stream count on the same table (instead of
--streams); --no-one-row leaves the one_row section out.
Every decode is checked against the symbols that were encoded.  Prints one JSON line per stream
count; --out also writes them as a JSON list."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def set_decoder(ctx, name):
    """rc_stream_decode_rows's kernel for this context, through the library's host-only hook"""
    which = {"auto": 0, "wave": 1, "lane": 2}[name]
    if not hasattr(ctx._lib, "rc_rows_decoder_"):
        if which:
            raise SystemExit("this library has one row decoder: --decoder auto only")
        return
    if ctx._lib.rc_rows_decoder_(ctx.handle, which) != 0:
        raise SystemExit("rc_rows_decoder_ refused " + name)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--streams", type=int, default=4096)
    p.add_argument("--sweep-streams", type=lambda v: [int(x) for x in v.split(",")], default=None,
                   help="comma-separated stream counts, one result each (instead of --streams)")
    p.add_argument("--decoder", choices=("auto", "wave", "lane"), default="auto",
                   help="rc_stream_decode_rows's kernel: the library's rule, or one forced")
    p.add_argument("--compare-decoders", action="store_true",
                   help="also the forced wave against the forced lane kernel, alternated")
    p.add_argument("--no-one-row", action="store_true", help="leave the one_row section out")
    p.add_argument("--symbols", type=int, default=4096)
    p.add_argument("--n-symbols", type=int, default=256)
    p.add_argument("--rows", type=int, default=1024)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--route-b", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    from range_coder_rust_amd import _native as N
    ctx = rc.default_context(0)
    set_decoder(ctx, a.decoder)
    dev = torch.device("cuda", 0)
    L, A, R = a.symbols, a.n_symbols, a.rows
    rng = np.random.default_rng(1)
    counts = rng.integers(1, 1 << 19, (R, A))
    counts[rng.random((R, A)) > 0.7] = 0
    counts[np.arange(R), rng.integers(0, A, R)] |= 1
    table = rc.RowTable.from_counts(counts, ctx=ctx)
    tab = (table.c, table.cum, table.total)
    total_h = counts.sum(axis=1)
    live = torch.from_numpy(counts > 0).to(dev)
    order = torch.argsort((~live).to(torch.uint8), dim=1, stable=True)  # a row's live symbols first
    n_live = live.sum(dim=1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def symbols_for(row_of):
        """one live symbol of its row per entry of row_of (int32 tensor)"""
        out = torch.empty(row_of.numel(), dtype=torch.uint8, device=dev)
        for i in range(0, row_of.numel(), 1 << 24):
            r = row_of[i:i + (1 << 24)].long()
            u = torch.randint(0, 1 << 30, (r.numel(),), device=dev, generator=gen)
            out[i:i + (1 << 24)] = order[r, u % n_live[r]].to(torch.uint8)
        return out

    results, ok = [], True
    for n in a.sweep_streams or [a.streams]:
        res, good = run_one(a, n, ctx, dev, rc, N, torch, tab, table, total_h, rng, gen,
                            symbols_for)
        print(json.dumps(res), flush=True)
        results.append(res)
        ok = ok and good
        if a.out:  # (rewritten after every count: a sweep cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    sys.exit(0 if ok else 3)


def run_one(a, n, ctx, dev, rc, N, torch, tab, table, total_h, rng, gen, symbols_for):
    """every section at n streams: (the result, everything round-tripped)"""
    L, A, R = a.symbols, a.n_symbols, a.rows
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = N.stream_max_bytes(L, True)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fl = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n * L, dtype=torch.uint8, device=dev)
    fresh = rc.stream_states(n, dev)
    states = fresh.clone()

    def timed(calls, pairs):
        """calls run in this order `pairs` times, each from fresh states between two events"""
        ms = [[] for _ in calls]
        for _ in range(pairs):
            ev = []
            for f in calls:
                states.copy_(fresh)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            for m, (e0, e1) in zip(ms, ev):
                m.append(round(e0.elapsed_time(e1), 3))
        return ms

    def enc_rows(row_of, syms):
        return lambda: rc.stream_encode_rows_batch(ctx, *tab, row_of, syms, states, so, out, oo,
                                                   out_len=ol, finish=True, flags=fl)

    def dec_rows(row_of):
        return lambda: rc.stream_decode_rows_batch(ctx, *tab, row_of, states, out, co, ol, dec, so,
                                                   flags=fl)

    def clean():
        return int(fl.abs().sum()) == 0

    def gsym(ms):
        return round(n * L / float(np.mean(ms)) / 1e6, 4)

    res = dict(streams=n, symbols_per_stream=L, n_symbols=A, rows=R, pairs=a.pairs,
               lib=os.path.basename(N.LIB_PATH), decoder=a.decoder,
               sweep_streams=a.sweep_streams)
    if hasattr(ctx._lib, "rc_rows_decode_plan_"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        res["plan"] = ("wave", "lane")[ctx._lib.rc_rows_decode_plan_(n, A, cus)]
    ok = True

    # ---- the new calls on random rows
    row_of = torch.randint(0, R, (n * L,), device=dev, generator=gen).to(torch.int32)
    syms = symbols_for(row_of)
    calls = [enc_rows(row_of, syms), dec_rows(row_of)]
    timed(calls, a.warmup)
    ok_new = clean() and torch.equal(dec, syms)
    t = timed(calls, a.pairs)
    ok_new = ok_new and clean() and torch.equal(dec, syms)
    res["new"] = dict(encode_ms=t[0], decode_ms=t[1], encode_gsym_s=gsym(t[0]),
                      decode_gsym_s=gsym(t[1]), code_bytes_per_symbol=round(int(ol.sum()) / (n * L), 4),
                      round_trip=bool(ok_new))
    ok = ok and ok_new

    # ---- the two decoders, forced, alternated on the same streams
    if a.compare_decoders:
        def forced(name):
            def call():
                set_decoder(ctx, name)
                dec_rows(row_of)()
            return call

        states.copy_(fresh)
        enc_rows(row_of, syms)()
        calls = [forced("wave"), forced("lane")]
        good = True
        for reps in (a.warmup, a.pairs):
            t = timed(calls, reps)
            for f in calls:  # (each kernel's symbols checked, not only the last call's)
                states.copy_(fresh)
                dec.zero_()
                f()
                good = good and clean() and torch.equal(dec, syms)
        set_decoder(ctx, a.decoder)
        res["decoders"] = dict(wave_ms=t[0], lane_ms=t[1], wave_gsym_s=gsym(t[0]),
                               lane_gsym_s=gsym(t[1]),
                               lane_speedup=round(float(np.mean(t[0]) / np.mean(t[1])), 3),
                               round_trip=bool(good))
        ok = ok and good
    del row_of, syms
    # ---- every row_of = 0, beside the one-table kernels on the same input
    if not a.no_one_row:
        row0 = torch.zeros(n * L, dtype=torch.int32, device=dev)
        syms0 = symbols_for(row0)
        s64 = syms0.long()
        trip = torch.stack([table.c[0][s64], table.cum[0][s64],
                            table.total[0].expand(n * L)], dim=1).contiguous().view(-1)
        del s64
        c0, cum0 = table.c[0].contiguous(), table.cum[0].contiguous()
        calls = [lambda: rc.stream_encode_batch(ctx, states, trip, so, out, oo, out_len=ol,
                                                finish=True, flags=fl),
                 enc_rows(row0, syms0),
                 lambda: rc.stream_decode_batch(ctx, c0, cum0, int(total_h[0]), states, out, co, ol,
                                                dec, so, flags=fl),
                 dec_rows(row0)]
        timed(calls, a.warmup)
        t = timed(calls, a.pairs)
        ok0 = clean() and torch.equal(dec, syms0)
        res["one_row"] = dict(stream_encode_ms=t[0], encode_rows_ms=t[1], stream_decode_ms=t[2],
                              decode_rows_ms=t[3],
                              encode_ratio=round(float(np.mean(t[0]) / np.mean(t[1])), 4),
                              decode_ratio=round(float(np.mean(t[2]) / np.mean(t[3])), 4),
                              stream_encode_gsym_s=gsym(t[0]), encode_rows_gsym_s=gsym(t[1]),
                              stream_decode_gsym_s=gsym(t[2]), decode_rows_gsym_s=gsym(t[3]),
                              round_trip=bool(ok0))
        ok = ok and ok0
        del row0, syms0, trip

    # ---- the batch route for changing rows before these calls: a launch per run of equal rows
    if a.route_b:
        res["route_b"] = []
        for run in (1, 64):
            runs = L // run
            seq = rng.integers(0, R, runs)
            row_of = torch.from_numpy(np.repeat(seq, run).astype(np.int32)).to(dev).repeat(n)
            syms = symbols_for(row_of)
            states.copy_(fresh)
            enc_rows(row_of, syms)()
            ok = ok and clean()
            # launch j decodes symbols [j run, (j + 1) run) of every stream into a run-major array
            so_b = (torch.arange(runs, dtype=torch.int64, device=dev)[:, None] * n +
                    torch.arange(n + 1, dtype=torch.int64, device=dev)[None, :]) * run
            dec_b = torch.zeros(n * L, dtype=torch.uint8, device=dev)
            rows_c = [(table.c[r], table.cum[r], int(total_h[r])) for r in seq]

            def route_b():
                for j, (cj, cumj, tj) in enumerate(rows_c):
                    rc.stream_decode_batch(ctx, cj, cumj, tj, states, out, co, ol, dec_b, so_b[j],
                                           flags=fl)

            calls = [route_b, dec_rows(row_of)]
            timed(calls, a.warmup)
            t = timed(calls, a.pairs)
            same = torch.equal(dec, syms) and torch.equal(
                dec_b.view(runs, n, run).permute(1, 0, 2).reshape(-1), syms)
            res["route_b"].append(dict(
                run=run, launches=runs, launches_ms=t[0], decode_rows_ms=t[1],
                launches_gsym_s=gsym(t[0]), decode_rows_gsym_s=gsym(t[1]),
                speedup=round(float(np.mean(t[0]) / np.mean(t[1])), 2), same_symbols=bool(same)))
            ok = ok and same and clean()
            del row_of, syms, so_b, dec_b
    return res, ok


if __name__ == "__main__":
    main()
