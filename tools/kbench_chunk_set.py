#!/usr/bin/env python3
"""Static chunk sets (a model per chunk) beside the single-table static coders
and beside the indexed coders fed the index stream expanded from class_of (the only route before
chunk sets), on the same symbols in one process: HIP-event times after warm-up, the round trip
checked.  Then the kernels that fit the classes.  Run by hand, not by a test.

  python3 tools/kbench_chunk_set.py --chunks 65536 --chunk-bytes 16384 --k 1 8 64 --out FILE
  python3 tools/kbench_chunk_set.py --fit-rows 1048576 --k 8 64 --out FILE
  python3 tools/kbench_chunk_set.py --fit-symbols 268435456 --out FILE

Coders.  Symbols: Zipf(1.2) over 256 symbols, generated in HBM (rc_synth_fill).  Row j of a set of
K is the Zipf(1.2) table rotated by j * 256 / K; class_of is a hash of the chunk id.  The
yardstick is the single-table coder with row 0.  Reported per K: Gsym/s of the chunk-set and the
indexed calls, their ratios to the yardstick, the decoder variant, workgroup size and grid the
launch really took (rc_chunk_last_), the grouping step's own time at that size (rc_chunk_group_)
and the share of dead lanes in its used workgroups.  With these symbols
a chunk of class j > 0 meets a table that does not fit it (nearly twice the code bytes, and the
coders' rare paths far more often), so its work is not the yardstick's.  --matched rotates the
symbols of chunk k with its row, so that every chunk meets its own table and does the
yardstick's work: that run isolates what the grouped launch itself costs.  --sorted-classes gives
the classes as contiguous runs of chunks, so that the grouped order is the chunk order and a wave's
chunks are neighbours in memory as in the ungrouped launch.

Fit.  --fit-rows: rc_chunk_set_costs over that many random histogram rows against K calls of
rc_ideal_bits plus a torch argmin (the route before it), and against the time to read the rows
once at the rate a device copy reaches.  --fit-symbols: fit_chunk_set end to end on a four-source
mixture of that many symbols in 4 KiB chunks."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in ev]))


def coders(a, torch, rc, results):
    from range_coder_rust_amd import synth
    from range_coder_rust_amd.api import _ptr
    ctx = rc.default_context(0)
    n, L = a.chunks, a.chunk_bytes
    c, cum, total = synth.zipf_table()
    dev = torch.device("cuda", 0)
    syms = torch.empty(n * L, dtype=torch.uint8, device=dev)
    synth.fill(ctx, 0x5EED0001, synth.inverse_cdf(c), syms, L, n)
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = rc.slot_capacity(L, float(np.log2(total / float(c.min()))), slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(name, enc, dcd, extra, ref=None):
        ref = syms if ref is None else ref
        te = event_ms(torch, enc, a.steps, a.warmup)
        td = event_ms(torch, dcd, a.steps, a.warmup)
        ok = int(fe.abs().sum()) == 0 and int(fd.abs().sum()) == 0
        for i in range(0, n * L, 1 << 30):
            ok = ok and torch.equal(dec[i:i + (1 << 30)], ref[i:i + (1 << 30)])
        res = dict(coder=name, chunks=n, chunk_bytes=L, steps=a.steps, table_total=int(total),
                   encode_ms=round(te, 3), decode_ms=round(td, 3),
                   encode_gsym_s=round(n * L / te / 1e6, 3),
                   decode_gsym_s=round(n * L / td / 1e6, 3),
                   bytes_per_symbol=round(int(ol.sum()) / (n * L), 5),
                   bit_exact_round_trip=bool(ok))
        res.update(extra)
        print(json.dumps(res), flush=True)
        results.append(res)
        return res

    m = rc.StaticModel(c, cum, total, ctx=ctx)
    base = timed("static", lambda: rc.encode_batch(m, syms, so, out, oo, ol, fe),
                 lambda: rc.decode_batch(m, out, co, ol, dec, so, fd), {})
    k_id = np.arange(n, dtype=np.uint64)
    for K in a.k:
        rows = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // K) for j in range(K)])
        cls_h = ((k_id * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(40)) % np.uint64(K))
        if a.sorted_classes:  # the classes as contiguous runs of chunks: the grouped order is k
            cls_h = k_id * np.uint64(K) // np.uint64(n)
        cls = torch.from_numpy(cls_h.astype(np.uint8)).to(dev)
        cset = rc.ChunkModelSet(rows, None, total, ctx=ctx)
        src = syms
        if a.matched:  # chunk k's symbols rotated with its row: every chunk meets its own table
            rot = torch.from_numpy(((np.arange(K) * 256) // K).astype(np.uint8)).to(dev)
            src = (syms.view(n, L) + rot[cls.to(torch.int64)].view(n, 1)).reshape(-1)
        # what the decoder's launch really takes (LUT 6 runs 1,024 lanes once the padded grid
        # fills the device, whatever the set's plan says): one round trip, then the context's
        # record of its last coder launch
        rc.encode_batch_chunk_set(cset, cls, src, so, out, oo, ol, fe)
        rc.decode_batch_chunk_set(cset, cls, out, co, ol, dec, so, fd)
        last = (ctypes.c_uint32 * 3)()
        ctx._lib.rc_chunk_last_(ctx.handle, last)
        W, lut, grid = int(last[0]), int(last[1]), int(last[2])
        d_order = torch.empty(grid * W, dtype=torch.int32, device=dev)
        d_row = torch.empty(grid, dtype=torch.int32, device=dev)
        d_fl = torch.empty(n, dtype=torch.int32, device=dev)
        ctx.bind_stream()
        t_group = event_ms(torch, lambda: ctx._lib.rc_chunk_group_(
            ctx.handle, _ptr(cls), n, K, W, _ptr(d_order), _ptr(d_row), _ptr(d_fl)), a.steps,
            a.warmup)
        dead = 1.0 - n / float(int((d_row >= 0).sum()) * W)
        r = timed("chunk_set",
                  lambda: rc.encode_batch_chunk_set(cset, cls, src, so, out, oo, ol, fe),
                  lambda: rc.decode_batch_chunk_set(cset, cls, out, co, ol, dec, so, fd),
                  dict(k=K, matched=bool(a.matched), sorted_classes=bool(a.sorted_classes),
                       group_ms=round(t_group, 4), group_lanes=W,
                       dead_lane_share=round(dead, 5), decoder_lut=lut, decoder_grid=grid),
                  ref=src)
        r["encode_vs_static"] = round(r["encode_gsym_s"] / base["encode_gsym_s"], 4)
        r["decode_vs_static"] = round(r["decode_gsym_s"] / base["decode_gsym_s"], 4)
        cset.close()
        if not a.no_indexed:
            mset = rc.StaticModelSet(rows, None, total, ctx=ctx)
            idx = cls.repeat_interleave(L)  # the index stream expanded from class_of
            ri = timed("indexed",
                       lambda: rc.encode_batch_indexed(mset, src, idx, so, out, oo, ol, fe),
                       lambda: rc.decode_batch_indexed(mset, out, co, ol, idx, dec, so, fd),
                       dict(k=K, matched=bool(a.matched)), ref=src)
            ri["encode_vs_static"] = round(ri["encode_gsym_s"] / base["encode_gsym_s"], 4)
            ri["decode_vs_static"] = round(ri["decode_gsym_s"] / base["decode_gsym_s"], 4)
            del idx
            mset.close()
        print(json.dumps({kk: r[kk] for kk in ("k", "encode_vs_static", "decode_vs_static",
                                               "group_ms", "dead_lane_share")}), flush=True)


def fit_rows(a, torch, rc, results):
    from range_coder_rust_amd import model_build as MB
    from range_coder_rust_amd import synth
    ctx = rc.default_context(0)
    dev = torch.device("cuda", 0)
    n = a.fit_rows
    hist = torch.randint(0, 64, (n, 256), dtype=torch.int32, device=dev)
    c, cum, total = synth.zipf_table()
    copy = torch.empty_like(hist)
    t_copy = event_ms(torch, lambda: copy.copy_(hist), a.steps, a.warmup)
    read_ms = t_copy / 2  # (a copy reads and writes the rows once each)
    del copy
    for K in a.k:
        rows = [np.roll(np.asarray(c, np.uint32), (j * 256) // K) for j in range(K)]
        tabs = np.stack([MB.cost_table(r, total) for r in rows])
        t_cost = event_ms(torch, lambda: MB.chunk_set_costs(hist, tabs, ctx=ctx), a.steps,
                          a.warmup)
        models = [rc.StaticModel(r, None, total, ctx=ctx) for r in rows]

        def before():
            bits = torch.stack([MB.ideal_bits(mm, hist) for mm in models])
            return torch.argmin(bits, dim=0)
        t_before = event_ms(torch, before, max(1, a.steps // 2), 1)
        for mm in models:
            mm.close()
        res = dict(bench="chunk_set_costs", rows=n, k=K, costs_ms=round(t_cost, 3),
                   ideal_bits_argmin_ms=round(t_before, 3), read_rows_once_ms=round(read_ms, 3),
                   rows_gb_s=round(n * 1024 / t_cost / 1e6, 1),
                   vs_before=round(t_before / t_cost, 2), vs_read=round(t_cost / read_ms, 2))
        print(json.dumps(res), flush=True)
        results.append(res)


def fit_end_to_end(a, torch, rc, results):
    dev = torch.device("cuda", 0)
    L = 4096
    n = a.fit_symbols // L
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    w = 1.0 / torch.arange(1, 257, dtype=torch.float64, device=dev) ** 1.2
    base = torch.multinomial((w / w.sum()).float(), n * L, replacement=True,
                             generator=g).to(torch.uint8).view(n, L)
    src = torch.randint(0, 4, (n, 1), device=dev, generator=g)
    uni = torch.randint(0, 256, (n, L), device=dev, generator=g, dtype=torch.uint8)
    syms = torch.where(src == 0, base, torch.where(src == 1, 255 - base, torch.where(
        src == 2, base + 128, uni))).reshape(-1)
    del base, uni
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    for K in a.k:
        rc.fit_chunk_set(syms, so, n_models=K)  # (warm-up: allocations, first launches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cs, cls = rc.fit_chunk_set(syms, so, n_models=K)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        agree = None
        if len(cs.c) >= 4:  # chunks of one source share a class
            pairs = torch.unique(torch.stack([src.view(-1), cls.to(torch.int64)]), dim=1)
            agree = int(pairs.shape[1])
        res = dict(bench="fit_chunk_set", symbols=n * L, chunks=n, k=K, rows_kept=len(cs.c),
                   seconds=round(dt, 4), gsym_s=round(n * L / dt / 1e9, 3),
                   source_class_pairs=agree)
        print(json.dumps(res), flush=True)
        results.append(res)
        cs.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=0)
    p.add_argument("--chunk-bytes", type=int, default=16384)
    p.add_argument("--k", type=int, nargs="+", default=[1, 8, 64])
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--no-indexed", action="store_true")
    p.add_argument("--matched", action="store_true")
    p.add_argument("--sorted-classes", action="store_true")
    p.add_argument("--fit-rows", type=int, default=0)
    p.add_argument("--fit-symbols", type=int, default=0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    results = []
    if a.chunks:
        coders(a, torch, rc, results)
    if a.fit_rows:
        fit_rows(a, torch, rc, results)
    if a.fit_symbols:
        fit_end_to_end(a, torch, rc, results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r.get("bit_exact_round_trip", True) for r in results) else 3)


if __name__ == "__main__":
    main()
