#!/usr/bin/env python3
"""The wide16 batch coders (16-bit symbols, one static table of up to 65536 symbols held in device
memory) beside the wide coders (tables in LDS, up to 4096 symbols) and the single-table 8-bit
static coders, in one process: HIP-event times of encode and decode, warm-up as in
tools/kbench.py, the round trip checked.  Run by hand, not by a test.

  python3 tools/kbench_wide16.py --chunks 65536 --chunk-symbols 16384 --n 4096 16384 65536 --out F
  python3 tools/kbench_wide16.py --bf16 --out F

Symbols: Zipf(1.2) over n symbols, quantised to a total of 65536 with every c >= 1
(rc_quantize_counts_wide16), drawn in HBM through the table's inverse CDF.  Two yardsticks: the
wide coder at n = 4096 on the same symbols (the price of moving the table out of LDS), and the
8-bit static coder on the n = 256 symbol values as bytes (DESIGN.md §9.6's).  A scratch build with
-DRC_WIDE16_STATS (RC_LIB_PATH) adds the share of wave-symbols that took the decoder's fix-up.
Prints one JSON line per run; --out also writes them as a JSON list.

--fine: after each wide16 run, the same symbols through wide16 fine models of the same Zipf weights
quantised to totals 2^17, 2^20 and 2^24, in the same process, so that each rate's ratio to the
wide16 coders at total 2^16 is a same-run ratio.  A scratch build with -DRC_WIDE16_FINE_STATS adds
the shares of wave-symbols that ran the decoder's rank search and its fix-up.

--dense: int16 Laplace(b = 1500) samples and fp16 bit patterns of standard normals, 2^26 symbols in
2^12 chunks: code bytes and rates under build_wide16_model at totals 2^16 (wide16), 2^20 and 2^24
(fine), beside the ideal bits numpy gives for the same tables.  A report.

--bf16: float32 normals cast to bf16 bit patterns, 2^26 symbols in 2^12 chunks: the code bytes and
the rates of build_wide16_model + the wide16 coders against the route such data had before, the
same bytes through fit_order1_set(period=2, n_models=8) and the order-1 coders.  A report."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zipf_table(rc, n, total=65536):
    w = 1.0 / np.arange(1, n + 1, dtype=np.float64) ** 1.2
    counts = np.maximum(1, np.round(w / w.sum() * 1e12)).astype(np.uint64)
    if total > 65536:
        return rc.quantize_counts_wide16_fine(counts, total, all_symbols=True)
    return rc.quantize_counts_wide16(counts, total, all_symbols=True)


FINE_TOTALS = (1 << 17, 1 << 20, 1 << 24)


def timed(torch, a, enc, dcd, fe, fd, ol, src, dst, n_sym, sym_bytes, extra):
    for _ in range(a.warmup):
        enc()
        dcd()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]
    torch.cuda.synchronize()
    for e0, e1, e2 in ev:
        e0.record()
        enc()
        e1.record()
        dcd()
        e2.record()
    torch.cuda.synchronize()
    te = float(np.mean([x.elapsed_time(y) for x, y, _ in ev]))
    td = float(np.mean([y.elapsed_time(z) for _, y, z in ev]))
    ok = int(fe.abs().sum()) == 0 and int(fd.abs().sum()) == 0
    for i in range(0, dst.numel(), 1 << 30):
        ok = ok and torch.equal(dst[i:i + (1 << 30)], src[i:i + (1 << 30)])
    code = int(ol.sum())
    res = dict(steps=a.steps, symbols=n_sym, encode_ms=round(te, 3), decode_ms=round(td, 3),
               encode_gsym_s=round(n_sym / te / 1e6, 3), decode_gsym_s=round(n_sym / td / 1e6, 3),
               code_bytes=code, bytes_per_symbol=round(code / n_sym, 5),
               alg_bytes=sym_bytes * n_sym + code, bit_exact_round_trip=bool(ok))
    res.update(extra)
    print(json.dumps(res), flush=True)
    return res


def bench_zipf(a, torch, rc, ctx):
    n, L = a.chunks, a.chunk_symbols
    dev = torch.device("cuda", 0)
    total = 65536
    syms = torch.empty(n * L, dtype=torch.int16, device=dev)
    dec = torch.empty(n * L, dtype=torch.int16, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    # (every c >= 1 of 65536: 16 bits at most; of 2^24: 24 and the fine models' allowance)
    cap = rc.slot_capacity(L, 24.125 if a.fine else 16.0, slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

    def fill(c, seed):
        """syms <- inverse CDF of c at uniform 16-bit draws, a piece at a time"""
        inv = torch.from_numpy(np.repeat(np.arange(len(c), dtype=np.uint16), c)
                               .view(np.int16)).to(dev)
        assert inv.numel() == total
        g = torch.Generator(device=dev).manual_seed(seed)
        step = 1 << 26
        for i in range(0, n * L, step):
            m = min(step, n * L - i)
            u = torch.randint(0, total, (m,), dtype=torch.int32, device=dev, generator=g)
            syms[i:i + m] = inv[u]

    def run(name, enc, dcd, src, dst, sym_bytes, extra):
        extra = dict(coder=name, chunks=n, chunk_symbols=L, table_total=total, **extra)
        return timed(torch, a, enc, dcd, fe, fd, ol, src, dst, n * L, sym_bytes, extra)

    results = []
    # yardstick 1: the n = 256 symbol values as bytes through the 8-bit static coders
    c, cum, _ = zipf_table(rc, 256)
    fill(c, 0x5EED0100)
    syms8 = syms.to(torch.uint8)
    dec8 = torch.empty_like(syms8)
    m = rc.StaticModel(c, cum, total, ctx=ctx)
    base = run("static", lambda: rc.encode_batch(m, syms8, so, out, oo, ol, fe),
               lambda: rc.decode_batch(m, out, co, ol, dec8, so, fd), syms8, dec8, 1, {})
    results.append(base)
    del dec8, syms8
    wide4096 = None
    stats = getattr(ctx._lib, "rc_wide16_stats_read_", None)
    st = (ctypes.c_uint64 * 2)()
    for ns in a.n:
        c, cum, _ = zipf_table(rc, ns)
        fill(c, 0x5EED0000 + ns)
        if ns <= 4096:  # yardstick 2: the wide coders (table in LDS) on the same symbols
            w = rc.WideStaticModel(c, cum, total, ctx=ctx)
            wide4096 = run("wide", lambda: rc.encode_batch_wide(w, syms, so, out, oo, ol, fe),
                           lambda: rc.decode_batch_wide(w, out, co, ol, dec, so, fd), syms, dec,
                           2, dict(n_symbols=ns))
            results.append(wide4096)
            w.close()
            dec.zero_()
        w16 = rc.Wide16StaticModel(c, cum, total, ctx=ctx)
        if stats is not None:
            stats(st)  # (reading clears the counters)
        r = run("wide16", lambda: rc.encode_batch_wide16(w16, syms, so, out, oo, ol, fe),
                lambda: rc.decode_batch_wide16(w16, out, co, ol, dec, so, fd), syms, dec, 2,
                dict(n_symbols=ns, plan=w16.plan()))
        if stats is not None and stats(st) == 0 and st[0]:
            r["fixup_wave_symbol_share"] = round(st[1] / st[0], 6)
        r["encode_vs_static"] = round(r["encode_gsym_s"] / base["encode_gsym_s"], 4)
        r["decode_vs_static"] = round(r["decode_gsym_s"] / base["decode_gsym_s"], 4)
        if ns <= 4096:
            r["encode_vs_wide"] = round(r["encode_gsym_s"] / wide4096["encode_gsym_s"], 4)
            r["decode_vs_wide"] = round(r["decode_gsym_s"] / wide4096["decode_gsym_s"], 4)
        print(json.dumps({k: v for k, v in r.items() if "_vs_" in k or k in
                          ("n_symbols", "fixup_wave_symbol_share")}), flush=True)
        results.append(r)
        w16.close()
        if a.fine:
            results += bench_fine(a, rc, ctx, ns, r, run, syms, dec, so, out, oo, co, ol, fe, fd)
    return results


def bench_fine(a, rc, ctx, ns, w16_res, run, syms, dec, so, out, oo, co, ol, fe, fd):
    """The symbols the wide16 run just coded, through fine models of the same weights."""
    stats = getattr(ctx._lib, "rc_wide16_fine_stats_read_", None)
    st = (ctypes.c_uint64 * 3)()
    res = []
    for total in FINE_TOTALS:
        c, cum, t = zipf_table(rc, ns, total)
        fm = rc.Wide16FineModel(c, cum, t, ctx=ctx)
        dec.zero_()
        if stats is not None:
            stats(st)  # (reading clears the counters)
        r = run("wide16_fine", lambda: rc.encode_batch_wide16(fm, syms, so, out, oo, ol, fe),
                lambda: rc.decode_batch_wide16(fm, out, co, ol, dec, so, fd), syms, dec, 2,
                dict(n_symbols=ns, plan=fm.plan()))
        r["table_total"] = total
        if stats is not None and stats(st) == 0 and st[0]:
            r["search_wave_symbol_share"] = round(st[1] / st[0], 6)
            r["fixup_wave_symbol_share"] = round(st[2] / st[0], 6)
        r["encode_vs_wide16"] = round(r["encode_gsym_s"] / w16_res["encode_gsym_s"], 4)
        r["decode_vs_wide16"] = round(r["decode_gsym_s"] / w16_res["decode_gsym_s"], 4)
        r["bytes_per_symbol_wide16"] = w16_res["bytes_per_symbol"]
        print(json.dumps({k: v for k, v in r.items() if "_vs_" in k or "share" in k or k in
                          ("n_symbols", "table_total", "bytes_per_symbol",
                           "bytes_per_symbol_wide16")}), flush=True)
        res.append(r)
        fm.close()
    return res


def bench_dense(a, torch, rc, ctx):
    """Dense 16-bit sources: the code under tables of total 2^16, 2^20 and 2^24."""
    dev = torch.device("cuda", 0)
    n, L = 1 << 12, 1 << 14
    g = torch.Generator(device=dev).manual_seed(0xDE75E)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = rc.slot_capacity(L, 18.0, slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)
    results = []
    for data in ("int16 Laplace(b=1500)", "fp16 bits of N(0,1)"):
        if data.startswith("int16"):
            u = torch.rand(n * L, device=dev, generator=g, dtype=torch.float64) - 0.5
            x = -1500.0 * torch.sign(u) * torch.log1p(-2.0 * u.abs())
            syms = x.round().clamp_(-32768, 32767).to(torch.int16)
            del u, x
        else:
            x = torch.randn(n * L, device=dev, generator=g, dtype=torch.float32)
            syms = x.to(torch.float16).view(torch.int16)
            del x
        counts = rc.histogram16(syms, so, ctx=ctx).cpu().numpy().astype(np.float64)
        nz = counts > 0
        entropy = float(-(counts[nz] / counts.sum() * np.log2(counts[nz] / counts.sum())).sum())
        dec = torch.empty_like(syms)
        for total in (1 << 16, 1 << 20, 1 << 24):
            m = rc.build_wide16_model(syms, so, target_total=total, ctx=ctx)
            cm = m.c.astype(np.float64)
            ideal = float((counts[:len(cm)][cm > 0] * np.log2(total / cm[cm > 0])).sum())
            dec.zero_()
            results.append(timed(
                torch, a, lambda: rc.encode_batch_wide16(m, syms, so, out, oo, ol, fe),
                lambda: rc.decode_batch_wide16(m, out, co, ol, dec, so, fd), fe, fd, ol, syms, dec,
                n * L, 2, dict(coder=type(m).__name__, data=data, chunks=n, chunk_symbols=L,
                               table_total=total, n_symbols=m.n_symbols,
                               distinct_symbols=int(nz.sum()), entropy_bits=round(entropy, 4),
                               ideal_bits_per_symbol=round(ideal / (n * L), 4),
                               ideal_bytes=int(np.ceil(ideal / 8)))))
            m.close()
        del syms, dec
    return results


def bench_bf16(a, torch, rc, ctx):
    """bf16 bit patterns of standard normals: wide16 against the periodic order-1 route."""
    dev = torch.device("cuda", 0)
    n, L = 1 << 12, 1 << 14
    g = torch.Generator(device=dev).manual_seed(0xBF16)
    x = torch.randn(n * L, device=dev, generator=g, dtype=torch.float32)
    syms = (x.view(torch.int32) >> 16).to(torch.int16)
    del x
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = rc.slot_capacity(L, 17.0, slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)
    results = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w16 = rc.build_wide16_model(syms, so, ctx=ctx)
    w16.handle
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    dec = torch.empty_like(syms)
    distinct = int((w16.c > 0).sum())
    results.append(timed(torch, a, lambda: rc.encode_batch_wide16(w16, syms, so, out, oo, ol, fe),
                         lambda: rc.decode_batch_wide16(w16, out, co, ol, dec, so, fd), fe, fd,
                         ol, syms, dec, n * L, 2,
                         dict(coder="wide16", data="bf16 bits of N(0,1)", chunks=n,
                              chunk_symbols=L, n_symbols=w16.n_symbols,
                              distinct_symbols=distinct, model_build_s=round(t_build, 3))))
    # the route before: the same bytes, a periodic order-1 set (the low byte's row chosen by the
    # previous symbol's high byte, the high byte's by the low byte in front of it)
    b = syms.view(torch.uint8)
    bo = so * 2
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o1 = rc.fit_order1_set(b, bo, n_models=8, period=2, ctx=ctx)
    o1.handle
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    decb = torch.empty_like(b)
    r = timed(torch, a, lambda: rc.encode_batch_order1(o1, b, bo, out, oo, ol, fe),
              lambda: rc.decode_batch_order1(o1, out, co, ol, decb, bo, fd), fe, fd, ol, b, decb,
              n * L, 2, dict(coder="order1 period 2, 8 rows, on the bytes",
                             data="bf16 bits of N(0,1)", chunks=n, chunk_symbols=L,
                             model_build_s=round(t_fit, 3)))
    results.append(r)
    print(json.dumps(dict(wide16_vs_order1_code_bytes=round(results[0]["code_bytes"] /
                                                             r["code_bytes"], 4),
                          wide16_vs_order1_encode=round(results[0]["encode_gsym_s"] /
                                                        r["encode_gsym_s"], 4),
                          wide16_vs_order1_decode=round(results[0]["decode_gsym_s"] /
                                                        r["decode_gsym_s"], 4))), flush=True)
    return results


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=1 << 16)
    p.add_argument("--chunk-symbols", type=int, default=16384)
    p.add_argument("--n", type=int, nargs="+", default=[4096, 16384, 65536])
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--fine", action="store_true")
    p.add_argument("--dense", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    ctx = rc.default_context(0)
    results = (bench_bf16(a, torch, rc, ctx) if a.bf16 else bench_dense(a, torch, rc, ctx)
               if a.dense else bench_zipf(a, torch, rc, ctx))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["bit_exact_round_trip"] for r in results) else 3)


if __name__ == "__main__":
    main()
