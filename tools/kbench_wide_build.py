#!/usr/bin/env python3
"""Model construction for wide models (rc_histogram_wide, rc_ideal_bits_wide) beside the 8-bit
rc_histogram, in one process: HIP-event times of the batch-only histogram, the histogram with
per-chunk rows and the ideal bits, warm-up as in tools/kbench_wide.py, the counts checked against
torch.bincount.  Run by hand, not by a test.

  python3 tools/kbench_wide_build.py --chunks 65536 --chunk-symbols 16384 --n 256 1024 4096 --out FILE

Symbols: Zipf(1.2) over n symbols, quantised to a total of 65536 with every c >= 1
(rc_quantize_counts_wide), drawn in HBM through the table's inverse CDF.  The yardstick is the
8-bit rc_histogram (batch only, and with rows) on the n = 256 symbol values as bytes.  GB/s count
the symbols read (2 B per wide symbol, 1 B per byte symbol).  Prints one JSON line per n and one
for the yardstick; --out also writes them as a JSON list."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zipf_table(rc, n, total=65536):
    w = 1.0 / np.arange(1, n + 1, dtype=np.float64) ** 1.2
    counts = np.maximum(1, np.round(w / w.sum() * 1e12)).astype(np.uint64)
    return rc.quantize_counts_wide(counts, total, all_symbols=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=1 << 16)
    p.add_argument("--chunk-symbols", type=int, default=16384)
    p.add_argument("--n", type=int, nargs="+", default=[256, 1024, 4096])
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    from range_coder_rust_amd import _native as N
    from range_coder_rust_amd.api import _ptr
    ctx = rc.default_context(0)
    lib = ctx._lib
    n, L = a.chunks, a.chunk_symbols
    dev = torch.device("cuda", 0)
    total = 65536
    syms = torch.empty(n * L, dtype=torch.int16, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    bits = torch.empty(n, dtype=torch.float64, device=dev)
    oob = torch.zeros((), dtype=torch.int64, device=dev)

    def fill(c, seed):
        """syms <- inverse CDF of c at uniform 16-bit draws, a piece at a time"""
        inv = torch.from_numpy(np.repeat(np.arange(len(c), dtype=np.int16), c)).to(dev)
        assert inv.numel() == total
        g = torch.Generator(device=dev).manual_seed(seed)
        step = 1 << 26
        for i in range(0, n * L, step):
            m = min(step, n * L - i)
            u = torch.randint(0, total, (m,), dtype=torch.int32, device=dev, generator=g)
            syms[i:i + m] = inv[u]

    def counts_of(src, bins):
        want = torch.zeros(bins, dtype=torch.int64, device=dev)
        for i in range(0, n * L, 1 << 28):
            want += torch.bincount(src[i:i + (1 << 28)].to(torch.int32), minlength=bins)
        return want

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(a.steps)]
        torch.cuda.synchronize()
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return float(np.mean([x.elapsed_time(y) for x, y in ev]))

    def rates(ms, sym_bytes):
        return dict(ms=round(ms, 3), gsym_s=round(n * L / ms / 1e6, 2),
                    gb_s=round(sym_bytes * n * L / ms / 1e6, 1))

    def ok(rcode):
        N.check(rcode, "kbench_wide_build")

    ctx.bind_stream()
    results = []
    # the yardstick: the n = 256 symbol values as bytes through the 8-bit histogram
    c, cum, _ = zipf_table(rc, 256)
    fill(c, 0x5EED0100)
    syms8 = syms.to(torch.uint8)
    want = counts_of(syms8, 256)
    hist = torch.zeros(256, dtype=torch.int64, device=dev)
    rows = torch.empty((n, 256), dtype=torch.int32, device=dev)
    t_b = timed(lambda: ok(lib.rc_histogram(ctx.handle, _ptr(syms8), _ptr(so), n, None,
                                            _ptr(hist))))
    exact = torch.equal(hist, want * (a.warmup + a.steps))
    t_r = timed(lambda: ok(lib.rc_histogram(ctx.handle, _ptr(syms8), _ptr(so), n, _ptr(rows),
                                            None)))
    exact = exact and torch.equal(rows.sum(0, dtype=torch.int64), want)
    base = dict(kernel="rc_histogram", chunks=n, chunk_symbols=L, steps=a.steps,
                batch_only=rates(t_b, 1), with_rows=rates(t_r, 1), counts_exact=bool(exact))
    print(json.dumps(base), flush=True)
    results.append(base)
    del syms8, rows
    for ns in a.n:
        c, cum, _ = zipf_table(rc, ns)
        if ns != 256:
            fill(c, 0x5EED0000 + ns)
        want = counts_of(syms, ns)
        w = rc.WideStaticModel(c, cum, total, ctx=ctx)
        hist = torch.zeros(ns, dtype=torch.int64, device=dev)
        rows = torch.empty((n, ns), dtype=torch.int32, device=dev)
        t_b = timed(lambda: ok(lib.rc_histogram_wide(ctx.handle, _ptr(syms), _ptr(so), n, ns, None,
                                                     _ptr(hist), _ptr(oob))))
        exact = torch.equal(hist, want * (a.warmup + a.steps)) and int(oob) == 0
        t_r = timed(lambda: ok(lib.rc_histogram_wide(ctx.handle, _ptr(syms), _ptr(so), n, ns,
                                                     _ptr(rows), None, None)))
        exact = exact and torch.equal(rows.sum(0, dtype=torch.int64), want)
        del rows
        t_i = timed(lambda: ok(lib.rc_ideal_bits_wide(ctx.handle, w.handle, _ptr(syms), _ptr(so),
                                                      n, _ptr(bits))))
        # the batch's ideal bits from the counts, against the sum of the per-chunk results
        icl = np.log2(total / np.asarray(c, np.float64))
        ideal = float((want.cpu().numpy() * icl).sum())
        got = float(bits.sum())
        r = dict(kernel="rc_histogram_wide", n_symbols=ns, chunks=n, chunk_symbols=L,
                 steps=a.steps, copies=int(lib.rc_histogram_wide_copies_(ns)),
                 batch_only=rates(t_b, 2), with_rows=rates(t_r, 2), ideal_bits=rates(t_i, 2),
                 counts_exact=bool(exact), ideal_bits_rel_err=abs(got - ideal) / ideal,
                 batch_only_vs_8bit=round(t_b and base["batch_only"]["ms"] / t_b, 4),
                 with_rows_vs_8bit=round(t_r and base["with_rows"]["ms"] / t_r, 4))
        print(json.dumps(r), flush=True)
        results.append(r)
        w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    good = all(r["counts_exact"] for r in results) and all(
        r.get("ideal_bits_rel_err", 0.0) < 1e-9 for r in results)
    sys.exit(0 if good else 3)


if __name__ == "__main__":
    main()
