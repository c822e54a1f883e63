#!/usr/bin/env python3
"""Fitting an order-1 set (rc_histogram_pairs, rc_ideal_bits_order1) beside what the library
already had, in one process on the same symbols: HIP-event times, warm-up as in tools/kbench.py.
Run by hand, not by a test.

  python3 tools/kbench_order1_fit.py --chunks 65536 --chunk-bytes 16384 --out FILE

Symbols: the K = 8 Markov source of tools/kbench_order1.py, generated in HBM.

Pair counts.  The yardstick is a composition of the existing kernel: five calls of
rc_histogram_order1 with K = 64, call q giving the contexts 63 q .. 63 q + 62 a row of their own
and every other context (and the chunks' first symbols) the dump row 63; the five results hold
every pair count.  Composition and rc_histogram_pairs are timed as alternated pairs, and the new
kernel is worth keeping only if every one of its runs is faster than every run of the
composition (`every_run_faster`).  The two results are compared count by count.  For scale:
rc_histogram (batch counts) and one rc_histogram_order1 call (K = 64, map s >> 2).

Ideal bits.  rc_ideal_bits_order1 under sets of K = 1, 8 and 64 rows beside rc_ideal_bits_wide at
n = 256 on the same symbols widened to 16 bits (--period P: the sets are periodic, with P copies
of the map as their slices, so the periodic kernel sums the same bits).  Both calls read their table back and wait for
the stream, so the times are of the whole call.  Prints one JSON line per measurement; --out also
writes them as a JSON list."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=1 << 16)
    p.add_argument("--chunk-bytes", type=int, default=16384)
    p.add_argument("--pairs", type=int, default=5, help="alternated (composition, new) pairs")
    p.add_argument("--steps", type=int, default=3, help="timed runs of the other measurements")
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--k", type=int, nargs="*", default=[1, 8, 64], help="ideal bits: set sizes")
    p.add_argument("--period", type=int, default=1,
                   help="ideal bits: the sets' period (> 1: every slice the same map)")
    p.add_argument("--label", default=None, help="copied into every result (build variant)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    from range_coder_rust_amd import _native as N
    from range_coder_rust_amd import model_build as mb
    from range_coder_rust_amd import synth
    from range_coder_rust_amd.api import _ptr
    from kbench_order1 import markov_fill
    ctx = rc.default_context(0)
    lib = ctx._lib
    n, L = a.chunks, a.chunk_bytes
    dev = torch.device("cuda", 0)
    c, _, total = synth.zipf_table()

    def source(K):
        rows = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // K) for j in range(K)])
        return rows, ((np.arange(256) * K) >> 8).astype(np.uint8)

    rows8, map8 = source(8)
    syms = markov_fill(torch, rows8, map8, 0, n, L, 0x01D0C5EED + 8, dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    ctx.bind_stream()
    results = []

    def ok(st):
        assert st == N.RC_OK, st

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def emit(**kw):
        kw.update(chunks=n, chunk_bytes=L)
        if a.label:
            kw["label"] = a.label
        if "ms" in kw:
            kw["ms_mean"] = round(float(np.mean(kw["ms"])), 3)
            kw["gsym_s"] = round(n * L / float(np.mean(kw["ms"])) / 1e6, 2)
            kw["ms"] = [round(t, 3) for t in kw["ms"]]
        print(json.dumps(kw), flush=True)
        results.append(kw)
        return kw

    # ---- pair counts: the composition of the existing kernel against the new one ----
    comp_maps = []
    for q in range(5):
        m = np.full(256, 63, np.uint8)
        own = np.arange(63 * q, min(63 * q + 63, 256))
        m[own] = (own - 63 * q).astype(np.uint8)
        comp_maps.append(m)
    comp_hist = torch.zeros((5, 64, 256), dtype=torch.int64, device=dev)
    pair = torch.zeros((256, 256), dtype=torch.int64, device=dev)
    first = torch.zeros(256, dtype=torch.int64, device=dev)

    def composition():
        for q in range(5):
            ok(lib.rc_histogram_order1(ctx.handle, 64, ctypes.c_void_p(comp_maps[q].ctypes.data),
                                       63, _ptr(syms), _ptr(so), n, _ptr(comp_hist[q])))

    def new():
        ok(lib.rc_histogram_pairs(ctx.handle, _ptr(syms), _ptr(so), n, _ptr(pair), _ptr(first)))

    for _ in range(a.warmup):
        composition()
        new()
    torch.cuda.synchronize()
    comp_hist.zero_()
    pair.zero_()
    first.zero_()
    t_comp, t_new = [], []
    for _ in range(a.pairs):
        t_comp.append(once(composition))
        t_new.append(once(new))
    want = torch.cat([comp_hist[q, :63] for q in range(5)])[:256]
    same = bool(torch.equal(want, pair))
    firsts_ok = int(first.sum()) == a.pairs * n and int(pair.sum()) == a.pairs * n * (L - 1)
    emit(what="pairs_composition_5x_histogram_order1_k64", ms=t_comp)
    emit(what="rc_histogram_pairs", ms=t_new, same_counts_as_composition=same,
         totals_ok=firsts_ok, every_run_faster=bool(max(t_new) < min(t_comp)),
         speedup_mean=round(float(np.mean(t_comp) / np.mean(t_new)), 3))
    good = same and firsts_ok

    # ---- for scale: the order-0 histogram and one call of the existing kernel ----
    hist0 = torch.zeros(256, dtype=torch.int64, device=dev)
    h0 = lambda: ok(lib.rc_histogram(ctx.handle, _ptr(syms), _ptr(so), n, None, _ptr(hist0)))
    map64 = (np.arange(256) >> 2).astype(np.uint8)
    hist64 = torch.zeros((64, 256), dtype=torch.int64, device=dev)
    h1 = lambda: ok(lib.rc_histogram_order1(ctx.handle, 64, ctypes.c_void_p(map64.ctypes.data), 0,
                                            _ptr(syms), _ptr(so), n, _ptr(hist64)))
    for name, fn in (("rc_histogram", h0), ("rc_histogram_order1_k64", h1)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        emit(what=name, ms=[once(fn) for _ in range(a.steps)])

    # ---- ideal bits: order-1 sets of K rows against the wide model on the widened symbols ----
    if a.k:
        bits = torch.empty(n, dtype=torch.float64, device=dev)
        syms16 = syms.to(torch.int16)
        wide = rc.WideStaticModel(np.asarray(c, np.uint32), None, total, ctx=ctx)
        fw = lambda: ok(lib.rc_ideal_bits_wide(ctx.handle, wide.handle, _ptr(syms16), _ptr(so), n,
                                               _ptr(bits)))
        for _ in range(a.warmup):
            fw()
        emit(what="rc_ideal_bits_wide_n256", ms=[once(fw) for _ in range(a.steps)],
             finite=bool(torch.isfinite(bits).all()))
        del syms16
        for K in a.k:
            rows, cmap = source(K)
            if a.period > 1:
                cmap = np.tile(cmap, (a.period, 1))
            o1 = rc.Order1ModelSet(rows, None, total, ctx_map=cmap, first_row=0, ctx=ctx,
                                   period=a.period)
            fo = lambda: ok(lib.rc_ideal_bits_order1(ctx.handle, o1.handle, _ptr(syms), _ptr(so),
                                                     n, _ptr(bits)))
            for _ in range(a.warmup):
                fo()
            t = [once(fo) for _ in range(a.steps)]
            emit(what="rc_ideal_bits_order1", k=K, period=a.period, ms=t, finite=bool(torch.isfinite(bits).all()),
                 bits_per_symbol=round(float(bits.sum()) / (n * L), 5))
            o1.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if good else 3)


if __name__ == "__main__":
    main()
