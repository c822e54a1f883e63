#!/usr/bin/env python3
"""The periodic order-1 coders (rc_model_create_order1_set_periodic: the position in a record
joins the context) beside the period-1 order-1 coders on the same symbols, in one process:
HIP-event times of encode and decode as alternated pairs, warm-up as in tools/kbench.py, the
round trip checked; and rc_histogram_pairs_periodic beside rc_histogram_pairs.  Run by hand, not
by a test.

  python3 tools/kbench_periodic.py --chunks 65536 --chunk-bytes 16384 --k 8 --out FILE

Symbols: tools/kbench_order1.py's K-state Markov source (row j the Zipf(1.2) table rotated by
j * 256 / K, the map sends symbol s to row s * K >> 8), generated in HBM.  The periodic set has P
copies of that map as its slices, so the source matches both sets, both code every symbol with
the same row and write the same bytes: the ratio of the two rates is the cost of the periodic
kernels' per-lane map bases, plan (lanes, layout, buckets) and heads, and of nothing else.  The
kernels cannot tell that the slices are equal: each phase reads its own KiB of LDS.  Prints one
JSON line per period; --out also writes them as a JSON list."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEYS = ("enc_lanes", "enc_lds", "enc_layout", "enc_tab", "dec_lanes", "dec_lds", "dec_bits",
        "dec_shift")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=1 << 16)
    p.add_argument("--chunk-bytes", type=int, default=16384)
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--periods", type=int, nargs="+", default=[2, 4, 8])
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    from range_coder_rust_amd import synth
    from kbench_order1 import markov_fill
    ctx = rc.default_context(0)
    n, L, K = a.chunks, a.chunk_bytes, a.k
    c, _, total = synth.zipf_table()
    assert total == 65536
    dev = torch.device("cuda", 0)
    rows = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // K) for j in range(K)])
    ctx_map = ((np.arange(256) * K) >> 8).astype(np.uint8)
    syms = markov_fill(torch, rows, ctx_map, 0, n, L, 0x9E210D1C + K, dev)
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = rc.slot_capacity(L, float(np.log2(total / float(c.min()))), slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

    def plan_of(P):
        pl = (ctypes.c_uint32 * 8)()
        ctx._lib.rc_model_order1_plan_periodic_(K, total, P, pl)
        return dict(zip(KEYS, [int(v) for v in pl]))

    def event_ms(calls, pairs):
        """calls: functions run in this order `pairs` times, each between two events; returns
        the per-call lists of times."""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
              for _ in range(pairs)]
        torch.cuda.synchronize()
        for row in ev:
            row[0].record()
            for f, e in zip(calls, row[1:]):
                f()
                e.record()
        torch.cuda.synchronize()
        return [[row[i].elapsed_time(row[i + 1]) for row in ev] for i in range(len(calls))]

    def checked():
        ok = int(fe.abs().sum()) == 0 and int(fd.abs().sum()) == 0
        for i in range(0, n * L, 1 << 30):
            ok = ok and torch.equal(dec[i:i + (1 << 30)], syms[i:i + (1 << 30)])
        dec.zero_()
        return bool(ok)

    old = rc.Order1ModelSet(rows, None, total, ctx_map=ctx_map, first_row=0, ctx=ctx)
    results = []
    for P in a.periods:
        new = rc.Order1ModelSet(rows, None, total, ctx_map=np.tile(ctx_map, (P, 1)), first_row=0,
                                ctx=ctx, period=P)
        calls = [lambda: rc.encode_batch_order1(old, syms, so, out, oo, ol, fe),
                 lambda: rc.decode_batch_order1(old, out, co, ol, dec, so, fd),
                 lambda: rc.encode_batch_order1(new, syms, so, out, oo, ol, fe),
                 lambda: rc.decode_batch_order1(new, out, co, ol, dec, so, fd)]
        # each coder alone first: its round trip and its lengths
        calls[0](), calls[1]()
        ok_old, len_old = checked(), ol.clone()
        calls[2](), calls[3]()
        ok_new, same = checked(), bool(torch.equal(ol, len_old))
        event_ms(calls, a.warmup)
        t = event_ms(calls, a.pairs)
        m = [float(np.mean(x)) for x in t]
        # the pair counts, alternated likewise
        ph = torch.zeros((P, 256, 256), dtype=torch.int64, device=dev)
        p1 = torch.zeros((256, 256), dtype=torch.int64, device=dev)
        f1 = torch.zeros(256, dtype=torch.int64, device=dev)
        f2 = torch.zeros(256, dtype=torch.int64, device=dev)
        hcalls = [lambda: rc.histogram_pairs(syms, so, p1, f1, ctx=ctx),
                  lambda: rc.histogram_pairs_periodic(syms, so, P, ph, f2, ctx=ctx)]
        event_ms(hcalls, a.warmup)
        p1.zero_(), ph.zero_()
        th = event_ms(hcalls, a.pairs)
        hist_ok = bool(torch.equal(ph.sum(dim=0), p1))
        res = dict(period=P, k=K, chunks=n, chunk_bytes=L, pairs=a.pairs, table_total=int(total),
                   plan_period_1=plan_of(1), plan=plan_of(P),
                   encode_ms_period_1=[round(x, 3) for x in t[0]],
                   decode_ms_period_1=[round(x, 3) for x in t[1]],
                   encode_ms=[round(x, 3) for x in t[2]], decode_ms=[round(x, 3) for x in t[3]],
                   encode_gsym_s_period_1=round(n * L / m[0] / 1e6, 3),
                   decode_gsym_s_period_1=round(n * L / m[1] / 1e6, 3),
                   encode_gsym_s=round(n * L / m[2] / 1e6, 3),
                   decode_gsym_s=round(n * L / m[3] / 1e6, 3),
                   encode_vs_period_1=round(m[0] / m[2], 4),
                   decode_vs_period_1=round(m[1] / m[3], 4),
                   bytes_per_symbol=round(int(len_old.sum()) / (n * L), 5),
                   same_lengths_as_period_1=same,
                   bit_exact_round_trip=bool(ok_old and ok_new),
                   histogram_pairs_ms=[round(x, 3) for x in th[0]],
                   histogram_pairs_periodic_ms=[round(x, 3) for x in th[1]],
                   histogram_time_ratio=round(float(np.mean(th[1]) / np.mean(th[0])), 3),
                   histogram_sums_agree=hist_ok)
        print(json.dumps(res), flush=True)
        results.append(res)
        new.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["bit_exact_round_trip"] and r["same_lengths_as_period_1"] and
                      r["histogram_sums_agree"] for r in results) else 3)


if __name__ == "__main__":
    main()
