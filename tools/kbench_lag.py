#!/usr/bin/env python3
"""The lagged order-1 coders (rc_model_create_order1_set_lagged: the context is the symbol D
positions back) beside the lag-1 coders of the same K and P fitted on the same symbols, in one
process: HIP-event times of encode and decode as alternated pairs, warm-up as in tools/kbench.py,
the round trip checked; and rc_histogram_pairs_lagged beside rc_histogram_pairs_periodic.  Run by
hand, not by a test.

  python3 tools/kbench_lag.py --source walk --chunks 65536 --chunk-bytes 16384 --k 8 --out FILE

Symbols: 2^18 bytes of records, tiled in HBM to chunks x chunk-bytes symbols (chunk-bytes divides
2^18, so every chunk starts on a record):
  walk   int32 random walk, cumsum(integers(-50, 51, 2^16)), period 4, lag 4
  bf16   the top 16 bits of float32 sin(t / 300) + 0.05 normal, 2^17 values, period 2, lag 2
both from numpy default_rng(1), little-endian.  Both sets are fitted on the
2^18 bytes as chunks of chunk-bytes (fit_order1_set, joint=True), so unlike tools/
kbench_periodic.py the two code different bytes: the yardstick is what a user of lag 1 gets today
at the same K and P.  Prints one JSON line; --out also writes it as a JSON list."""
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
BASE = 1 << 18


def source_bytes(kind):
    """(2^18 bytes, period = lag = the record's size)."""
    rng = np.random.default_rng(1)
    if kind == "walk":
        return np.cumsum(rng.integers(-50, 51, 2 ** 16)).astype("<i4").view(np.uint8), 4
    if kind == "bf16":
        t = np.arange(2 ** 17)
        x = (np.sin(t / 300) + 0.05 * rng.standard_normal(2 ** 17)).astype("<f4")
        return (x.view("<u4") >> 16).astype("<u2").view(np.uint8), 2
    raise ValueError(kind)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--source", choices=("walk", "bf16"), default="walk")
    p.add_argument("--chunks", type=int, default=1 << 16)
    p.add_argument("--chunk-bytes", type=int, default=16384)
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--control", action="store_true",
                   help="both sets get the lagged fit's rows under a purely positional map (row "
                        "ph mod K in phase ph, whatever the context), so both code every symbol "
                        "but a chunk's first lag - 1 with the same row: the ratio of the rates is "
                        "the kernels', not the data's")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    ctx = rc.default_context(0)
    n, L, K = a.chunks, a.chunk_bytes, a.k
    assert BASE % L == 0 and (n * L) % BASE == 0, "whole copies of the 2^18 bytes, whole chunks"
    dev = torch.device("cuda", 0)
    base_h, P = source_bytes(a.source)
    D = P
    base = torch.from_numpy(base_h.copy()).to(dev)
    bo = torch.arange(BASE // L + 1, dtype=torch.int64, device=dev) * L
    near = rc.fit_order1_set(base, bo, n_models=K, period=P, lag=1, joint=True, ctx=ctx)
    far = rc.fit_order1_set(base, bo, n_models=K, period=P, lag=D, joint=True, ctx=ctx)
    if a.control:
        pos = np.repeat((np.arange(P) % far.n_models)[:, None], 256, axis=1).astype(np.uint8)
        rows = (far.c, far.cum, far.total)
        near = rc.Order1ModelSet(*rows, ctx_map=pos, first_row=0, ctx=ctx, period=P, lag=1)
        far = rc.Order1ModelSet(*rows, ctx_map=pos, first_row=0, ctx=ctx, period=P, lag=D)
    syms = base.repeat(n * L // BASE)
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = rc.slot_capacity(L, max(near.max_bits_per_symbol(), far.max_bits_per_symbol()),
                           slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

    pl = (ctypes.c_uint32 * 8)()
    ctx._lib.rc_model_order1_plan_lagged_(far.n_models, far.total, P, D, pl)
    plan = dict(zip(KEYS, [int(v) for v in pl]))

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

    calls = [lambda: rc.encode_batch_order1(near, syms, so, out, oo, ol, fe),
             lambda: rc.decode_batch_order1(near, out, co, ol, dec, so, fd),
             lambda: rc.encode_batch_order1(far, syms, so, out, oo, ol, fe),
             lambda: rc.decode_batch_order1(far, out, co, ol, dec, so, fd)]
    # each coder alone first: its round trip and its bytes
    calls[0](), calls[1]()
    ok_near, bytes_near = checked(), int(ol.sum())
    calls[2](), calls[3]()
    ok_far, bytes_far = checked(), int(ol.sum())
    ideal_near = float(rc.ideal_bits_order1(near, base, bo).sum()) / BASE
    ideal_far = float(rc.ideal_bits_order1(far, base, bo).sum()) / BASE
    event_ms(calls, a.warmup)
    t = event_ms(calls, a.pairs)
    m = [float(np.mean(x)) for x in t]
    # the pair counts, alternated likewise
    h1 = torch.zeros((P, 256, 256), dtype=torch.int64, device=dev)
    hd = torch.zeros((P, 256, 256), dtype=torch.int64, device=dev)
    f1 = torch.zeros(256, dtype=torch.int64, device=dev)
    f2 = torch.zeros(256, dtype=torch.int64, device=dev)
    hcalls = [lambda: rc.histogram_pairs_periodic(syms, so, P, h1, f1, ctx=ctx),
              lambda: rc.histogram_pairs_periodic(syms, so, P, hd, f2, ctx=ctx, lag=D)]
    event_ms(hcalls, a.warmup)
    for x in (h1, hd, f1, f2):
        x.zero_()
    th = event_ms(hcalls, a.pairs)
    hist_ok = bool(int(hd.sum() + f2.sum()) == a.pairs * n * L == int(h1.sum() + f1.sum()))
    res = dict(source=a.source, control=bool(a.control), period=P, lag=D, k=K,
               rows_lag_1=near.n_models, rows=far.n_models, chunks=n, chunk_bytes=L, pairs=a.pairs,
               table_total=int(far.total), plan=plan,
               encode_ms_lag_1=[round(x, 3) for x in t[0]],
               decode_ms_lag_1=[round(x, 3) for x in t[1]],
               encode_ms=[round(x, 3) for x in t[2]], decode_ms=[round(x, 3) for x in t[3]],
               encode_gsym_s_lag_1=round(n * L / m[0] / 1e6, 3),
               decode_gsym_s_lag_1=round(n * L / m[1] / 1e6, 3),
               encode_gsym_s=round(n * L / m[2] / 1e6, 3),
               decode_gsym_s=round(n * L / m[3] / 1e6, 3),
               encode_vs_lag_1=round(m[0] / m[2], 4), decode_vs_lag_1=round(m[1] / m[3], 4),
               bytes_per_symbol_lag_1=round(bytes_near / (n * L), 5),
               bytes_per_symbol=round(bytes_far / (n * L), 5),
               bytes_vs_lag_1=round(bytes_far / bytes_near, 4),
               ideal_bits_per_symbol_lag_1=round(ideal_near, 4),
               ideal_bits_per_symbol=round(ideal_far, 4),
               bit_exact_round_trip=bool(ok_near and ok_far),
               histogram_pairs_periodic_ms=[round(x, 3) for x in th[0]],
               histogram_pairs_lagged_ms=[round(x, 3) for x in th[1]],
               histogram_time_ratio=round(float(np.mean(th[1]) / np.mean(th[0])), 3),
               histogram_sums_agree=hist_ok)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([res], f, indent=1)
            f.write("\n")
    sys.exit(0 if res["bit_exact_round_trip"] and res["histogram_sums_agree"] else 3)


if __name__ == "__main__":
    main()
