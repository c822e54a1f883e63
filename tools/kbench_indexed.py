#!/usr/bin/env python3
"""The indexed batch coders (a static model set, one model index per symbol) beside the
single-table static coders on the same symbols, in one process: HIP-event times of encode and
decode, warm-up as in tools/kbench.py, the round trip checked.  Run by hand, not by a test.

  python3 tools/kbench_indexed.py --chunks 65536 --chunk-bytes 16384 --k 1 8 64 --out FILE

Symbols: Zipf(1.2) over 256 symbols, generated in HBM (rc_synth_fill).  Row j of a set of K is
the Zipf(1.2) table rotated by j * 256 / K; the indexes come from a second rc_synth_fill with
another seed, mapped uniformly to 0 .. K-1.  The yardstick is the single-table coder with row 0
(at K = 1 the work is identical except for the index read).  The index byte per symbol counts
in the algorithmic bytes of both directions.  Prints one JSON line per K and one for the
yardstick; --out also writes them as a JSON list."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=1 << 16)
    p.add_argument("--chunk-bytes", type=int, default=16384)
    p.add_argument("--k", type=int, nargs="+", default=[1, 8, 64])
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    from range_coder_rust_amd import synth
    ctx = rc.default_context(0)
    n, L = a.chunks, a.chunk_bytes
    c, cum, total = synth.zipf_table()
    dev = torch.device("cuda", 0)
    syms = torch.empty(n * L, dtype=torch.uint8, device=dev)
    synth.fill(ctx, 0x5EED0001, synth.inverse_cdf(c), syms, L, n)
    idx = torch.empty(n * L, dtype=torch.uint8, device=dev)
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    # a rotated row prices the common symbols at up to log2(total / min c) bits
    cap = rc.slot_capacity(L, float(np.log2(total / float(c.min()))), slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(name, enc, dcd, idx_bytes, extra):
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
        for i in range(0, n * L, 1 << 30):
            ok = ok and torch.equal(dec[i:i + (1 << 30)], syms[i:i + (1 << 30)])
        code = int(ol.sum())
        alg = n * L + code + idx_bytes  # symbols, code, and the index byte per symbol
        res = dict(coder=name, chunks=n, chunk_bytes=L, steps=a.steps, table_total=int(total),
                   encode_ms=round(te, 3), decode_ms=round(td, 3),
                   encode_gsym_s=round(n * L / te / 1e6, 3),
                   decode_gsym_s=round(n * L / td / 1e6, 3),
                   bytes_per_symbol=round(code / (n * L), 5), alg_bytes=alg,
                   encode_alg_gb_s=round(alg / te / 1e6, 2),
                   decode_alg_gb_s=round(alg / td / 1e6, 2), bit_exact_round_trip=bool(ok))
        res.update(extra)
        print(json.dumps(res), flush=True)
        return res

    results = []
    m = rc.StaticModel(c, cum, total, ctx=ctx)
    base = timed("static", lambda: rc.encode_batch(m, syms, so, out, oo, ol, fe),
                 lambda: rc.decode_batch(m, out, co, ol, dec, so, fd), 0, {})
    results.append(base)
    plan = ctypes.c_uint32 * 8
    for K in a.k:
        rows = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // K) for j in range(K)])
        mset = rc.StaticModelSet(rows, None, total, ctx=ctx)
        inv = ((np.arange(65536, dtype=np.int64) * K) >> 16).astype(np.uint8)
        synth.fill(ctx, 0x1D0C5EED + K, inv, idx, L, n)
        pl = plan()
        ctx._lib.rc_model_set_plan_(K, total, pl)
        extra = dict(k=K, plan=dict(zip(("enc_lanes", "enc_lds", "enc_layout", "enc_tab",
                                         "dec_lanes", "dec_lds", "dec_bits", "dec_shift"),
                                        [int(v) for v in pl])))
        # a scratch build with -DRC_SET_STATS (RC_LIB_PATH) counts the decoder's fix-up branches
        stats = getattr(ctx._lib, "rc_set_stats_read_", None)
        st = (ctypes.c_uint64 * 2)()
        if stats is not None:
            stats(st)  # (reading clears the counters)
        r = timed("indexed", lambda: rc.encode_batch_indexed(mset, syms, idx, so, out, oo, ol, fe),
                  lambda: rc.decode_batch_indexed(mset, out, co, ol, idx, dec, so, fd), n * L,
                  extra)
        if stats is not None and stats(st) == 0 and st[0]:
            r["fixup_branch_share"] = round(st[1] / st[0], 5)
        r["encode_vs_static"] = round(r["encode_gsym_s"] / base["encode_gsym_s"], 4)
        r["decode_vs_static"] = round(r["decode_gsym_s"] / base["decode_gsym_s"], 4)
        print(json.dumps(dict(k=K, encode_vs_static=r["encode_vs_static"],
                              decode_vs_static=r["decode_vs_static"])), flush=True)
        results.append(r)
        mset.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["bit_exact_round_trip"] for r in results) else 3)


if __name__ == "__main__":
    main()
