#!/usr/bin/env python3
"""The wide batch coders (16-bit symbols, one static table of up to 4096 symbols) beside the
single-table 8-bit static coders, in one process: HIP-event times of encode and decode, warm-up
as in tools/kbench.py, the round trip checked.  Run by hand, not by a test.

  python3 tools/kbench_wide.py --chunks 65536 --chunk-symbols 16384 --n 256 1024 4096 --out FILE

Symbols: Zipf(1.2) over n symbols, quantised to a total of 65536 with every c >= 1
(rc_quantize_counts_wide), drawn in HBM through the table's inverse CDF.  The yardstick is the
8-bit static coder on the n = 256 symbol values as bytes (the same table, the same symbols).
Algorithmic bytes count 2 B per wide symbol.  Prints one JSON line per n and one for the
yardstick; --out also writes them as a JSON list."""
import argparse
import ctypes
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
    ctx = rc.default_context(0)
    n, L = a.chunks, a.chunk_symbols
    dev = torch.device("cuda", 0)
    total = 65536
    syms = torch.empty(n * L, dtype=torch.int16, device=dev)
    dec = torch.empty(n * L, dtype=torch.int16, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cap = rc.slot_capacity(L, 16.0, slack=1.02)  # (every c >= 1 of 65536: 16 bits at most)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

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

    def timed(name, enc, dcd, src, dst, sym_bytes, extra):
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
            ok = ok and torch.equal(dst[i:i + (1 << 30)], src[i:i + (1 << 30)])
        code = int(ol.sum())
        alg = sym_bytes * n * L + code
        res = dict(coder=name, chunks=n, chunk_symbols=L, steps=a.steps, table_total=total,
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
    # the yardstick: the n = 256 symbol values as bytes through the 8-bit static coders
    c, cum, _ = zipf_table(rc, 256)
    fill(c, 0x5EED0100)
    syms8 = syms.to(torch.uint8)
    dec8 = torch.empty_like(syms8)
    m = rc.StaticModel(c, cum, total, ctx=ctx)
    base = timed("static", lambda: rc.encode_batch(m, syms8, so, out, oo, ol, fe),
                 lambda: rc.decode_batch(m, out, co, ol, dec8, so, fd), syms8, dec8, 1, {})
    results.append(base)
    del dec8
    plan = ctypes.c_uint32 * 8
    for ns in a.n:
        c, cum, _ = zipf_table(rc, ns)
        if ns != 256:
            fill(c, 0x5EED0000 + ns)
        w = rc.WideStaticModel(c, cum, total, ctx=ctx)
        pl = plan()
        ctx._lib.rc_model_wide_plan_(ns, total, pl)
        extra = dict(n_symbols=ns, plan=dict(zip(("enc_lanes", "enc_lds", "enc_layout", "enc_tab",
                                                  "dec_lanes", "dec_lds", "dec_bits", "dec_shift"),
                                                 [int(v) for v in pl])))
        # a scratch build with -DRC_WIDE_STATS (RC_LIB_PATH) counts the decoder's walk branches
        stats = getattr(ctx._lib, "rc_wide_stats_read_", None)
        st = (ctypes.c_uint64 * 2)()
        if stats is not None:
            stats(st)  # (reading clears the counters)
        r = timed("wide", lambda: rc.encode_batch_wide(w, syms, so, out, oo, ol, fe),
                  lambda: rc.decode_batch_wide(w, out, co, ol, dec, so, fd), syms, dec, 2, extra)
        if stats is not None and stats(st) == 0 and st[0]:
            r["walk_branch_share"] = round(st[1] / st[0], 5)
        r["encode_vs_static"] = round(r["encode_gsym_s"] / base["encode_gsym_s"], 4)
        r["decode_vs_static"] = round(r["decode_gsym_s"] / base["decode_gsym_s"], 4)
        print(json.dumps(dict(n_symbols=ns, encode_vs_static=r["encode_vs_static"],
                              decode_vs_static=r["decode_vs_static"])), flush=True)
        results.append(r)
        w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["bit_exact_round_trip"] for r in results) else 3)


if __name__ == "__main__":
    main()
