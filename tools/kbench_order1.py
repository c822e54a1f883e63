#!/usr/bin/env python3
"""The order-1 batch coders (the previous symbol picks the row of a static model set) beside the
indexed coders on the same symbols, in one process: HIP-event times of encode and decode,
warm-up as in tools/kbench.py, the round trip checked.  Run by hand, not by a test.

  python3 tools/kbench_order1.py --chunks 65536 --chunk-bytes 16384 --k 1 8 64 --out FILE

Symbols: a K-state Markov source whose rows are the set's rows, generated in HBM (one vectorised
step per symbol position over all chunks): row j is the Zipf(1.2) table over 256 symbols rotated
by j * 256 / K, the context map sends symbol s to row s * K >> 8, and every chunk starts in row
0.  The data therefore has exactly the order-1 structure the model describes and the coded size
is that of the source.  The yardstick is the indexed coders on the same symbols, given the
derived index stream (idx[i] = map[sym[i-1]]) precomputed in HBM: the same rows, the same
arithmetic, the same bytes out; the order-1 encoder reads one byte per symbol less, and the
order-1 decoder must find each row from the symbol before instead of prefetching it.  Prints one
JSON line per coder and K; --out also writes them as a JSON list."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def markov_fill(torch, rows, ctx_map, first_row, n, L, seed, dev):
    """n chunks of L symbols of the chain (rows: K x 256 counts of one total 65536)."""
    K = rows.shape[0]
    inv = np.zeros((K, 65536), np.uint8)  # inverse CDFs
    for j in range(K):
        inv[j] = np.repeat(np.arange(256, dtype=np.uint8), rows[j])
    inv_d = torch.from_numpy(inv).to(dev).view(-1)
    map_d = torch.from_numpy(ctx_map.astype(np.int64) << 16).to(dev)  # premultiplied row offsets
    g = torch.Generator(device=dev).manual_seed(seed)
    cols = torch.empty((L, n), dtype=torch.uint8, device=dev)
    row = torch.full((n,), int(first_row) << 16, dtype=torch.int64, device=dev)
    for i in range(L):
        u = torch.randint(0, 65536, (n,), dtype=torch.int64, device=dev, generator=g)
        s = inv_d[row + u]
        cols[i] = s
        row = map_d[s.long()]
    return cols.t().contiguous().view(-1)


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
    assert total == 65536
    dev = torch.device("cuda", 0)
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    # a rotated row prices the symbols at up to log2(total / min c) bits
    cap = rc.slot_capacity(L, float(np.log2(total / float(c.min()))), slack=1.02)
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    oo = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    co = oo[:-1].contiguous()
    ol = torch.zeros(n, dtype=torch.int64, device=dev)
    fe = torch.zeros(n, dtype=torch.int32, device=dev)
    fd = torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(name, syms, enc, dcd, idx_bytes, extra):
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
        tes = [x.elapsed_time(y) for x, y, _ in ev]
        tds = [y.elapsed_time(z) for _, y, z in ev]
        te, td = float(np.mean(tes)), float(np.mean(tds))
        ok = int(fe.abs().sum()) == 0 and int(fd.abs().sum()) == 0
        for i in range(0, n * L, 1 << 30):
            ok = ok and torch.equal(dec[i:i + (1 << 30)], syms[i:i + (1 << 30)])
        code = int(ol.sum())
        alg = n * L + code + idx_bytes  # symbols, code, and the index byte per symbol if any
        res = dict(coder=name, chunks=n, chunk_bytes=L, steps=a.steps, table_total=int(total),
                   encode_ms=round(te, 3), decode_ms=round(td, 3),
                   encode_ms_steps=[round(t, 3) for t in tes],
                   decode_ms_steps=[round(t, 3) for t in tds],
                   encode_gsym_s=round(n * L / te / 1e6, 3),
                   decode_gsym_s=round(n * L / td / 1e6, 3),
                   bytes_per_symbol=round(code / (n * L), 5), alg_bytes=alg,
                   encode_alg_gb_s=round(alg / te / 1e6, 2),
                   decode_alg_gb_s=round(alg / td / 1e6, 2), bit_exact_round_trip=bool(ok))
        res.update(extra)
        print(json.dumps(res), flush=True)
        dec.zero_()
        return res

    results = []
    plan = ctypes.c_uint32 * 8
    keys = ("enc_lanes", "enc_lds", "enc_layout", "enc_tab", "dec_lanes", "dec_lds", "dec_bits",
            "dec_shift")
    for K in a.k:
        rows = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // K) for j in range(K)])
        ctx_map = ((np.arange(256) * K) >> 8).astype(np.uint8)
        syms = markov_fill(torch, rows, ctx_map, 0, n, L, 0x01D0C5EED + K, dev)
        # the derived index stream, for the yardstick
        idx = torch.from_numpy(ctx_map).to(dev)[syms.long()].view(n, L).roll(1, dims=1)
        idx[:, 0] = 0
        idx = idx.reshape(-1).contiguous()
        mset = rc.StaticModelSet(rows, None, total, ctx=ctx)
        o1 = rc.Order1ModelSet(rows, None, total, ctx_map=ctx_map, first_row=0, ctx=ctx)
        pl = plan()
        ctx._lib.rc_model_set_plan_(K, total, pl)
        base = timed("indexed", syms,
                     lambda: rc.encode_batch_indexed(mset, syms, idx, so, out, oo, ol, fe),
                     lambda: rc.decode_batch_indexed(mset, out, co, ol, idx, dec, so, fd), n * L,
                     dict(k=K, plan=dict(zip(keys, [int(v) for v in pl]))))
        want_len = ol.clone()
        ctx._lib.rc_model_order1_plan_(K, total, pl)
        r = timed("order1", syms, lambda: rc.encode_batch_order1(o1, syms, so, out, oo, ol, fe),
                  lambda: rc.decode_batch_order1(o1, out, co, ol, dec, so, fd), 0,
                  dict(k=K, plan=dict(zip(keys, [int(v) for v in pl]))))
        r["same_lengths_as_indexed"] = bool(torch.equal(ol, want_len))
        r["encode_vs_indexed"] = round(r["encode_gsym_s"] / base["encode_gsym_s"], 4)
        r["decode_vs_indexed"] = round(r["decode_gsym_s"] / base["decode_gsym_s"], 4)
        print(json.dumps(dict(k=K, encode_vs_indexed=r["encode_vs_indexed"],
                              decode_vs_indexed=r["decode_vs_indexed"])), flush=True)
        results += [base, r]
        mset.close()
        o1.close()
        del syms, idx
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["bit_exact_round_trip"] and r.get("same_lengths_as_indexed", True)
                      for r in results) else 3)


if __name__ == "__main__":
    main()
