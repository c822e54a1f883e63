#!/usr/bin/env python3
"""The joint device clustering (rc_cluster_contexts_dev) beside the host clustering it follows
(rc_cluster_contexts), in one process on the same counts, the two sides of every comparison
alternated.  Whole calls, wall clock (both calls return with their results on the host).  Run by
hand, not by a test.

  python3 tools/kbench_cluster.py --out profiles/joint_fit/kbench_cluster.json

(a) P = 1: the pair counts of the K = 8 Markov source of tools/kbench_order1.py, clustered into
    K = 1, 8 and 64 classes by both calls.  The host call is the yardstick, timed on counts that
    already lie in host memory (the copy it needs first is timed beside it); the device call is
    worth keeping only if every one of its runs is faster than every host run
    (`every_run_faster`).  Maps, first_row and n_models are compared.
(b) P = 2, 4, 8: the periodic pair counts of the same symbols; one device call over the 256 P + 1
    items against the P host calls with n_models // P classes that fit_order1_set(period=P) makes.
    The two do not compute the same thing; the costs of both are recorded.
(c) fit_order1_set(period=4, n_models=8) with joint=False and joint=True on 2^18 bytes of float32
    standard normals and of int32 uniform in [0, 3000), 16-KiB chunks: the time of the fit, the
    total code bytes and the ideal bits.
Prints one JSON line per measurement; --out also writes them as a JSON list."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunks", type=int, default=4096)
    p.add_argument("--chunk-bytes", type=int, default=4096)
    p.add_argument("--pairs", type=int, default=5, help="alternated (host, device) pairs")
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--k", type=int, nargs="*", default=[1, 8, 64])
    p.add_argument("--periods", type=int, nargs="*", default=[2, 4, 8])
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
    rows8 = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // 8) for j in range(8)])
    map8 = ((np.arange(256) * 8) >> 8).astype(np.uint8)
    syms = markov_fill(torch, rows8, map8, 0, n, L, 0x01D0C5EED + 8, dev)
    so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    ctx.bind_stream()
    results = []
    good = True

    def emit(**kw):
        kw.update(chunks=n, chunk_bytes=L)
        if a.label:
            kw["label"] = a.label
        for key in [k for k in kw if k.startswith("ms")]:
            kw[key + "_mean"] = round(float(np.mean(kw[key])), 3)
            kw[key] = [round(t, 3) for t in kw[key]]
        print(json.dumps(kw), flush=True)
        results.append(kw)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def host(pair_h, first_h, K):
        cm = np.zeros(256, np.uint8)
        fr, k, cost = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
        st = lib.rc_cluster_contexts(ctypes.c_void_p(pair_h.ctypes.data),
                                     ctypes.c_void_p(first_h.ctypes.data), 256, K,
                                     ctypes.c_void_p(cm.ctypes.data), ctypes.byref(fr),
                                     ctypes.byref(k), ctypes.byref(cost))
        assert st == N.RC_OK, st
        return cm, fr.value, k.value, cost.value

    def device(pair_t, first_t, P, K):
        cm = np.zeros((P, 256), np.uint8)
        fr, k, cost = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
        st = lib.rc_cluster_contexts_dev(ctx.handle, P, _ptr(pair_t), _ptr(first_t), 256, K,
                                         ctypes.c_void_p(cm.ctypes.data), ctypes.byref(fr),
                                         ctypes.byref(k), ctypes.byref(cost))
        assert st == N.RC_OK, st
        return cm, fr.value, k.value, cost.value

    # ---- (a) P = 1 ----
    pair_t, first_t = mb.histogram_pairs(syms, so, ctx=ctx)
    torch.cuda.synchronize()
    t_copy = [wall(lambda: (pair_t.cpu(), first_t.cpu()))[0] for _ in range(a.pairs)]
    pair_h = np.ascontiguousarray(pair_t.cpu().numpy(), np.uint64)
    first_h = np.ascontiguousarray(first_t.cpu().numpy(), np.uint64)
    emit(what="copy_counts_to_host", period=1, ms=t_copy)
    for K in a.k:
        for _ in range(a.warmup):
            host(pair_h, first_h, K)
            device(pair_t, first_t, 1, K)
        t_h, t_d = [], []
        for _ in range(a.pairs):
            th, rh = wall(lambda: host(pair_h, first_h, K))
            td, rd = wall(lambda: device(pair_t, first_t, 1, K))
            t_h.append(th)
            t_d.append(td)
        same = bool(np.array_equal(rh[0], rd[0][0]) and rh[1:3] == rd[1:3])
        good &= same
        emit(what="cluster_p1", k=K, ms_host=t_h, ms_dev=t_d, same_map=same,
             cost_rel_diff=abs(rh[3] - rd[3]) / max(rh[3], 1e-300),
             every_run_faster=bool(max(t_d) < min(t_h)),
             speedup_mean=round(float(np.mean(t_h) / np.mean(t_d)), 2))

    # ---- (b) P = 2, 4, 8 ----
    for P in a.periods:
        pp_t, pf_t = mb.histogram_pairs_periodic(syms, so, P, ctx=ctx)
        torch.cuda.synchronize()
        pp_h = np.ascontiguousarray(pp_t.cpu().numpy(), np.uint64)
        pf_h = np.ascontiguousarray(pf_t.cpu().numpy(), np.uint64)
        zero = np.zeros(256, np.uint64)

        def per_phase(K):
            return [host(pp_h[ph], pf_h if ph == 0 else zero, K // P) for ph in range(P)]

        for K in [k for k in a.k if k >= P]:
            for _ in range(a.warmup):
                device(pp_t, pf_t, P, K)
            t_h, t_d = [], []
            for _ in range(a.pairs):
                th, rh = wall(lambda: per_phase(K))
                td, rd = wall(lambda: device(pp_t, pf_t, P, K))
                t_h.append(th)
                t_d.append(td)
            emit(what="cluster_periodic", period=P, k=K, ms_host_p_calls=t_h, ms_dev=t_d,
                 rows_host=int(sum(r[2] for r in rh)), rows_dev=int(rd[2]),
                 cost_host=float(sum(r[3] for r in rh)), cost_dev=float(rd[3]),
                 every_run_faster=bool(max(t_d) < min(t_h)),
                 speedup_mean=round(float(np.mean(t_h) / np.mean(t_d)), 2))

    # ---- (c) the fit ----
    def coded_bytes(o1, s, off, Lc):
        m = off.numel() - 1
        cap = rc.slot_capacity(Lc, 17.0)
        out_off = torch.arange(m + 1, dtype=torch.int64, device=dev) * cap
        out = torch.zeros(m * cap, dtype=torch.uint8, device=dev)
        out_len, fl = rc.encode_batch_order1(o1, s, off, out, out_off)
        dec = torch.zeros_like(s)
        fd = rc.decode_batch_order1(o1, out, out_off[:-1].contiguous(), out_len, dec, off)
        torch.cuda.synchronize()
        ok = int(fl.abs().sum()) == 0 and int(fd.abs().sum()) == 0 and bool(torch.equal(dec, s))
        return int(out_len.sum()), ok

    rng = np.random.default_rng(7)
    inputs = {"float32": rng.standard_normal(1 << 16).astype(np.float32).view(np.uint8)}
    rng = np.random.default_rng(7)
    inputs["int32"] = rng.integers(0, 3000, 1 << 16).astype(np.int32).view(np.uint8)
    for kind, b in inputs.items():
        s = torch.from_numpy(b.copy()).to(dev)
        off = torch.arange(len(b) // 16384 + 1, dtype=torch.int64, device=dev) * 16384
        fit = lambda j: mb.fit_order1_set(s, off, n_models=8, period=4, ctx=ctx, joint=j)
        for _ in range(a.warmup):
            fit(False).close()
            fit(True).close()
        t = {False: [], True: []}
        for _ in range(a.pairs):
            for j in (False, True):
                dt, m = wall(lambda: fit(j))
                t[j].append(dt)
                if len(t[j]) < a.pairs:
                    m.close()
                else:
                    nbytes, ok = coded_bytes(m, s, off, 16384)
                    ideal = float(mb.ideal_bits_order1(m, s, off).sum())
                    good &= ok
                    emit(what="fit_order1_set_p4_k8", input=kind, joint=j, ms_fit=t[j],
                         rows=int(m.n_models), code_bytes=nbytes, ideal_bits=round(ideal, 1),
                         round_trip=ok)
                    m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if good else 3)


if __name__ == "__main__":
    main()
