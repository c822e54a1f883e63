#!/usr/bin/env python3
"""The RCB2 container's new work beside its yardsticks, in one process on the same bytes:
HIP-event times for the kernels, wall-clock (synchronised) times for the codec calls.  Run by
hand, not by a test.

  python3 tools/kbench_container2.py --out profiles/container2/kbench_container2.json

Symbols: the K = 8 Markov source of tools/kbench_order1.py, generated in HBM.

Checksum.  rc_checksum_batch (k_chunk_checksum) over --bytes symbols cut into 16-KiB and 4-KiB
chunks, in TB/s of symbols read.  The yardstick is rc_histogram (batch counts) on the same bytes
in the same process, alternated with it; for scale also rc_container_pack of as many stream
bytes (k_pack_payload reads and writes each byte: its rate counts both).  A few chunks'
checksums are compared with the numpy definition (tests/container2_ref.py).

Codec.  compress / decompress end to end on --codec-symbols symbols in 64-KiB chunks: order 0,
order 1 with the set fitted by compress (K <= 8) and order 1 with that set given, each with and
without checksums: container bytes per symbol and Gsym/s of the whole call.  Prints one JSON
line per measurement; --out also writes them as a JSON list."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bytes", type=int, default=1 << 30)
    p.add_argument("--chunk-bytes", type=int, nargs="*", default=[16384, 4096])
    p.add_argument("--codec-symbols", type=int, default=1 << 28)
    p.add_argument("--pairs", type=int, default=5, help="alternated (histogram, checksum) pairs")
    p.add_argument("--steps", type=int, default=3, help="timed runs of the other measurements")
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import range_coder_rust_amd as rc
    from range_coder_rust_amd import _native as N
    from range_coder_rust_amd import container as C
    from range_coder_rust_amd import synth
    from range_coder_rust_amd.api import _ptr
    from kbench_order1 import markov_fill
    import container2_ref as R
    ctx = rc.default_context(0)
    lib = ctx._lib
    dev = torch.device("cuda", 0)
    c, cum, total = synth.zipf_table()
    rows8 = np.stack([np.roll(np.asarray(c, np.uint32), (j * 256) // 8) for j in range(8)])
    map8 = ((np.arange(256) * 8) >> 8).astype(np.uint8)
    results = []
    good = True

    def ok(st):
        assert st == N.RC_OK, st

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def emit(**kw):
        if "ms" in kw:
            kw["ms_mean"] = round(float(np.mean(kw["ms"])), 3)
            kw["ms"] = [round(t, 3) for t in kw["ms"]]
        print(json.dumps(kw), flush=True)
        results.append(kw)
        return kw

    # ---- the checksum kernel beside the histogram and the payload gather ----
    ctx.bind_stream()
    for L in a.chunk_bytes:
        n = a.bytes // L
        syms = markov_fill(torch, rows8, map8, 0, n, L, 0x01D0C5EED + 8, dev)
        so = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
        sums = torch.zeros(n, dtype=torch.int32, device=dev)
        hist = torch.zeros(256, dtype=torch.int64, device=dev)
        fh = lambda: ok(lib.rc_histogram(ctx.handle, _ptr(syms), _ptr(so), n, None, _ptr(hist)))
        fc = lambda: ok(lib.rc_checksum_batch(ctx.handle, _ptr(syms), _ptr(so), n, 1, _ptr(sums)))
        for _ in range(a.warmup):
            fh()
            fc()
        torch.cuda.synchronize()
        th, tc = [], []
        for _ in range(a.pairs):
            th.append(once(fh))
            tc.append(once(fc))
        h = sums.cpu().numpy().view(np.uint32)
        same = all(int(h[k]) == R.checksum(syms[k * L:(k + 1) * L].cpu().numpy())
                   for k in (0, 1, n // 2, n - 1))
        good = good and same
        tb = lambda t: round(n * L / float(np.mean(t)) / 1e9, 3)
        emit(what="rc_histogram", chunks=n, chunk_bytes=L, ms=th, tb_s=tb(th))
        emit(what="rc_checksum_batch", chunks=n, chunk_bytes=L, ms=tc, tb_s=tb(tc),
             matches_numpy=same, of_histogram=round(float(np.mean(th) / np.mean(tc)), 3))
        # the payload gather on as many stream bytes (whole rc_container_pack call: two scans,
        # the gather, two waits)
        m = rc.StaticModel(c, cum, total, ctx=ctx)
        ln = torch.full((n,), L, dtype=torch.int64, device=dev)
        size = ctypes.c_uint64()
        lib.rc_container_pack(ctx.handle, m.handle, _ptr(syms), _ptr(so), _ptr(ln), _ptr(so), n,
                              None, 0, ctypes.byref(size))
        dst = torch.empty(size.value, dtype=torch.uint8, device=dev)
        fp = lambda: ok(lib.rc_container_pack(ctx.handle, m.handle, _ptr(syms), _ptr(so), _ptr(ln),
                                              _ptr(so), n, _ptr(dst), dst.numel(),
                                              ctypes.byref(size)))
        for _ in range(a.warmup):
            fp()
        tp = [once(fp) for _ in range(a.steps)]
        emit(what="rc_container_pack", chunks=n, chunk_bytes=L, ms=tp,
             tb_s_read_plus_write=round(2 * n * L / float(np.mean(tp)) / 1e9, 3))
        del syms, so, sums, dst, ln

    # ---- the codec end to end ----
    L = 65536
    n = max(a.codec_symbols // L, 1)
    syms = markov_fill(torch, rows8, map8, 0, n, L, 0x01D0C5EED + 9, dev)
    fitted = {}

    def codec(name, **kw):
        nonlocal good
        for _ in range(a.warmup):
            blob = rc.compress(syms, chunk_size=L, **kw)
            rc.decompress(blob)
        tcs, tds = [], []
        for _ in range(a.steps):
            t, blob = wall(lambda: rc.compress(syms, chunk_size=L, **kw))
            tcs.append(t)
            t, out = wall(lambda: rc.decompress(blob))
            tds.append(t)
        back = bool(torch.equal(out, syms))
        good = good and back
        inf = C.info(blob)
        if name == "order1_fit":
            fitted["model"] = C.model_of(blob, inf, ctx)
        emit(what="codec_" + name, symbols=n * L, chunk_bytes=L, kind=int(inf.kind),
             n_models=int(getattr(inf, "n_models", 0)), checksums=bool(kw.get("checksum", False)),
             container_bytes=int(blob.numel()),
             bytes_per_symbol=round(blob.numel() / (n * L), 5), round_trip=back,
             compress_ms=[round(t, 2) for t in tcs], decompress_ms=[round(t, 2) for t in tds],
             compress_gsym_s=round(n * L / float(np.mean(tcs)) / 1e6, 2),
             decompress_gsym_s=round(n * L / float(np.mean(tds)) / 1e6, 2))

    codec("order0")
    codec("order0_checksum", checksum=True)
    codec("order1_fit", order=1, n_models=8)
    codec("order1_given", model=fitted["model"])
    codec("order1_given_checksum", model=fitted["model"], checksum=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    sys.exit(0 if good else 3)


if __name__ == "__main__":
    main()
