"""Scratch RC_RING_GUARD builds of librc_amd.so (part 3).

RC_RING_GUARD makes k_decode_static flag a chunk (RC_F_RING_GUARD = 0x100, scratch builds only)
when a symbol's no_carry_expansion bytes or a range_reduction_expansion byte lie past the bytes
its code ring has staged (rc_decode.inc dec_apply / dec_rare): the read would have taken stale
ring bytes from 64 B earlier.

    python tools/ring_guard.py build      # CPU, after build(): variants/librc_guard.so,
                                          # librc_guard_wide1.so, librc_guard_span16.so
    python tools/ring_guard.py probe      # GPU: the guard fires where the ring does run short
    python tools/ring_guard.py probe_tight span16|guard|shipped   # GPU: the tight streams

* variants/librc_guard.so: the shipped ring needs plus the guard.  Run the GPU parity tests with
  RC_LIB_PATH pointing at it: any guard hit makes a chunk's flags non-zero, which those tests
  assert against the oracle's (zero) flags.
* variants/librc_guard_wide1.so: the guard plus a ring need cut to 1 byte for wide models
  (DEC_NEED_WIDE=1, so the decoder may read past its ring).  `probe` decodes wide streams that
  settle 3 bytes per symbol with it and reports how many chunks the guard flagged, and that
  every chunk decoded wrong was flagged (the guard sees the under-runs that happen).
* variants/librc_guard_span16.so: the guard plus DEC_NEED_SPAN cut from 24 to 16 in all four
  static-model decoders (rc_decode.inc allows the override for guard builds; the families take
  the same macro).  `probe_tight span16` runs the decodes of tests/test_gpu_ring.py and
  tests/test_gpu_ring_families.py on the tight streams (tests/golden/ring_tight.json) and on the
  older ring fixtures against it and reports, per decoder, how many chunks the guard flagged, how
  many decoded wrong, and whether the flagged ones are those tests/ring_sim.py's replay of that
  decoder's schedule predicts (the check that the schedules were read off the kernels
  correctly).  `probe_tight guard` and `probe_tight shipped` do the same against the shipped
  needs, with and without the guard: nothing may be flagged or wrong.  Each run adds its part to
  profiles/ring_tight/mutants.json.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GUARD = os.path.join(ROOT, "variants", "librc_guard.so")
WIDE1 = os.path.join(ROOT, "variants", "librc_guard_wide1.so")
SPAN16 = os.path.join(ROOT, "variants", "librc_guard_span16.so")
MUTANTS = os.path.join(ROOT, "profiles", "ring_tight", "mutants.json")
DECODERS = ["rc_decode_pow2.hip", "rc_decode_magic.hip", "rc_indexed.hip", "rc_order1.hip",
            "rc_order1_lag2.hip", "rc_order1_lag4.hip", "rc_order1_lag8.hip", "rc_wide.hip"]
F_RING_GUARD = 0x100


def build():
    import __graft_entry__ as g
    g.build_variant(GUARD, ["-DRC_RING_GUARD"])
    g.build_variant(WIDE1, ["-DRC_RING_GUARD", "-DDEC_NEED_WIDE=1u"])
    g.build_variant(SPAN16, ["-DRC_RING_GUARD", "-DDEC_NEED_SPAN=16u"], only=DECODERS)


def probe():
    import numpy as np
    os.environ["RC_LIB_PATH"] = WIDE1
    import torch
    import range_coder_rust_amd as rc
    from oracle import cpu
    from gpu_helpers import run_decode

    rc.default_context(0)
    rng = np.random.default_rng(4)
    out = {}
    for total in (1 << 24, 1 << 20):
        c = np.ones(256, np.uint32)
        c[0] = total - 255
        cum = np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.uint32)
        m = rc.StaticModel(c, cum, total)
        lens = [int(x) for x in rng.integers(200, 3000, 512)]
        chunks = [rng.integers(1, 256, L).astype(np.uint8) for L in lens]
        codes = [cpu.encode(c, cum, total, ch)[1] for ch in chunks]
        dec, fd = run_decode(m, codes, lens, misalign=True, seed=total)
        wrong = [k for k, ch in enumerate(chunks) if not (dec[k] == ch).all()]
        flagged = [k for k in range(len(chunks)) if fd[k] & F_RING_GUARD]
        out[str(total)] = dict(chunks=len(chunks), guard_flagged=len(flagged),
                               decoded_wrong=len(wrong),
                               wrong_unflagged=len(set(wrong) - set(flagged)))
        torch.cuda.synchronize()
    print(json.dumps(out))
    for v in out.values():
        assert v["guard_flagged"] > 0 and v["wrong_unflagged"] == 0, out


def probe_tight(which):
    """The decodes of the GPU ring tests, counted instead of asserted."""
    import numpy as np
    lib = dict(span16=SPAN16, guard=GUARD, shipped=None)[which]
    need_span = 16 if which == "span16" else 24
    if lib:
        os.environ["RC_LIB_PATH"] = lib
    import torch
    import range_coder_rust_amd as rc
    import ring_sim
    from gpu_helpers import dev, ring_decode_at

    here = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(here, "ring_tight.json")) as f:
        tight = json.load(f)
    with open(os.path.join(here, "ring_fixtures.json")) as f:
        old = json.load(f)
    sets = {}  # fixture set -> model name -> (c, cum, total, chunks)
    for name, md in tight["models"].items():
        sets.setdefault("tight", {})[name] = (
            np.array(md["c"], np.uint32), np.array(md["cum"], np.uint32), md["total"],
            [ch for ch in tight["chunks"] if ch["model"] == name])
    sets["old"] = {"pow2": (np.array(old["c"], np.uint32), np.array(old["cum"], np.uint32),
                            old["total"], old["chunks"])}
    for models in sets.values():
        for c, cum, total, chunks in models.values():
            for ch in chunks:
                ch["km"] = ring_sim.settle(c.tolist(), cum.tolist(), total, ch["symbols"])

    out = {}

    def count(fixture, decoder, schedule, chunks, head, s, sym_off, flags, skip=()):
        r = out.setdefault(fixture, {}).setdefault(decoder, dict(
            chunks=0, guard_flagged=0, decoded_wrong=0, wrong_unflagged=0, replay_predicts=0,
            flagged_not_predicted=0, predicted_not_flagged=0, streams_flagged=[]))
        want = np.array([ch["symbols"] for ch in chunks], s.dtype)
        got = s[sym_off[0]:sym_off[-1]].reshape(want.shape)
        for k, ch in enumerate(chunks):
            if k in skip:
                continue
            flagged = bool(flags[k] & F_RING_GUARD)
            wrong = bool((got[k] != want[k]).any()) or bool(flags[k] & ~F_RING_GUARD)
            predicted = bool(ring_sim.replay(ch["km"], ch["align"], head, need_span=need_span,
                                             schedule=schedule)[0])
            r["chunks"] += 1
            r["guard_flagged"] += flagged
            r["decoded_wrong"] += wrong
            r["wrong_unflagged"] += wrong and not flagged
            r["replay_predicts"] += predicted
            r["flagged_not_predicted"] += flagged and not predicted
            r["predicted_not_flagged"] += predicted and not flagged
            tag = [ch.get("model", "pow2"), chunks.index(ch), head]
            if flagged and tag not in r["streams_flagged"]:
                r["streams_flagged"].append(tag)

    rng = np.random.default_rng(16)
    for fixture, models in sets.items():
        for name, (c, cum, total, chunks) in models.items():
            heads = sorted({ch.get("head", 0) for ch in chunks} | {16, 48, 59})
            for pair in ("0", "6", "4", "512", "1024"):
                os.environ["RC_DEC_PAIR"] = pair
                ctx = rc.Context(0)
                m = rc.StaticModel(c, cum, total, ctx=ctx)
                for head in heads:
                    r = ring_decode_at(lambda *a: rc.decode_batch(m, *a), chunks, (64 - head) % 64)
                    count(fixture, "static", "static", chunks, head, *r)
                torch.cuda.synchronize()
                m.close()
                ctx.close()
            os.environ.pop("RC_DEC_PAIR")
            n = len(chunks[0]["symbols"])
            for K in (1, 64):
                mset = rc.StaticModelSet(np.tile(c, (K, 1)), np.tile(cum, (K, 1)), total)
                for poison in (False, True):
                    for head in heads:
                        off = (64 - head) % 64
                        idx = rng.integers(0, K, off + n * len(chunks) + 64).astype(np.uint8)
                        bad = [7] if poison else []
                        for k in bad:
                            idx[off + n * k:off + n * (k + 1)] = K
                        r = ring_decode_at(
                            lambda code, coff, clen, syms, so: rc.decode_batch_indexed(
                                mset, code, coff, clen, dev(idx), syms, so), chunks, off)
                        sch = "indexed_rolled" if poison else "indexed"
                        count(fixture, sch, sch, chunks, head, *r, skip=bad)
            for K, P in ((1, 1), (8, 1), (64, 1), (8, 2), (8, 8)):
                cm = rng.integers(0, K, (P, 256))
                o1 = rc.Order1ModelSet(np.tile(c, (K, 1)), np.tile(cum, (K, 1)), total,
                                       ctx_map=cm if P > 1 else cm[0],
                                       first_row=int(rng.integers(0, K)), period=P)
                for head in heads:
                    r = ring_decode_at(lambda *a: rc.decode_batch_order1(o1, *a), chunks,
                                       (64 - head) % 64)
                    count(fixture, "order1" if P == 1 else "order1_periodic", "order1", chunks,
                          head, *r)
            w = rc.WideStaticModel(c, cum, total)
            for head in [h for h in heads if h <= 31]:
                r = ring_decode_at(lambda *a: rc.decode_batch_wide(w, *a), chunks,
                                   (32 - head) % 32, wide=True)
                count(fixture, "wide", "wide", chunks, head, *r)
    torch.cuda.synchronize()
    res = {}
    if os.path.exists(MUTANTS):
        with open(MUTANTS) as f:
            res = json.load(f)
    res[which] = dict(library=os.path.relpath(lib, ROOT) if lib else "the shipped library",
                      need_span=need_span, guard=which != "shipped", **out)
    os.makedirs(os.path.dirname(MUTANTS), exist_ok=True)
    with open(MUTANTS, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({fx: {d: {k: v for k, v in r.items() if k != "streams_flagged"}
                           for d, r in ds.items()} for fx, ds in out.items()}, indent=1))


if __name__ == "__main__":
    {"build": build, "probe": probe, "probe_tight": lambda: probe_tight(sys.argv[2])}[sys.argv[1]]()
