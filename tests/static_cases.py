"""The case table of the single-table static coders (tests/test_static_cases.py without a device,
tests/test_gpu_static_classes.py on one): for every class rc_model_create_static sorts a table
into, on both sides of every threshold and for totals above 2^16, a table, the class it is meant
to reach, its chunks and, where marked, its garbage streams.  Plain numpy, fixed seeds.

A case's class is what rc_model_static_plan_ must report for its table:

    class          (sm, direct, flat)  totals          decoder table
    wide_direct    (0, 1, 0)           1 .. 255        4-byte direct entries, wide arithmetic
    direct16       (1, 2, 0)           256 .. 512      16-byte direct entries
    flat           (1, 2, 1)           256, all ones   none
    direct4        (1, 1, 0)           513 .. 2048     4-byte direct entries
    small_bucket   (1, 0, 0)           2049 .. 2^15    8-byte buckets / q-to-symbol bytes
    pair_bucket    (1, 0, 0) + pair    2^15+1 .. 2^16  the same, and the pair buckets
    wide_bucket    (0, 0, 0)           above 2^16      4-byte buckets, wide arithmetic
"""
import zlib
from collections import namedtuple

import numpy as np

# (sm, direct, flat, has_pair, has_symof) of every class
CLASSES = {
    "wide_direct": (0, 1, 0, 0, 0),
    "direct16": (1, 2, 0, 0, 0),
    "flat": (1, 2, 1, 0, 0),
    "direct4": (1, 1, 0, 0, 0),
    "small_bucket": (1, 0, 0, 0, 1),
    "pair_bucket": (1, 0, 0, 1, 1),
    "wide_bucket": (0, 0, 0, 0, 0),
}
DIV_POW2, DIV_MAGIC = 0, 1
# the encoder variants: wide, small and incomplete, small and complete, flat
SMV_WIDE, SMV_INCOMPLETE, SMV_COMPLETE, SMV_FLAT = 0, 1, 2, 3
WIDE_LUT_BITS = 12  # buckets of a total > 2^16: 2^12

# every chunk length comes from here: the head, the tail and the 16-symbol phases of both kernels
LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 1000, 4099]
N_CHUNKS = 40  # per case (at most 64); every length at least once
RARE_LENGTHS = [64, 640, 4096, 4099, 1000, 127, 0] * 2
N_GARBAGE = 64

# name: the case's id; build() -> (c, total); cls: a key of CLASSES; smv: the encoder variant;
# shift: the bucket shift of a wide_bucket table (None elsewhere); kind: how chunks are drawn
# ("plain": by probability, "rare": rare-heavy, "split": around the split-seam starts);
# garbage: the case also decodes garbage and truncated streams
Case = namedtuple("Case", "name build cls smv shift kind garbage")


def seed_of(name):
    return zlib.crc32(name.encode())


def cum_of(c):
    c = np.asarray(c, dtype=np.uint64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.uint32)


def div_of(total):
    return DIV_POW2 if total & (total - 1) == 0 else DIV_MAGIC


def alloc(w, total):
    """Counts in proportion to the weights w that sum to total: 1 for every w > 0, the rest by
    floor, the remainder on the heaviest symbol.  w == 0 gives c == 0."""
    w = np.asarray(w, np.float64)
    nz = w > 0
    k = int(nz.sum())
    assert 1 <= k <= total
    c = np.zeros(len(w), np.int64)
    c[nz] = 1 + np.floor(w[nz] / w[nz].sum() * (total - k)).astype(np.int64)
    c[int(np.argmax(w))] += total - int(c.sum())
    assert c.sum() == total and (c[nz] >= 1).all() and c.max() < 1 << 32
    return c.astype(np.uint32)


def zipf_w(n):
    return 1.0 / np.arange(1, n + 1) ** 1.2


def zeros_w(name, n=200, flat=False):
    """n weights with about 30 % zeros, ending in zeros (Pareto, or nearly equal for `flat`: a
    table of high entropy, whose garbage streams run out of bytes often enough)."""
    rng = np.random.default_rng(seed_of("w:" + name))
    w = rng.uniform(0.5, 1.5, n) if flat else rng.pareto(1.1, n) + 0.05
    z = rng.random(n) < 0.3
    z[-3:] = True
    z[int(np.argmax(w))] = False
    w[z] = 0.0
    return w


def runs_table(name, n, total):
    """Runs of c = 1, 2 and 3 symbols between large ones (every 37th symbol), so that a bucket
    holds three or more symbol starts and the candidate pair misses."""
    rng = np.random.default_rng(seed_of("r:" + name))
    c = rng.choice([1, 1, 2, 3], n).astype(np.int64)
    big = np.arange(0, n, 37)
    c[big] = 0
    rest = total - int(c.sum())
    assert rest >= len(big)
    c[big] = rest // len(big)
    c[big[0]] += total - int(c.sum())
    assert c.sum() == total and c.min() >= 1
    return c.astype(np.uint32)


def rare_heavy_table(total):
    c = np.ones(256, np.int64)
    c[0] = total - 255
    return c.astype(np.uint32)


# The split seam (bucket_table in rc_kernels.hip): a bucket's second candidate is stored by its
# offset inside the bucket in 16 bits, 0xFFFF meaning "none".  In four buckets of a table whose
# buckets are wider than that, the first symbol start with c > 0 lies at offset 0xFFFE, 0xFFFF,
# 0x10000 and, behind a zero-frequency symbol at the same offset, 0xFFFE again.
SPLIT_BUCKETS = (5, 100, 1000, 3000)
SPLIT_OFFSETS = (0xFFFE, 0xFFFF, 0x10000, 0xFFFE)


def split_seam_table(total):
    """-> (c, total, near): near = the symbols on either side of the four starts."""
    shift = max(0, (total - 1).bit_length() - WIDE_LUT_BITS)
    assert shift > 16
    starts, zero_at = [0], None
    for k, (b, off) in enumerate(zip(SPLIT_BUCKETS, SPLIT_OFFSETS)):
        f = (b << shift) + off
        if k == 3:
            zero_at = len(starts)  # a symbol of c = 0 standing at the start itself
            starts.append(f)
        starts += [f, f + 3, f + 4]  # the start (c = 3), a c = 1 symbol, then a long one
    starts += [total - 700, total - 2]
    assert all(a <= b for a, b in zip(starts, starts[1:])) and starts[-1] < total
    c = np.diff(np.array(starts + [total], np.int64))
    assert c.sum() == total and (c == 0).sum() == 1 and c[zero_at] == 0
    near = [i for i in range(len(c)) if c[i] in (1, 3) or (i + 1 < len(c) and c[i + 1] in (0, 3))]
    return c.astype(np.uint32), total, [i for i in near if c[i] > 0]


def _case(name, build, cls, complete=False, shift=None, kind="plain", garbage=False):
    sm = CLASSES[cls][0]
    smv = SMV_FLAT if cls == "flat" else (SMV_COMPLETE if complete else SMV_INCOMPLETE) if sm \
        else SMV_WIDE
    return Case(name, build, cls, smv, shift, kind, garbage)


def _tab(w, total):
    return lambda: (alloc(w, total), total)


def _build_cases():
    cs = []
    # ---- below 256: the wide coder's direct table
    cs.append(_case("t1_n1", lambda: (np.array([1], np.uint32), 1), "wide_direct"))
    cs.append(_case("t2_n2", lambda: (np.array([1, 1], np.uint32), 2), "wide_direct"))
    cs.append(_case("t128_zeros", _tab(zeros_w("t128", 100), 128), "wide_direct"))
    cs.append(_case("t255_zeros", _tab(zeros_w("t255", 200, flat=True), 255), "wide_direct",
                    garbage=True))
    # ---- the 256 seam (t255_seam / t256_seam: one set of weights)
    w = zeros_w("seam256", 200)
    cs.append(_case("t255_seam", _tab(w, 255), "wide_direct"))
    cs.append(_case("t256_seam", _tab(w, 256), "direct16"))
    cs.append(_case("t256_flat", lambda: (np.ones(256, np.uint32), 256), "flat", complete=True))
    cs.append(_case("t256_not_flat",
                    lambda: (np.array([2, 0] + [1] * 254, np.uint32), 256), "direct16"))
    cs.append(_case("t257_complete", lambda: (np.array([2] + [1] * 255, np.uint32), 257),
                    "direct16", complete=True))
    # ---- the 512 seam
    w = zipf_w(256)
    cs.append(_case("t512_seam", _tab(w, 512), "direct16", complete=True))
    cs.append(_case("t513_seam", _tab(w, 513), "direct4", complete=True))
    # ---- 4-byte direct entries
    for total in (513, 1000, 2047, 2048):
        cs.append(_case(f"t{total}_zipf", _tab(zipf_w(128), total), "direct4"))
        cs.append(_case(f"t{total}_runs",
                        (lambda t: lambda: (runs_table(f"t{t}", 128, t), t))(total), "direct4"))
        cs.append(_case(f"t{total}_zeros", _tab(zeros_w(f"t{total}", 200, flat=total == 513),
                                                 total), "direct4", garbage=True))
    cs.append(_case("t2048_n1", lambda: (np.array([2048], np.uint32), 2048), "direct4"))
    cs.append(_case("t2048_n2", lambda: (np.array([2047, 1], np.uint32), 2048), "direct4"))
    # ---- the 2048 seam
    w = zipf_w(256)
    cs.append(_case("t2048_seam", _tab(w, 2048), "direct4", complete=True))
    cs.append(_case("t2049_seam", _tab(w, 2049), "small_bucket", complete=True))
    # ---- the 2^16 seam
    cs.append(_case("t65536_seam", _tab(w, 65536), "pair_bucket", complete=True))
    cs.append(_case("t65537_seam", _tab(w, 65537), "wide_bucket", shift=5))
    cs.append(_case("t131072_seam", _tab(w, 1 << 17), "wide_bucket", shift=5))
    cs.append(_case("t65537_zeros", _tab(zeros_w("t65537"), 65537), "wide_bucket", shift=5,
                    garbage=True))
    # ---- above 2^16: the wide coder's buckets, lut_shift 6, 8, 13, 17, 19 and 20
    for total, shift in (((1 << 17) + 1, 6), (1 << 20, 8), ((1 << 24) + 1, 13),
                         ((1 << 28) + 3, 17), (1 << 31, 19), ((1 << 32) - 1, 20)):
        t = f"t{total}"
        cs.append(_case(t + "_zipf", _tab(zipf_w(256), total), "wide_bucket", shift=shift))
        cs.append(_case(t + "_runs", (lambda t_, n_: lambda: (runs_table(n_, 256, t_), t_))(total, t),
                        "wide_bucket", shift=shift))
        cs.append(_case(t + "_zeros", _tab(zeros_w(t), total), "wide_bucket", shift=shift,
                        garbage=True))
        if total >= 1 << 31:
            cs.append(_case(t + "_n1", (lambda t_: lambda: (np.array([t_], np.uint32), t_))(total),
                            "wide_bucket", shift=shift))
            cs.append(_case(t + "_n2",
                            (lambda t_: lambda: (np.array([t_ - 1, 1], np.uint32), t_))(total),
                            "wide_bucket", shift=shift))
    # (weights "t131072" gave a table of so little entropy that only 7 of its 64 garbage streams
    # ran out of bytes; test_static_cases.py asks for 8)
    cs.append(_case("t131072_zeros", _tab(zeros_w("t131072b"), 1 << 17), "wide_bucket", shift=5,
                    garbage=True))
    # ---- rare-heavy above 2^16: nearly every coded symbol is c = 1
    for total, shift in (((1 << 24) + 1, 13), (1 << 31, 19), ((1 << 32) - 1, 20)):
        cs.append(_case(f"t{total}_rare", (lambda t_: lambda: (rare_heavy_table(t_), t_))(total),
                        "wide_bucket", shift=shift, kind="rare"))
    # ---- the split seam
    for total, shift in ((1 << 29, 17), ((1 << 32) - 1, 20)):
        cs.append(_case(f"t{total}_split", (lambda t_: lambda: split_seam_table(t_)[:2])(total),
                        "wide_bucket", shift=shift, kind="split"))
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
RARE_CASES = [c.name for c in CASES if c.kind == "rare"]
SPLIT_CASES = [c.name for c in CASES if c.kind == "split"]
RUNS_WIDE_CASES = [c.name for c in CASES if c.cls == "wide_bucket" and c.name.endswith("_runs")]
GARBAGE_CASES = [c.name for c in CASES if c.garbage]
# the thresholds of the classification, a case on either side, one set of weights per pair
SEAM_PAIRS = [("t255_seam", "t256_seam"), ("t512_seam", "t513_seam"),
              ("t2048_seam", "t2049_seam"), ("t65536_seam", "t65537_seam")]

_cache = {}


def table(name):
    """-> (c, cum, total) of a case, c and cum as uint32 arrays (built once; do not modify)."""
    if ("t", name) not in _cache:
        c, total = BY_NAME[name].build()
        c = np.ascontiguousarray(c, np.uint32)
        assert int(c.astype(np.uint64).sum()) == total
        _cache["t", name] = (c, cum_of(c), int(total))
    return _cache["t", name]


def _lengths(rng):
    first = list(rng.permutation(LENGTHS))
    return [int(x) for x in first + list(rng.choice(LENGTHS, N_CHUNKS - len(first)))]


def chunks(name):
    """The case's chunks, a list of uint8 arrays (built once; do not modify)."""
    if ("c", name) in _cache:
        return _cache["c", name]
    case = BY_NAME[name]
    c, _, total = table(name)
    rng = np.random.default_rng(seed_of("c:" + name))
    nz = np.nonzero(c)[0]
    if case.kind == "rare":
        out = []
        for L in RARE_LENGTHS:
            ch = rng.integers(1, 256, L)
            ch[rng.random(L) < 0.05] = 0
            out.append(ch.astype(np.uint8))
    elif case.kind == "split":
        near = split_seam_table(total)[2]
        out = []
        for L in _lengths(rng):
            ch = rng.choice(nz, L)
            pick = rng.random(L) < 0.5
            ch[pick] = rng.choice(near, int(pick.sum()))
            out.append(ch.astype(np.uint8))
    else:
        p = c[nz].astype(np.float64) / float(total)
        out = [rng.choice(nz, L, p=p).astype(np.uint8) for L in _lengths(rng)]
    _cache["c", name] = out
    return out


def seam_chunks(pair):
    """Chunks for both tables of a seam pair: symbols of their common support, drawn evenly."""
    a, b = pair
    if ("s", a) not in _cache:
        both = np.nonzero((table(a)[0] > 0) & (table(b)[0][:len(table(a)[0])] > 0))[0]
        rng = np.random.default_rng(seed_of("s:" + a))
        _cache["s", a] = [rng.choice(both, L).astype(np.uint8) for L in _lengths(rng)]
    return _cache["s", a]


def garbage(name):
    """-> (codes, counts): N_GARBAGE streams of 8 .. 400 random bytes and 0 .. 300 symbols to
    decode from each (built once)."""
    if ("g", name) not in _cache:
        rng = np.random.default_rng(seed_of("g:" + name))
        codes = [rng.integers(0, 256, int(rng.integers(8, 400))).astype(np.uint8).tobytes()
                 for _ in range(N_GARBAGE)]
        _cache["g", name] = (codes, [int(rng.integers(0, 300)) for _ in codes])
    return _cache["g", name]


def cuts(name):
    """How many bytes (0 .. 5) to cut from the end of each sound stream of the case."""
    rng = np.random.default_rng(seed_of("u:" + name))
    return [int(x) for x in rng.integers(0, 6, len(chunks(name)))]
