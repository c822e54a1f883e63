"""The case table of the single-table static coders (tests/static_cases.py) is sound and reaches
what it claims, shown without a device: the class of every case as rc_model_create_static itself
computes it (the host-only hook rc_model_static_plan_), the union of the classes, divisions and
encoder variants, a round trip of every chunk through the oracle, the split-seam and runs
buckets as the wide bucket decoder gets them (rc_bucket_table_), the cost of the rare-heavy
streams and the share of garbage streams the oracle flags.  tests/test_gpu_static_classes.py
runs the same cases on the device."""
import ctypes

import numpy as np
import pytest

import static_cases as S
from oracle import cpu
from range_coder_rust_amd import _native as N

PLAN_WORDS = ("sm", "direct", "flat", "has_pair", "has_symof", "lut_bits", "lut_shift", "div",
              "enc_variant")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _plan(c, cum, total):
    out = (ctypes.c_uint32 * len(PLAN_WORDS))()
    rc = N.load().rc_model_static_plan_(len(c), _ptr(c), _ptr(cum), total, out)
    return rc, dict(zip(PLAN_WORDS, out))


def _buckets(c, cum, total, cap=4096):
    out = np.zeros(max(cap, 1), np.uint32)
    size = ctypes.c_uint32(0)
    rc = N.load().rc_bucket_table_(len(c), _ptr(c), _ptr(cum), total, _ptr(out), cap,
                                   ctypes.byref(size))
    return rc, out[:size.value]


@pytest.fixture(scope="module")
def encoded():
    """name -> [(flags, bytes, length)] of every chunk of every case, from the oracle."""
    return {case.name: [cpu.encode(*S.table(case.name), ch) for ch in S.chunks(case.name)]
            for case in S.CASES}


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_case_lands_in_its_class(name):
    case = S.BY_NAME[name]
    c, cum, total = S.table(name)
    rc, p = _plan(c, cum, total)
    assert rc == N.RC_OK
    got = (p["sm"], p["direct"], p["flat"], p["has_pair"], p["has_symof"])
    assert got == S.CLASSES[case.cls], (name, p)
    assert p["div"] == S.div_of(total) and p["enc_variant"] == case.smv, (name, p)
    if case.cls == "wide_bucket":
        assert (p["lut_bits"], p["lut_shift"]) == (S.WIDE_LUT_BITS, case.shift), (name, p)


def test_cases_cover_every_class_division_and_encoder():
    # every (sm, direct, flat) that rc_model_create_static can produce, under both divisions
    # (the pair buckets, dense in test_gpu_parity.py, are here for the 2^16 seam alone)
    seen = {(S.CLASSES[c.cls][:3], S.div_of(S.table(c.name)[2])) for c in S.CASES}
    assert {c.cls for c in S.CASES} == set(S.CLASSES)
    for sdf in ((0, 1, 0), (1, 2, 0), (1, 2, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0)):
        assert (sdf, S.DIV_POW2) in seen, sdf
        if sdf != (1, 2, 1):  # (the flat model: total 256)
            assert (sdf, S.DIV_MAGIC) in seen, sdf
    assert {S.table(c.name)[2] for c in S.CASES if c.cls == "wide_direct"} >= {1, 2, 128, 255}
    assert {c.smv for c in S.CASES} == {S.SMV_WIDE, S.SMV_INCOMPLETE, S.SMV_COMPLETE, S.SMV_FLAT}
    # both encoder variants of the small-model range under both divisions
    for smv in (S.SMV_INCOMPLETE, S.SMV_COMPLETE):
        assert {S.div_of(S.table(c.name)[2]) for c in S.CASES if c.smv == smv} == {0, 1}, smv
    totals = {S.table(c.name)[2] for c in S.CASES}
    assert {1, 2, 255, 256, 257, 512, 513, 2047, 2048, 2049, 65536, 65537, 1 << 17,
            (1 << 32) - 1} <= totals
    assert {c.shift for c in S.CASES if c.cls == "wide_bucket"} >= {5, 6, 8, 13, 17, 19, 20}


def test_cases_keep_to_their_shapes():
    for case in S.CASES:
        lens = [len(ch) for ch in S.chunks(case.name)]
        assert len(lens) <= 64 and set(lens) <= set(S.LENGTHS + S.RARE_LENGTHS), case.name
        if case.kind != "rare":
            assert set(lens) == set(S.LENGTHS), case.name
    for pair in S.SEAM_PAIRS:
        ta, tb = S.table(pair[0])[2], S.table(pair[1])[2]
        assert tb == ta + 1
        assert S.BY_NAME[pair[0]].cls != S.BY_NAME[pair[1]].cls
        for name in pair:
            c = S.table(name)[0]
            assert all((c[ch] > 0).all() for ch in S.seam_chunks(pair)), name


def test_the_hooks_check_their_arguments():
    c, cum, total = S.table("t1048576_zipf")
    out = (ctypes.c_uint32 * 9)()
    lib = N.load()
    assert lib.rc_model_static_plan_(len(c), _ptr(c), _ptr(cum), total, None) == N.RC_E_ARG
    assert lib.rc_model_static_plan_(len(c), None, _ptr(cum), total, out) == N.RC_E_ARG
    assert lib.rc_model_static_plan_(len(c), _ptr(c), _ptr(cum), total - 1, out) == \
        N.RC_E_BAD_MODEL
    assert lib.rc_model_static_plan_(0, _ptr(c), _ptr(cum), total, out) == N.RC_E_BAD_MODEL
    assert _buckets(c, cum, total, cap=4095)[0] == N.RC_E_ARG
    assert _buckets(c, cum, total - 1)[0] == N.RC_E_BAD_MODEL
    for name in ("t255_seam", "t2048_zipf", "t65536_seam"):  # classes with other tables
        assert _buckets(*S.table(name), cap=1 << 16)[0] == N.RC_E_BAD_MODEL, name


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_case_round_trips_through_the_oracle(name, encoded):
    c, cum, total = S.table(name)
    for ch, (f, b, L) in zip(S.chunks(name), encoded[name]):
        assert f == 0 and L == len(b)
        fd, d = cpu.decode(c, cum, total, b, len(ch))
        assert fd == 0 and (d == ch).all()
    if name in [p[0] for p in S.SEAM_PAIRS]:
        pair = [p for p in S.SEAM_PAIRS if p[0] == name][0]
        for other in pair:
            co, cumo, to = S.table(other)
            for ch in S.seam_chunks(pair):
                f, b, _ = cpu.encode(co, cumo, to, ch)
                assert f == 0 and (cpu.decode(co, cumo, to, b, len(ch))[1] == ch).all()


def _starts_in_bucket(c, cum, b, shift, total):
    lo, hi = b << shift, min((b + 1) << shift, total)
    return [int(cum[s]) - lo for s in range(len(c)) if c[s] and lo < cum[s] < hi]


@pytest.mark.parametrize("name", S.SPLIT_CASES)
def test_split_seam_tables_hold_the_three_entries(name):
    """0xFFFE and 0xFFFF are stored as the second candidate's offset (the latter reads like
    "none", but with s1 != s0 the decoder's compare against it is still right); 0x10000 does
    not fit the field and is stored as "none", s1 = s0: the exact fix-up finds the symbol."""
    c, cum, total = S.table(name)
    shift = S.BY_NAME[name].shift
    rc, lut = _buckets(c, cum, total)
    assert rc == N.RC_OK and len(lut) == 1 << S.WIDE_LUT_BITS
    want = {}
    for b, off in zip(S.SPLIT_BUCKETS, S.SPLIT_OFFSETS):
        e = int(lut[b])
        s0, s1, split = e & 255, (e >> 8) & 255, e >> 16
        starts = _starts_in_bucket(c, cum, b, shift, total)
        assert starts[0] == off and len(starts) >= 3, (b, starts)
        assert cum[s0] <= (b << shift) < cum[s0] + c[s0]
        if off <= 0xFFFF:
            assert split == off and s1 != s0 and c[s1] > 0 and cum[s1] == (b << shift) + off
        else:
            assert split == 0xFFFF and s1 == s0
        want[off, s1 - s0] = True
    assert set(want) == {(0xFFFE, 1), (0xFFFF, 1), (0x10000, 0), (0xFFFE, 2)}
    # (the last: a zero-frequency symbol stands between s0 and the start)
    b = S.SPLIT_BUCKETS[3]
    s0 = int(lut[b]) & 255
    assert c[s0 + 1] == 0 and cum[s0 + 1] == (b << shift) + 0xFFFE
    # and the chunks visit both sides of every start
    near = set(S.split_seam_table(total)[2])
    seen = set(np.concatenate(S.chunks(name)).tolist())
    assert near <= seen and len(near) == 12


@pytest.mark.parametrize("name", S.RUNS_WIDE_CASES)
def test_runs_tables_hold_buckets_with_three_starts(name):
    c, cum, total = S.table(name)
    shift = S.BY_NAME[name].shift
    rc, lut = _buckets(c, cum, total)
    assert rc == N.RC_OK and len(lut) == 1 << S.WIDE_LUT_BITS
    b = np.minimum(cum[c > 0].astype(np.int64) >> shift, len(lut) - 1)
    assert np.bincount(b).max() >= 3
    # the entries: s0 holds the bucket's first frequency, s1 is the next start with c > 0
    for k in np.flatnonzero(np.bincount(b, minlength=len(lut)) >= 3)[:8]:
        e = int(lut[k])
        s0, s1, split = e & 255, (e >> 8) & 255, e >> 16
        assert cum[s0] <= (int(k) << shift) < int(cum[s0]) + int(c[s0])
        st = _starts_in_bucket(c, cum, int(k), shift, total)
        if st and st[0] <= 0xFFFF:
            assert split == st[0] and cum[s1] == (int(k) << shift) + st[0] and c[s1] > 0


@pytest.mark.parametrize("name", S.RARE_CASES)
def test_rare_heavy_streams_cost_what_they_should(name, encoded):
    """At least 0.95 x log2(total) / 8 bytes per symbol, all bytes of all chunks counted: every
    symbol but the 5 % of symbol 0 costs log2(total) bits.  (Read here: 2.8547 at 2^24 + 1,
    3.6929 at 2^31, 3.8035 at 2^32 - 1; chunks of c = 1 symbols alone cost the oracle 3.9998
    at 2^32 - 1.)"""
    total = S.table(name)[2]
    n_bytes = sum(L for _, _, L in encoded[name])
    n_syms = sum(len(ch) for ch in S.chunks(name))
    cost = n_bytes / n_syms
    print(name, "bytes per symbol:", round(cost, 4))
    assert cost >= 0.95 * np.log2(total) / 8


@pytest.mark.parametrize("name", S.GARBAGE_CASES)
def test_garbage_streams_split_both_ways(name):
    """Of the 64 garbage streams of a marked table the oracle alone flags at least 8 and decodes
    at least 8 cleanly, so the device test compares flags and symbols, not one of the two."""
    c, cum, total = S.table(name)
    codes, counts = S.garbage(name)
    assert len(codes) == S.N_GARBAGE
    assert all(8 <= len(g) < 400 for g in codes) and all(0 <= k < 300 for k in counts)
    flags = [cpu.decode(c, cum, total, g, k)[0] for g, k in zip(codes, counts)]
    print(name, "flagged:", sum(1 for f in flags if f), "clean:", sum(1 for f in flags if not f))
    assert sum(1 for f in flags if f) >= 8 and sum(1 for f in flags if not f) >= 8


def test_garbage_cases_are_the_tables_with_zeros():
    totals = {S.table(n)[2] for n in S.GARBAGE_CASES}
    assert totals >= {255, 513, 2047, 2048, 65537, 1 << 17, 1 << 20, 1 << 31, (1 << 32) - 1}
    for n in S.GARBAGE_CASES:
        c = S.table(n)[0]
        assert len(c) == 200 and c[-1] == 0 and 0.15 < (c == 0).mean() < 0.45, n
