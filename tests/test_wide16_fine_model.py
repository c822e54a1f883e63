"""wide16 fine models without a device: what the constructor accepts and rejects (the check the
constructor shares, rc_model_wide16_fine_check_), the plan, rc_quantize_counts_wide16_fine, the
Python errors, and the wide16 entry points' limits, which stay as they were."""
import ctypes

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N
from wide_ref import table

T24 = 1 << 24
SHAPES = [(1, 65537), (256, 1 << 20), (65536, 65537), (65536, T24), (65535, T24 - 3)]


def _check(c, cum, total, n=None):
    c = np.ascontiguousarray(c, np.uint32)
    cum = np.ascontiguousarray(cum, np.uint32)
    return N.load().rc_model_wide16_fine_check_(len(c) if n is None else n,
                                                ctypes.c_void_p(c.ctypes.data),
                                                ctypes.c_void_p(cum.ctypes.data), total)


def _flat(n, total):
    """n frequencies summing to total, as even as they come."""
    f = np.full(n, total // n, np.int64)
    f[: total - int(f.sum())] += 1
    return table(f)


def test_names_and_caps():
    assert N.MAX_WIDE16_FINE_TOTAL == T24 and N.MAX_WIDE16_SYMBOLS == 65536
    for name in ("rc_model_create_static_wide16_fine", "rc_quantize_counts_wide16_fine"):
        assert name in N.EXPORTS
    assert issubclass(rc.Wide16FineModel, rc.Wide16StaticModel)


@pytest.mark.parametrize("n,total", SHAPES)
def test_accepted(n, total):
    c, cum, t = _flat(n, total)
    assert t == total and _check(c, cum, total) == N.RC_OK
    m = rc.Wide16FineModel(c, cum, total)
    assert (m.n_symbols, m.total) == (n, total)
    assert np.array_equal(m.c, c) and np.array_equal(m.cum, cum)
    # the wide16 constructor still refuses every one of them
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(c, cum, total)


def test_zero_frequencies_are_allowed():
    f = np.zeros(65536, np.int64)
    f[3000], f[63000] = 1, T24 - 1
    c, cum, total = table(f)
    assert _check(c, cum, total) == N.RC_OK
    assert rc.Wide16FineModel(c, cum, total).max_bits_per_symbol() == 24.125


def test_rejected():
    c, cum, total = _flat(300, 1 << 20)
    assert _check(c, cum, total) == N.RC_OK
    assert _check(c, cum, total, n=0) == N.RC_E_BAD_MODEL
    z = np.zeros(65537, np.uint32)
    z[0] = 1 << 20
    zc = np.full(65537, 1 << 20, np.uint32)
    zc[0] = 0
    assert _check(z, zc, 1 << 20) == N.RC_E_BAD_MODEL  # n = 65537
    assert _check(z[:65536], zc[:65536], 1 << 20) == N.RC_OK
    for tot in (256, 65535, 65536, T24 + 1, (1 << 25)):  # 65536 is the wide16 constructor's
        c2, cum2, t2 = _flat(200, tot)
        assert t2 == tot and _check(c2, cum2, tot) == N.RC_E_BAD_MODEL
    bad = cum.copy()
    bad[100] += 1
    assert _check(c, bad, total) == N.RC_E_BAD_MODEL  # a broken cum
    bad = cum.copy()
    bad[0] = 1
    assert _check(c, bad, total) == N.RC_E_BAD_MODEL  # cum[0] != 0
    assert _check(c, cum, total - 1) == N.RC_E_BAD_MODEL  # a wrong sum
    assert _check(c, cum, total + 1) == N.RC_E_BAD_MODEL
    assert N.load().rc_model_wide16_fine_check_(300, None, None, total) == N.RC_E_ARG


@pytest.mark.parametrize("n,total", SHAPES + [(5000, 100003), (300, 1 << 17)])
def test_plan(n, total):
    out = (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_wide16_fine_plan_(n, total, out) == N.RC_OK
    enc_lanes, enc_lds, layout, enc_tab, dec_lanes, dec_lds, bits, shift = (int(v) for v in out)
    # the encoder's LDS holds the rings alone (148 B per lane): a CU's 1,024 lanes at every n
    assert (enc_lanes, enc_lds) == (1024, 1024 * 148) and enc_lds <= 160 * 1024
    assert layout == 0 and enc_tab == 8 * (n + (1 if n < 65536 else 0)) <= 512 * 1024
    # the decoder's holds 2^bits bucket halfwords, the sentinel (padded to 16 B) and 72 B of rings
    # per lane: 1,024 lanes beside 2^15 buckets, 384 beside 2^16
    assert bits in (15, 16) and dec_lanes == (1024 if bits == 15 else 384)
    assert dec_lds == (2 << bits) + 16 + dec_lanes * 72 <= 160 * 1024
    # the buckets cover the total: the last q's bucket is in the table's upper half
    assert shift == (total - 1).bit_length() - bits >= 1
    assert (1 << bits) > (total - 1) >> shift >= (1 << bits) // 2
    c, cum, t = _flat(n, total)
    p = rc.Wide16FineModel(c, cum, t).plan()
    assert p["enc_table_bytes"] == enc_tab and p["dec_lanes"] == dec_lanes
    assert p["dec_bucket_bytes"] == (2 << bits) + 4 and p["dec_shift"] == shift
    n_occ = int(np.count_nonzero(c))
    assert p["dec_rcum_bytes"] == 4 * (n_occ + 2) and p["dec_occ_bytes"] in (2 * n_occ, 2 * n_occ + 2)


def test_plan_rejects_what_the_constructor_rejects():
    out = (ctypes.c_uint32 * 8)()
    L = N.load()
    for n, total in ((0, 1 << 20), (65537, 1 << 20), (100, 65536), (100, 256), (100, T24 + 1)):
        assert L.rc_model_wide16_fine_plan_(n, total, out) == N.RC_E_BAD_MODEL
    assert L.rc_model_wide16_fine_plan_(100, 1 << 20, None) == N.RC_E_ARG


@pytest.mark.parametrize("target", [65537, T24])
def test_quantize_counts_wide16_fine_dense(target):
    rng = np.random.default_rng(target)
    counts = rng.integers(1, 1 << 30, 65536).astype(np.uint64)  # all 65536 symbols occur
    counts[rng.integers(0, 65536, 30000)] = 1
    c, cum, total = rc.quantize_counts_wide16_fine(counts, target)
    assert total == target and len(c) == 65536
    assert (c >= 1).all() and int(c.sum(dtype=np.uint64)) == target
    assert np.array_equal(cum, np.concatenate([[0], np.cumsum(c, dtype=np.uint64)[:-1]]))
    rc.Wide16FineModel(c, cum, total)
    m = rc.Wide16FineModel.from_counts(counts, target)
    assert m.total == target and (m.c >= 1).all()


def test_quantize_counts_wide16_fine_is_the_one_rule():
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 50, 4096).astype(np.uint64)
    # the rule is quantize_counts': where another entry point takes the same target, same table
    L = N.load()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    a = rc.quantize_counts_wide16_fine(counts[:256], 1 << 20)
    b = rc.quantize_counts(counts[:256], 1 << 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 1 << 20
    # absent symbols stay at 0 without all_symbols, and get 1 with it
    c, _, _ = rc.quantize_counts_wide16_fine(counts, 1 << 18)
    assert ((c > 0) == (counts > 0)).all()
    c, _, total = rc.quantize_counts_wide16_fine(counts, 1 << 18, all_symbols=True)
    assert (c >= 1).all() and total == 1 << 18
    # the target must be a fine model's: 0 (the exact table), 65536 and 2^24 + 1 are refused
    cc, cu, tot = np.zeros(4096, np.uint32), np.zeros(4096, np.uint32), ctypes.c_uint32()
    for target in (0, 4096, 65536, T24 + 1):
        assert L.rc_quantize_counts_wide16_fine(p(counts), 4096, target, 0, p(cc), p(cu),
                                                ctypes.byref(tot)) == N.RC_E_ARG
        with pytest.raises(ValueError):
            rc.quantize_counts_wide16_fine(counts, target)
    assert L.rc_quantize_counts_wide16_fine(p(counts), 65537, 1 << 20, 0, p(cc), p(cu),
                                            ctypes.byref(tot)) == N.RC_E_ARG


def test_python_constructor_errors():
    with pytest.raises(ValueError, match="65537..16777216"):
        rc.Wide16FineModel(np.ones(65536, np.uint32))  # total 65536: the wide16 model's table
    with pytest.raises(ValueError):
        rc.Wide16FineModel(np.full(65537, 2, np.uint32))
    with pytest.raises(ValueError):
        rc.Wide16FineModel(np.zeros(0, np.uint32))
    with pytest.raises(ValueError):
        rc.Wide16FineModel(np.full(65536, 257, np.uint32))  # total above 2^24
    with pytest.raises(ValueError):
        rc.Wide16FineModel(np.full((16, 16), 1000, np.uint32))
    c, cum, total = _flat(5000, 1 << 20)
    with pytest.raises(ValueError):
        rc.Wide16FineModel(c, cum[:-1], total)
    with pytest.raises(ValueError):
        rc.Wide16FineModel(c, cum, total - 1)
    with pytest.raises(ValueError):
        rc.Wide16FineModel.from_counts(np.ones(300, np.uint64), 65536)
    m = rc.Wide16FineModel(np.full(65536, 2, np.uint32))  # cum and total from c
    assert m.total == 1 << 17 and m.cum[-1] == (1 << 17) - 2
    assert m.max_bits_per_symbol() == 16.125


def test_the_wide16_entry_points_keep_their_limits():
    out = (ctypes.c_uint32 * 8)()
    L = N.load()
    c, cum, total = _flat(200, 65537)
    cc, cu = np.ascontiguousarray(c, np.uint32), np.ascontiguousarray(cum, np.uint32)
    assert L.rc_model_wide16_check_(200, ctypes.c_void_p(cc.ctypes.data),
                                    ctypes.c_void_p(cu.ctypes.data), 65537) == N.RC_E_BAD_MODEL
    assert L.rc_model_wide16_plan_(200, 65537, out) == N.RC_E_BAD_MODEL
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(np.full(65536, 2, np.uint32))
    with pytest.raises(ValueError):  # rc_quantize_counts_wide16 at n = 65536 caps at its total
        rc.Wide16StaticModel(*rc.quantize_counts_wide16(np.ones(65536, np.uint64), 1 << 17))
