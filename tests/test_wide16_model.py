"""wide16 static models without a device: what the constructor accepts and rejects (the check the
constructor shares, rc_model_wide16_check_), the plan at the alphabet sizes around the wide
models' cap and at both ends, rc_quantize_counts_wide16, and the Python constructor's errors."""
import ctypes

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N
from wide_ref import table


def _check(c, cum, total, n=None):
    c = np.ascontiguousarray(c, np.uint32)
    cum = np.ascontiguousarray(cum, np.uint32)
    return N.load().rc_model_wide16_check_(len(c) if n is None else n,
                                           ctypes.c_void_p(c.ctypes.data),
                                           ctypes.c_void_p(cum.ctypes.data), total)


def _flat(n, total):
    """n frequencies summing to total, as even as they come (zeros when n > total)."""
    f = np.full(n, total // n, np.int64)
    f[: total - int(f.sum())] += 1
    return table(f)


def test_cap_is_the_whole_16_bit_alphabet():
    assert N.MAX_WIDE16_SYMBOLS == 65536 and N.MAX_WIDE_SYMBOLS == 4096
    for name in ("rc_model_create_static_wide16", "rc_encode_batch_wide16",
                 "rc_decode_batch_wide16", "rc_quantize_counts_wide16"):
        assert name in N.EXPORTS


@pytest.mark.parametrize("n,total", [(1, 256), (1, 65536), (4096, 65536), (4097, 65536),
                                     (20000, 65535), (65535, 40000), (65536, 65536),
                                     (65536, 256)])
def test_accepted(n, total):
    c, cum, t = _flat(n, total)
    assert t == total and _check(c, cum, total) == N.RC_OK
    m = rc.Wide16StaticModel(c, cum, total)
    assert (m.n_symbols, m.total) == (n, total)
    assert np.array_equal(m.c, c) and np.array_equal(m.cum, cum)


def test_rejected():
    c, cum, total = _flat(300, 4096)
    assert _check(c, cum, total, n=0) == N.RC_E_BAD_MODEL
    big = np.ones(65537, np.uint32)
    assert _check(big, np.arange(65537), 65537) == N.RC_E_BAD_MODEL  # n = 65537 (and the total)
    z = np.zeros(65537, np.uint32)
    z[0] = 65536
    zc = np.full(65537, 65536, np.uint32)
    zc[0] = 0
    assert _check(z, zc, 65536) == N.RC_E_BAD_MODEL  # n = 65537 alone
    assert _check(z[:65536], zc[:65536], 65536) == N.RC_OK
    for tot in (255, 65537):
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
    assert N.load().rc_model_wide16_check_(300, None, None, total) == N.RC_E_ARG


@pytest.mark.parametrize("n", [1, 4096, 4097, 65535, 65536])
@pytest.mark.parametrize("total", [256, 40000, 65535, 65536])
def test_plan(n, total):
    out = (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_wide16_plan_(n, total, out) == N.RC_OK
    enc_lanes, enc_lds, layout, enc_tab, dec_lanes, dec_lds, bits, shift = (int(v) for v in out)
    # the encoder's LDS holds the rings alone (148 B per lane): a CU's 1,024 lanes at every n
    assert (enc_lanes, enc_lds) == (1024, 1024 * 148) and enc_lds <= 160 * 1024
    # the decoder's holds the q-to-symbol halfwords and 72 B of rings per lane: 1,024 lanes up to
    # a total of 2^15, 384 beside the 128 KiB above it
    assert dec_lanes == (384 if total > 32768 else 1024)
    assert dec_lds == (2 << bits) + dec_lanes * 72 <= 160 * 1024
    # the tables in device memory: 8-B entries with a poison entry except at n = 65536, and one
    # q-to-symbol entry per q, padded to a power of two
    assert layout == 0 and enc_tab == 8 * (n + (1 if n < 65536 else 0)) <= 512 * 1024
    assert shift == 0 and (1 << bits) >= total > (1 << bits) // 2
    c, cum, t = _flat(n, total)
    p = rc.Wide16StaticModel(c, cum, t).plan()
    assert p["enc_table_bytes"] == enc_tab and p["dec_symof_bytes"] == 2 << bits <= 128 * 1024
    assert p["dec_row_bytes"] == 4 * (n + 2)


def test_plan_rejects_what_the_constructor_rejects():
    out = (ctypes.c_uint32 * 8)()
    L = N.load()
    for n, total in ((0, 4096), (65537, 65536), (100, 255), (100, 65537)):
        assert L.rc_model_wide16_plan_(n, total, out) == N.RC_E_BAD_MODEL
    assert L.rc_model_wide16_plan_(100, 4096, None) == N.RC_E_ARG


def test_quantize_counts_wide16():
    rng = np.random.default_rng(16)
    for n in (4097, 65536):
        counts = rng.integers(0, 1000, n).astype(np.uint64)
        counts[rng.integers(0, n, n // 2)] = 0
        c, cum, total = rc.quantize_counts_wide16(counts, 65536)
        assert total == 65536 and len(c) == n
        assert ((c > 0) == (counts > 0)).all()  # what occurs stays encodable, nothing else
        assert np.array_equal(cum, np.concatenate([[0], np.cumsum(c)[:-1]]))
        rc.Wide16StaticModel(c, cum, total)
        with pytest.raises(N.RCError):  # the wide rule keeps its cap
            rc.quantize_counts_wide(counts, 65536)
    # the one rule: below the wide cap the two calls agree
    counts = rng.integers(0, 50, 4096).astype(np.uint64)
    a, b = rc.quantize_counts_wide16(counts, 65536), rc.quantize_counts_wide(counts, 65536)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # every symbol kept: n = target = 65536 leaves one frequency each
    counts = rng.integers(0, 1 << 40, 65536).astype(np.uint64)
    c, cum, total = rc.quantize_counts_wide16(counts, 65536, all_symbols=True)
    assert total == 65536 and (c == 1).all()
    m = rc.Wide16StaticModel.from_counts(counts)
    assert m.total == 65536 and (m.c == 1).all()


def test_quantize_counts_wide16_errors():
    L = N.load()
    counts = np.ones(65536, np.uint64)
    c = np.zeros(65537, np.uint32)
    cum = np.zeros(65537, np.uint32)
    tot = ctypes.c_uint32()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    # RC_Q_ALL_SYMBOLS with more symbols than the target
    assert L.rc_quantize_counts_wide16(p(counts), 65536, 65535, N.Q_ALL_SYMBOLS, p(c), p(cum),
                                       ctypes.byref(tot)) == N.RC_E_ARG
    assert L.rc_quantize_counts_wide16(p(counts), 65536, 65536, N.Q_ALL_SYMBOLS, p(c), p(cum),
                                       ctypes.byref(tot)) == N.RC_OK
    # more distinct symbols than the target, without the flag: no table
    assert L.rc_quantize_counts_wide16(p(counts), 65536, 65535, 0, p(c), p(cum),
                                       ctypes.byref(tot)) == N.RC_E_BAD_MODEL
    big = np.ones(65537, np.uint64)
    assert L.rc_quantize_counts_wide16(p(big), 65537, 0, 0, p(c), p(cum),
                                       ctypes.byref(tot)) == N.RC_E_ARG
    with pytest.raises(ValueError):
        rc.quantize_counts_wide16(counts, 4096, all_symbols=True)
    with pytest.raises(ValueError):
        rc.quantize_counts_wide16(counts, 4096)


def test_python_constructor_errors():
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(np.ones(65537, np.uint32))
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(np.zeros(0, np.uint32))
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(np.ones(100, np.uint32))  # total 100 < 256
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(np.full(65536, 2, np.uint32))  # total 2^17
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(np.ones((16, 16), np.uint32))
    c, cum, total = _flat(5000, 65536)
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(c, cum[:-1], total)
    with pytest.raises(ValueError):
        rc.Wide16StaticModel(c, cum, total - 1)
    # the wide model keeps its cap and its message
    with pytest.raises(ValueError, match="1..4096"):
        rc.WideStaticModel(c, cum, total)
    m = rc.Wide16StaticModel(c)  # cum and total from c
    assert m.total == total and np.array_equal(m.cum, cum)
