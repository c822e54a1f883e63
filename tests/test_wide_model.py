"""Wide static models without a device: what rc_model_create_static_wide accepts
(rc_model_wide_check_), the LDS plan of the wide kernels for every alphabet size
(rc_model_wide_plan_), rc_quantize_counts_wide, the argument checks of the entry points, the host
side of WideStaticModel, and the build-time guarantee that the new coders use no scratch memory."""
import ctypes
import os
import sys

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840


def _table(n, total, rng=None, zeros=0):
    """A valid table of n symbols summing to total; `zeros` of them have c == 0."""
    rng = rng or np.random.default_rng(n * 7 + total)
    live = n - zeros
    c = np.zeros(n, np.uint32)
    pos = np.sort(rng.choice(n, live, replace=False))
    c[pos] = 1 + rng.multinomial(total - live, np.ones(live) / live).astype(np.uint32)
    cum = np.zeros_like(c)
    cum[1:] = np.cumsum(c)[:-1]
    return c, cum


def _check(n, c, cum, total):
    return N.load().rc_model_wide_check_(n, ctypes.c_void_p(c.ctypes.data),
                                         ctypes.c_void_p(cum.ctypes.data), total)


def test_check_accepts_what_the_header_says():
    for n, total in ((1, 256), (2, 65536), (257, 40000), (1000, 65535), (4096, 65536),
                     (4096, 4096)):
        c, cum = _table(n, total)
        assert _check(n, c, cum, total) == N.RC_OK, (n, total)
    # zero-frequency symbols: more symbols than frequencies
    c, cum = _table(4096, 256, zeros=4096 - 200)
    assert _check(4096, c, cum, 256) == N.RC_OK
    assert N.MAX_WIDE_SYMBOLS == 4096


def test_check_rejects_bad_tables():
    c, cum = _table(4096, 65536)
    big = np.concatenate([c, [0]]).astype(np.uint32)
    bigcum = np.concatenate([cum, [65536]]).astype(np.uint32)
    assert _check(0, c, cum, 65536) == N.RC_E_BAD_MODEL
    assert _check(4097, big, bigcum, 65536) == N.RC_E_BAD_MODEL
    for total in (255, 65537):
        c, cum = _table(100, total)
        assert _check(100, c, cum, total) == N.RC_E_BAD_MODEL
    c, cum = _table(1000, 4096)
    bad = cum.copy()
    bad[10] += 1  # cum does not scan
    assert _check(1000, c, bad, 4096) == N.RC_E_BAD_MODEL
    short = c.copy()
    short[999] -= 1  # the sum differs from the total
    assert _check(1000, short, cum, 4096) == N.RC_E_BAD_MODEL
    assert _check(1000, c, cum, 4096) == N.RC_OK
    assert N.load().rc_model_wide_check_(64, None, None, 4096) == N.RC_E_ARG


def _plan(n, total, out=None):
    out = out or (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_wide_plan_(n, total, out) == N.RC_OK
    return tuple(out)


@pytest.mark.parametrize("total", [256, 4096, 65535, 65536])
def test_plan_fits_the_cu_for_every_alphabet_size(total):
    bl = (total - 1).bit_length()
    out = (ctypes.c_uint32 * 8)()
    for n in range(1, 4097):
        enc_lanes, enc_lds, layout, enc_tab, dec_lanes, dec_lds, bits, shift = _plan(n, total, out)
        # it fits 163,840 B in both directions, with at least 768 lanes, a multiple of 64
        assert enc_lds <= LDS_PER_CU and dec_lds <= LDS_PER_CU, (n, tuple(out))
        for lanes in (enc_lanes, dec_lanes):
            assert lanes % 64 == 0 and 768 <= lanes <= 1024, (n, tuple(out))
        # the encoder's table (entry n, or cum[n] and cum[n + 1], included) and 148 B of rings
        # per lane; the rings are 1-KiB aligned
        tab = (n + 1) * 8 if layout == 0 else (n + 2) * 4
        assert layout in (0, 1) and enc_tab >= tab and enc_tab % 1024 == 0
        assert enc_lds == enc_tab + 148 * enc_lanes
        # the decoder's row cum[0 .. n], its buckets (covering every frequency), 72 B per lane
        assert 1 <= bits <= min(12, bl) and shift == bl - bits
        assert (1 << bits) << shift >= total
        assert dec_lds == 4 * (n + 1) + (4 << bits) + 72 * dec_lanes


def test_plan_at_the_largest_alphabet():
    enc_lanes, enc_lds, layout, enc_tab, dec_lanes, dec_lds, bits, _ = _plan(4096, 65536)
    assert (enc_lanes, layout, enc_tab) == (768, 0, 33792) and enc_lds == 33792 + 113664
    assert (dec_lanes, bits) == (1024, 12)
    assert _plan(256, 65536)[0] == 1024 and _plan(256, 65536)[2] == 0
    # between the two the cum-only row keeps 1,024 lanes where the 8-B entries no longer fit
    assert _plan(2000, 65536)[:3:2] == (1024, 1)


def test_plan_rejects_what_the_check_rejects():
    out = (ctypes.c_uint32 * 8)()
    lib = N.load()
    assert lib.rc_model_wide_plan_(0, 65536, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_wide_plan_(4097, 65536, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_wide_plan_(8, 255, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_wide_plan_(8, 65537, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_wide_plan_(8, 65536, None) == N.RC_E_ARG


def _quant(entry, counts, target, qflags):
    counts = np.ascontiguousarray(counts, np.uint64)
    n = len(counts)
    c, cum = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    total = ctypes.c_uint32()
    st = getattr(N.load(), entry)(ctypes.c_void_p(counts.ctypes.data), n, target, qflags,
                                  ctypes.c_void_p(c.ctypes.data), ctypes.c_void_p(cum.ctypes.data),
                                  ctypes.byref(total))
    return st, c, cum, total.value


def test_quantize_counts_wide_is_quantize_counts_where_they_overlap():
    rng = np.random.default_rng(9)
    for n in (1, 2, 100, 256):
        counts = rng.integers(0, 5000, n)
        counts[rng.integers(0, n, n // 4)] = 0
        for target, qf in ((0, 0), (0, 1), (65536, 0), (65536, 1), (4096, 1), (300, 1)):
            a = _quant("rc_quantize_counts", counts, target, qf)
            b = _quant("rc_quantize_counts_wide", counts, target, qf)
            assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[3] == b[3]


def test_quantize_counts_wide_takes_a_thousand_symbols():
    rng = np.random.default_rng(10)
    counts = rng.integers(0, 100, 1000)
    counts[100:400] = 0
    st, c, cum, total = _quant("rc_quantize_counts_wide", counts, 65536, N.Q_ALL_SYMBOLS)
    assert st == N.RC_OK and total == 65536 and int(c.sum()) == 65536 and (c >= 1).all()
    assert cum[0] == 0 and (cum[1:] == np.cumsum(c)[:-1]).all()
    assert _check(1000, c, cum, 65536) == N.RC_OK
    # the one-byte entry point keeps its limit, the wide one has its own
    assert _quant("rc_quantize_counts", np.ones(257), 65536, 1)[0] == N.RC_E_ARG
    assert _quant("rc_quantize_counts_wide", np.ones(257), 65536, 1)[0] == N.RC_OK
    assert _quant("rc_quantize_counts_wide", np.ones(4096), 65536, 1)[0] == N.RC_OK
    assert _quant("rc_quantize_counts_wide", np.ones(4097), 65536, 1)[0] == N.RC_E_ARG


def test_null_arguments_rejected():
    lib = N.load()
    h = ctypes.c_void_p()
    c, cum = _table(1000, 4096)
    pc, pcum = ctypes.c_void_p(c.ctypes.data), ctypes.c_void_p(cum.ctypes.data)
    assert lib.rc_model_create_static_wide(None, 1000, pc, pcum, 4096,
                                           ctypes.byref(h)) == N.RC_E_ARG
    assert lib.rc_model_create_static_wide(None, 1000, None, None, 4096, None) == N.RC_E_ARG
    assert h.value is None
    assert lib.rc_encode_batch_wide(None, None, None, None, 0, None, None, None, None) == N.RC_E_ARG
    assert lib.rc_decode_batch_wide(None, None, None, None, None, None, None, 0, None) == N.RC_E_ARG


def test_wide_static_model_validates_on_the_host():
    c, cum = _table(1000, 40000)
    m = rc.WideStaticModel(c)  # cum and total derived
    assert (m.n_symbols, m.total) == (1000, 40000) and (m.cum == cum).all()
    assert m.max_bits_per_symbol() == pytest.approx(np.log2(40000 / c[c > 0].min()))
    bad = c.copy()
    bad[1] += 1
    with pytest.raises(ValueError):
        rc.WideStaticModel(bad, total_freq=40000)
    with pytest.raises(ValueError):
        rc.WideStaticModel(np.ones(4097, np.uint32))
    with pytest.raises(ValueError):
        rc.WideStaticModel(np.ones(100, np.uint32))  # total 100 < 256
    counts = np.zeros(3000, np.uint64)
    counts[::7] = 5
    m = rc.WideStaticModel.from_counts(counts, 65536)
    assert (m.n_symbols, m.total) == (3000, 65536) and (m.c >= 1).all()
    t = rc.FreqTable(600)
    for i in range(600):
        t.add_alphabet_freq(i)
        t.add_alphabet_freq(i // 2)
    t.calc_cum()
    m = rc.WideStaticModel.from_pmodel(t)
    assert (m.n_symbols, m.total) == (600, 1200) and m.c[0] == 3 and m.c[599] == 1
    m.close()


def test_wide_coders_are_built_and_use_no_scratch():
    """Both wide kernels are in the library, keep their state and tiles in registers like the
    other coders, and are on the list build() checks for scratch memory."""
    lib = os.path.join(ROOT, "range_coder_rust_amd", "librc_amd.so")
    assert os.path.exists(lib), "library not built"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    sizes = isa_check.scratch_sizes(lib)
    enc = {k: v for k, v in sizes.items() if "k_encode_wide" in k}
    dec = {k: v for k, v in sizes.items() if "k_decode_wide" in k}
    assert len(enc) >= 4 and len(dec) >= 2, (enc, dec)  # 2 divisions x 2 layouts, 2 decoders
    assert not {k: v for k, v in {**enc, **dec}.items() if v}, (enc, dec)
    import __graft_entry__ as ge
    import inspect
    src = inspect.getsource(ge._check_isa)
    assert "k_encode_wide" in src and "k_decode_wide" in src
    assert any(s.endswith("rc_wide.hip") for s in ge.HIP_SOURCES)
