"""Static model sets without a device: what rc_model_create_static_set accepts
(rc_model_set_check_), the LDS plan of the indexed kernels for every set size
(rc_model_set_plan_), the argument checks of the three entry points, the host side of
StaticModelSet, and the build-time guarantee that the new coders use no scratch memory."""
import ctypes
import os
import sys

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840


def _rows(K, n, total, rng=None):
    """K valid rows of n symbols summing to total (every c >= 1)."""
    rng = rng or np.random.default_rng(K * 1000 + n)
    c = np.ones((K, n), np.uint32)
    for j in range(K):
        extra = rng.multinomial(total - n, np.ones(n) / n)
        c[j] += extra.astype(np.uint32)
    cum = np.zeros_like(c)
    cum[:, 1:] = np.cumsum(c, axis=1)[:, :-1]
    return c, cum


def _check(K, n, c, cum, total):
    return N.load().rc_model_set_check_(K, n, ctypes.c_void_p(c.ctypes.data),
                                        ctypes.c_void_p(cum.ctypes.data), total)


def test_check_accepts_one_and_sixty_four_rows():
    for K in (1, 64):
        c, cum = _rows(K, 256, 65536)
        assert _check(K, 256, c, cum, 65536) == N.RC_OK
    c, cum = _rows(3, 100, 40000)  # not a power of two, a smaller alphabet
    assert _check(3, 100, c, cum, 40000) == N.RC_OK
    assert N.MAX_SET_MODELS == 64


def test_check_accepts_zero_frequency_symbols():
    c, cum = _rows(2, 16, 256)
    c[1, 3] += c[1, 4]
    c[1, 4] = 0
    cum[1, 1:] = np.cumsum(c[1])[:-1]
    assert _check(2, 16, c, cum, 256) == N.RC_OK


def test_check_rejects_bad_sets():
    c, cum = _rows(65, 256, 65536)
    assert _check(0, 256, c, cum, 65536) == N.RC_E_BAD_MODEL
    assert _check(65, 256, c, cum, 65536) == N.RC_E_BAD_MODEL
    assert _check(2, 0, c, cum, 65536) == N.RC_E_BAD_MODEL
    assert _check(2, 257, c, cum, 65536) == N.RC_E_BAD_MODEL
    for total in (255, 65537):
        c, cum = _rows(2, 64, total)
        assert _check(2, 64, c, cum, total) == N.RC_E_BAD_MODEL
    c, cum = _rows(4, 64, 4096)
    bad = cum.copy()
    bad[2, 10] += 1  # a row whose cum does not scan
    assert _check(4, 64, c, bad, 4096) == N.RC_E_BAD_MODEL
    short = c.copy()
    short[3, 63] -= 1  # a row whose sum differs from the shared total
    assert _check(4, 64, short, cum, 4096) == N.RC_E_BAD_MODEL
    assert _check(4, 64, c, cum, 4096) == N.RC_OK
    assert N.load().rc_model_set_check_(1, 64, None, None, 4096) == N.RC_E_ARG


def _plan(K, total):
    out = (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_set_plan_(K, total, out) == N.RC_OK
    keys = ("enc_lanes", "enc_lds", "enc_layout", "enc_tab", "dec_lanes", "dec_lds", "dec_bits",
            "dec_shift")
    return dict(zip(keys, out))


@pytest.mark.parametrize("total", [256, 40000, 65536])
def test_plan_fits_the_cu_for_every_set_size(total):
    bl = (total - 1).bit_length()
    for K in range(1, 65):
        p = _plan(K, total)
        for side in ("enc", "dec"):
            lanes = p[side + "_lanes"]
            assert p[side + "_lds"] <= LDS_PER_CU, (K, side, p)
            assert lanes % 64 == 0 and 256 <= lanes <= 1024, (K, side, p)
        # the encoder's tables and 148 B of rings per lane; the rings are 1-KiB aligned
        rows = (K + 1) * (2048 if p["enc_layout"] == 0 else 4 * 257)
        assert p["enc_layout"] in (0, 1) and p["enc_tab"] >= rows and p["enc_tab"] % 1024 == 0
        assert p["enc_lds"] == p["enc_tab"] + 148 * p["enc_lanes"]
        # the decoder's cum rows, its buckets (covering every frequency) and 72 B per lane
        assert 1 <= p["dec_bits"] <= min(12, bl)
        assert p["dec_shift"] == bl - p["dec_bits"]
        assert (1 << p["dec_bits"]) << p["dec_shift"] >= total
        assert p["dec_lds"] == K * (4 * 257 + (4 << p["dec_bits"])) + 72 * p["dec_lanes"]


def test_plan_spends_spare_lds_on_finer_buckets():
    bits = [_plan(K, 65536)["dec_bits"] for K in (1, 8, 16, 32, 64)]
    assert bits == sorted(bits, reverse=True) and bits[0] == 12
    lanes = [_plan(K, 65536)["enc_lanes"] for K in (1, 8, 16, 32, 64)]
    assert lanes == sorted(lanes, reverse=True) and lanes[0] == 1024


def test_plan_rejects_what_the_check_rejects():
    out = (ctypes.c_uint32 * 8)()
    lib = N.load()
    assert lib.rc_model_set_plan_(0, 65536, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_set_plan_(65, 65536, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_set_plan_(8, 255, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_set_plan_(8, 65537, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_set_plan_(8, 65536, None) == N.RC_E_ARG


def test_null_arguments_rejected():
    lib = N.load()
    h = ctypes.c_void_p()
    c, cum = _rows(2, 64, 4096)
    pc, pcum = ctypes.c_void_p(c.ctypes.data), ctypes.c_void_p(cum.ctypes.data)
    assert lib.rc_model_create_static_set(None, 2, 64, pc, pcum, 4096, ctypes.byref(h)) == N.RC_E_ARG
    assert lib.rc_model_create_static_set(None, 2, 64, None, None, 4096, None) == N.RC_E_ARG
    assert h.value is None
    assert lib.rc_encode_batch_indexed(None, None, None, None, None, 0, None, None, None,
                                       None) == N.RC_E_ARG
    assert lib.rc_decode_batch_indexed(None, None, None, None, None, None, None, None, 0,
                                       None) == N.RC_E_ARG


def test_from_counts_rows_sum_to_the_target():
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 1000, (5, 256)).astype(np.uint64)
    counts[2, 10:200] = 0  # absent symbols stay encodable
    counts[4] = 0          # an empty sample still gives a row
    for target in (65536, 4096):
        s = rc.StaticModelSet.from_counts(counts, target)
        assert (s.n_models, s.n_symbols, s.total) == (5, 256, target)
        assert (s.c.astype(np.uint64).sum(axis=1) == target).all() and (s.c >= 1).all()
        assert (s.cum[:, 0] == 0).all()
        assert (s.cum[:, 1:] == np.cumsum(s.c, axis=1)[:, :-1]).all()


def test_static_model_set_validates_on_the_host():
    c, cum = _rows(3, 32, 1024)
    s = rc.StaticModelSet(c)  # cum and total derived
    assert s.total == 1024 and (s.cum == cum).all()
    bad = c.copy()
    bad[1, 0] += 1
    with pytest.raises(ValueError):
        rc.StaticModelSet(bad, total_freq=1024)
    with pytest.raises(ValueError):
        rc.StaticModelSet(np.ones((65, 256), np.uint32))
    with pytest.raises(ValueError):
        rc.StaticModelSet(np.ones((2, 16), np.uint32))  # total 16 < 256

    class Two(rc.FreqTable):
        pass

    a, b = Two(4), Two(4)
    for i, k in ((0, 100), (1, 100), (2, 50), (3, 6)):
        for _ in range(k):
            a.add_alphabet_freq(i)
            b.add_alphabet_freq(3 - i)
    a.calc_cum()
    b.calc_cum()
    s = rc.StaticModelSet.from_pmodels([a, b])
    assert s.c.tolist() == [[100, 100, 50, 6], [6, 50, 100, 100]] and s.total == 256
    b.add_alphabet_freq(0)
    b.calc_cum()
    with pytest.raises(ValueError):
        rc.StaticModelSet.from_pmodels([a, b])


def test_indexed_coders_use_no_scratch():
    """The indexed coders keep their state, tiles and index blocks in registers, like the
    single-table ones (tests/test_isa_check.py): build() refuses a library in which one uses
    scratch memory."""
    lib = os.path.join(ROOT, "range_coder_rust_amd", "librc_amd.so")
    assert os.path.exists(lib), "library not built"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    sizes = isa_check.scratch_sizes(lib)
    coders = {k: v for k, v in sizes.items() if "k_encode_indexed" in k or "k_decode_indexed" in k}
    assert len(coders) >= 6, coders  # 2 divisions x 2 table layouts, 2 decoders
    assert not {k: v for k, v in coders.items() if v}, coders
    import __graft_entry__ as ge
    import inspect
    src = inspect.getsource(ge._check_isa)
    assert "k_encode_indexed" in src and "k_decode_indexed" in src
