"""Order-1 sets without a device: what Order1ModelSet / rc_model_create_order1_set accept
(rc_model_order1_check_), the LDS plan with the context map (rc_model_order1_plan_) for every
set size, the set's own plan unchanged, the argument checks of the entry points and the
build-time guarantee that the two new coders use no scratch memory."""
import ctypes
import os
import sys

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840
KEYS = ("enc_lanes", "enc_lds", "enc_layout", "enc_tab", "dec_lanes", "dec_lds", "dec_bits",
        "dec_shift")


def _rows(K, n, total):
    """K valid rows of n symbols summing to total (every c >= 1)."""
    rng = np.random.default_rng(K * 1000 + n)
    c = np.ones((K, n), np.uint32)
    for j in range(K):
        c[j] += rng.multinomial(total - n, np.ones(n) / n).astype(np.uint32)
    return c


def _plan(fn, K, total):
    out = (ctypes.c_uint32 * 8)()
    assert getattr(N.load(), fn)(K, total, out) == N.RC_OK
    return dict(zip(KEYS, out))


# ---------------------------------------------------------------- validation
def test_accepts_the_largest_set():
    c = _rows(64, 256, 65536)
    m = rc.Order1ModelSet(c, None, 65536, ctx_map=np.arange(256) % 64, first_row=63)
    assert (m.n_models, m.n_symbols, m.total, m.first_row) == (64, 256, 65536, 63)
    assert m.ctx_map.dtype == np.uint8 and len(m.ctx_map) == 256
    assert 0 < m.max_bits_per_symbol() <= 16
    m.close()  # (no device snapshot was made)
    small = rc.Order1ModelSet(_rows(3, 100, 40000), ctx_map=np.arange(100) % 3)
    assert small.total == 40000 and small.first_row == 0


def test_rejects_bad_maps_and_first_rows():
    K, n = 4, 64
    c = _rows(K, n, 4096)
    good = np.arange(n) % K
    rc.Order1ModelSet(c, None, 4096, ctx_map=good, first_row=K - 1)
    bad = good.copy()
    bad[n - 1] = K  # a map entry equal to K
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=bad)
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=good, first_row=K)
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=good[:n - 1])  # shorter than n_symbols
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096)  # no map at all
    # and the library's own check, which the constructors go through
    lib = N.load()
    cum = np.zeros_like(c)
    cum[:, 1:] = np.cumsum(c, axis=1)[:, :-1]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    g8, b8 = good.astype(np.uint8), bad.astype(np.uint8)
    assert lib.rc_model_order1_check_(K, n, p(c), p(cum), 4096, p(g8), K - 1) == N.RC_OK
    assert lib.rc_model_order1_check_(K, n, p(c), p(cum), 4096, p(b8), 0) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_check_(K, n, p(c), p(cum), 4096, p(g8), K) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_check_(K, n, p(c), p(cum), 4096, None, 0) == N.RC_E_ARG


def test_rejects_what_the_set_rejects():
    with pytest.raises(ValueError):  # K = 0
        rc.Order1ModelSet(np.zeros((0, 16), np.uint32), None, 256, ctx_map=np.zeros(16))
    with pytest.raises(ValueError):  # K = 65
        rc.Order1ModelSet(_rows(65, 16, 256), None, 256, ctx_map=np.zeros(16))
    for total in (255, 65537):
        with pytest.raises(ValueError):
            rc.Order1ModelSet(_rows(2, 64, total), None, total, ctx_map=np.zeros(64))
    c = _rows(4, 64, 4096)
    c[3, 63] -= 1  # a row whose sum is not the total
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=np.zeros(64))


def test_from_counts_keeps_every_symbol_encodable():
    counts = np.zeros((2, 10), np.uint64)
    counts[0, 3] = 1000
    counts[1, :5] = 7
    m = rc.Order1ModelSet.from_counts(counts, np.arange(10) % 2, 1, 4096)
    assert m.total == 4096 and (m.c > 0).all() and m.c.sum(axis=1).tolist() == [4096, 4096]
    assert m.first_row == 1 and m.ctx_map.tolist() == [0, 1] * 5
    assert m.derive_indexes([3, 4, 4, 9]).tolist() == [1, 1, 0, 0]


# ---------------------------------------------------------------- the LDS plan
@pytest.mark.parametrize("total", [256, 257, 40000, 65535, 65536])
def test_plan_with_the_map_fits_the_cu_for_every_set_size(total):
    bl = (total - 1).bit_length()
    for K in range(1, 65):
        p = _plan("rc_model_order1_plan_", K, total)
        s = _plan("rc_model_set_plan_", K, total)
        # encoder: the set's plan; the map takes the place of row K, which holds >= 1 KiB
        assert [p[k] for k in KEYS[:4]] == [s[k] for k in KEYS[:4]]
        row = 2048 if p["enc_layout"] == 0 else 4 * 257
        assert K * row + 1024 <= p["enc_tab"] and p["enc_lds"] <= LDS_PER_CU
        # decoder: cum rows, the 1-KiB map, the buckets and 72 B per lane
        assert p["dec_lanes"] % 64 == 0 and 512 <= p["dec_lanes"] <= 1024
        assert 1 <= p["dec_bits"] <= min(12, bl) and p["dec_shift"] == bl - p["dec_bits"]
        assert (1 << p["dec_bits"]) << p["dec_shift"] >= total
        assert p["dec_lds"] == (K * (4 * 257 + (4 << p["dec_bits"])) + 1024 +
                                72 * p["dec_lanes"])
        assert p["dec_lds"] <= LDS_PER_CU, (K, p)
        # both halves of a decoder map word fit 16 bits: the bucket base and the row address,
        # in 4-B words
        assert (K << p["dec_bits"]) < 65536 and p["dec_lds"] // 4 < 65536


def test_the_sets_own_plan_did_not_move():
    """rc_model_set_plan_ at total 65536: the rows of DESIGN.md section 9.5's table."""
    want = {1: (1024, 155648, 0, 4096, 1024, 91140, 12, 4),
            8: (1024, 161792, 1, 10240, 1024, 147488, 11, 5),
            16: (768, 148480, 0, 34816, 1024, 155712, 10, 6),
            32: (768, 148480, 1, 34816, 1024, 139392, 8, 8),
            64: (512, 143360, 1, 67584, 768, 153856, 7, 9)}
    for K, w in want.items():
        assert tuple(_plan("rc_model_set_plan_", K, 65536).values()) == w, K


def test_plan_rejects_what_the_check_rejects():
    out = (ctypes.c_uint32 * 8)()
    lib = N.load()
    assert lib.rc_model_order1_plan_(0, 65536, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_(65, 65536, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_(8, 255, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_(8, 65537, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_(8, 65536, None) == N.RC_E_ARG


# ---------------------------------------------------------------- the entry points
def test_null_arguments_rejected():
    lib = N.load()
    h = ctypes.c_void_p()
    assert lib.rc_model_create_order1_set(None, 1, 1, None, None, 256, None, 0,
                                          ctypes.byref(h)) == N.RC_E_ARG
    assert lib.rc_encode_batch_order1(None, None, None, None, 0, None, None, None,
                                      None) == N.RC_E_ARG
    assert lib.rc_decode_batch_order1(None, None, None, None, None, None, None, 0,
                                      None) == N.RC_E_ARG
    assert lib.rc_histogram_order1(None, 1, None, 0, None, None, 0, None) == N.RC_E_ARG


def test_new_coders_use_no_scratch_and_128_vgprs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    res = isa_check.check_library(N.LIB_PATH)
    # (the period-1 instantiations: the map policy is part of the mangled name)
    names = [k for k in res
             if ("k_encode_order1" in k or "k_decode_order1" in k) and "O1Map1" in k]
    assert len(names) == 6  # encoder: 2 divisions x 2 layouts; decoder: 2 divisions
    for k in names:
        assert res[k][0] == 128 and not res[k][2], (k, res[k])
        assert isa_check.SCRATCH.get(k, 0) == 0, k
