"""Periodic order-1 sets without a device: the reference's self-checks (periodic_ref against
order1_ref), what rc_model_create_order1_set_periodic accepts (rc_model_order1_check_periodic_),
the LDS plan per (K, total, period), the new kernels' registers, and the refusals that need no
device (the ones that need a set on the device are in test_gpu_periodic.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N, container

import order1_ref
import periodic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840
KEYS = ("enc_lanes", "enc_lds", "enc_layout", "enc_tab", "dec_lanes", "dec_lds", "dec_bits",
        "dec_shift")
PERIODS = (1, 2, 4, 8)


def _rows(K, n, total, seed=0):
    """K valid rows of n symbols summing to total (every c >= 1)."""
    rng = np.random.default_rng(K * 1000 + n + seed)
    c = np.ones((K, n), np.uint32)
    for j in range(K):
        c[j] += rng.multinomial(total - n, np.ones(n) / n).astype(np.uint32)
    return c


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------- the reference against itself
def test_period_1_reference_is_order1_ref():
    rng = np.random.default_rng(1)
    K, n, total = 5, 100, 40000
    c, cum = periodic_ref.tables(order1_ref.markov_rows(rng, K, n, total))
    cm = rng.integers(0, K, n).astype(np.uint8)
    for L in (0, 1, 2, 17, 300):
        s = order1_ref.draw_markov(rng, c, cm, 3, L)
        assert np.array_equal(periodic_ref.derive_idx(cm[None], 3, s, n),
                              order1_ref.derive_idx(cm, 3, s, n))
        want = order1_ref.encode_ref(c, cum, total, cm, 3, s)
        assert periodic_ref.encode_ref(c, cum, total, cm[None], 3, s) == want
        f, d = periodic_ref.decode_ref(c, cum, total, cm[None], 3, want[1], L)
        f1, d1 = order1_ref.decode_ref(c, cum, total, cm, 3, want[1], L)
        assert f == f1 == 0 and np.array_equal(d, d1) and np.array_equal(d, s)


@pytest.mark.parametrize("P", [2, 4, 8])
def test_identical_slices_are_the_unphased_reference(P):
    rng = np.random.default_rng(P)
    K, n, total = 6, 256, 65536
    c, cum = periodic_ref.tables(order1_ref.markov_rows(rng, K, n, total))
    cm = rng.integers(0, K, n).astype(np.uint8)
    cmp_ = np.tile(cm, (P, 1))
    for L in (0, 1, P, P + 1, 33, 200):
        s = order1_ref.draw_markov(rng, c, cm, 1, L)
        want = order1_ref.encode_ref(c, cum, total, cm, 1, s)
        assert periodic_ref.encode_ref(c, cum, total, cmp_, 1, s) == want
        f, d = periodic_ref.decode_ref(c, cum, total, cmp_, 1, want[1], L)
        assert f == 0 and np.array_equal(d, s)
    # and a garbage stream: the same flag and the same symbols before it
    code = rng.integers(0, 256, 120).astype(np.uint8).tobytes()
    f, d = periodic_ref.decode_ref(c, cum, total, cmp_, 1, code, 150)
    f1, d1 = order1_ref.decode_ref(c, cum, total, cm, 1, code, 150)
    assert f == f1 and np.array_equal(d, d1)


def test_the_phase_reaches_the_reference():
    """Two rows with disjoint supports and a purely positional map of period 2: the reference
    codes a chunk that alternates the supports and refuses one that does not."""
    n, total = 16, 4096
    rows = np.zeros((2, n), np.int64)
    rows[0, :8] = total // 8
    rows[1, 8:] = total // 8
    c, cum = periodic_ref.tables(rows)
    cm = np.stack([np.zeros(n, np.uint8), np.ones(n, np.uint8)])  # even i: row 0, odd i: row 1
    good = np.array([1, 9, 2, 10, 3, 11], np.uint8)
    f, b = periodic_ref.encode_ref(c, cum, total, cm, 0, good)
    assert f == 0
    f2, d = periodic_ref.decode_ref(c, cum, total, cm, 0, b, len(good))
    assert f2 == 0 and np.array_equal(d, good)
    assert periodic_ref.encode_ref(c, cum, total, cm, 0, good[::-1].copy())[0] == N.F_ZERO_FREQ
    assert periodic_ref.ideal_bits(c, total, cm, 0, good) == pytest.approx(3.0 * len(good))
    assert periodic_ref.ideal_bits(c, total, cm, 0, good[::-1]) == float("inf")


# ---------------------------------------------------------------- creation
def test_accepts_the_largest_set():
    c = _rows(64, 256, 65536)
    cm = (np.arange(8 * 256).reshape(8, 256) * 7 + np.arange(8)[:, None]) % 64
    m = rc.Order1ModelSet(c, None, 65536, ctx_map=cm, first_row=63, period=8)
    assert (m.n_models, m.n_symbols, m.total, m.first_row, m.period) == (64, 256, 65536, 63, 8)
    assert m.ctx_map.dtype == np.uint8 and m.ctx_map.shape == (8, 256)
    s = np.arange(40, dtype=np.uint8)
    assert np.array_equal(m.derive_indexes(s), periodic_ref.derive_idx(cm, 63, s, 256))
    m.close()  # (no device snapshot was made)
    # a flat map is still a period-1 set, and so is a [1, n] one
    flat = rc.Order1ModelSet(c, None, 65536, ctx_map=np.arange(256) % 64)
    one = rc.Order1ModelSet(c, None, 65536, ctx_map=(np.arange(256) % 64)[None], period=1)
    assert flat.period == one.period == 1 and np.array_equal(flat.ctx_map, one.ctx_map)


def test_rejects_every_other_period():
    K, n = 4, 64
    c = _rows(K, n, 4096)
    cum = periodic_ref.tables(c)[1]
    lib = N.load()
    out = (ctypes.c_uint32 * 8)()
    h = ctypes.c_void_p()
    for P in range(18):
        cm = (np.arange(max(P, 1) * n) % K).astype(np.uint8)
        rc_ = lib.rc_model_order1_check_periodic_(K, n, _p(c), _p(cum), 4096, P, _p(cm), 0)
        assert rc_ == (N.RC_OK if P in PERIODS else N.RC_E_ARG), P
        assert lib.rc_model_order1_plan_periodic_(K, 4096, P, out) == \
            (N.RC_OK if P in PERIODS else N.RC_E_ARG), P
        if P not in PERIODS:
            with pytest.raises(ValueError):
                rc.Order1ModelSet(c, None, 4096, ctx_map=cm.reshape(max(P, 1), n), period=P)
    # a [P, n] map under another period, and a flat map under a period > 1
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=np.zeros((4, n)), period=2)
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=np.zeros(4 * n), period=4)
    assert h.value is None


@pytest.mark.parametrize("P", [2, 4, 8])
def test_rejects_a_bad_entry_in_each_slice_and_a_bad_first_row(P):
    K, n = 4, 64
    c = _rows(K, n, 4096)
    cum = periodic_ref.tables(c)[1]
    lib = N.load()
    good = (np.arange(P * n).reshape(P, n) % K).astype(np.uint8)
    assert lib.rc_model_order1_check_periodic_(K, n, _p(c), _p(cum), 4096, P, _p(good),
                                               K - 1) == N.RC_OK
    rc.Order1ModelSet(c, None, 4096, ctx_map=good, first_row=K - 1, period=P)
    for ph in range(P):
        for s in (0, n - 1):
            bad = good.copy()
            bad[ph, s] = K
            assert lib.rc_model_order1_check_periodic_(K, n, _p(c), _p(cum), 4096, P, _p(bad),
                                                       0) == N.RC_E_BAD_MODEL, (ph, s)
            with pytest.raises(ValueError):
                rc.Order1ModelSet(c, None, 4096, ctx_map=bad, period=P)
    assert lib.rc_model_order1_check_periodic_(K, n, _p(c), _p(cum), 4096, P, _p(good),
                                               K) == N.RC_E_BAD_MODEL
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=good, first_row=K, period=P)
    # the set's own rules still hold: a row whose sum is not the total
    c2 = c.copy()
    c2[K - 1, n - 1] -= 1
    assert lib.rc_model_order1_check_periodic_(K, n, _p(c2), _p(cum), 4096, P, _p(good),
                                               0) == N.RC_E_BAD_MODEL


def test_null_arguments_rejected():
    lib = N.load()
    h = ctypes.c_void_p()
    c = _rows(1, 16, 256)
    cum = periodic_ref.tables(c)[1]
    cm = np.zeros(32, np.uint8)
    assert lib.rc_model_create_order1_set_periodic(None, 1, 16, _p(c), _p(cum), 256, 2, _p(cm),
                                                   0, ctypes.byref(h)) == N.RC_E_ARG
    assert lib.rc_model_create_order1_set_periodic(None, 1, 16, None, None, 256, 2, None, 0,
                                                   None) == N.RC_E_ARG
    assert lib.rc_model_order1_check_periodic_(1, 16, _p(c), _p(cum), 256, 2, None,
                                               0) == N.RC_E_ARG
    assert lib.rc_model_order1_check_periodic_(1, 16, None, None, 256, 2, _p(cm),
                                               0) == N.RC_E_ARG
    assert lib.rc_model_order1_plan_periodic_(8, 65536, 2, None) == N.RC_E_ARG
    assert lib.rc_histogram_pairs_periodic(None, 2, None, None, 0, None, None) == N.RC_E_ARG
    assert h.value is None


# ---------------------------------------------------------------- the LDS plan
def _plan(K, total, P):
    out = (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_order1_plan_periodic_(K, total, P, out) == N.RC_OK
    return dict(zip(KEYS, out))


@pytest.mark.parametrize("total", [256, 4096, 40000, 65536])
def test_plan_fits_the_cu_for_every_set_size_and_period(total):
    bl = (total - 1).bit_length()
    lib = N.load()
    for K in range(1, 65):
        old = (ctypes.c_uint32 * 8)()
        assert lib.rc_model_order1_plan_(K, total, old) == N.RC_OK
        assert list(_plan(K, total, 1).values()) == list(old), K
        for P in (2, 4, 8):
            p = _plan(K, total, P)
            # encoder: K rows in the layout chosen, P KiB of maps behind them, 148 B per lane
            row = 2048 if p["enc_layout"] == 0 else 4 * 257
            assert p["enc_layout"] in (0, 1) and p["enc_tab"] % 1024 == 0
            assert K * row + P * 1024 <= p["enc_tab"] < K * row + P * 1024 + 1024
            assert p["enc_lanes"] % 64 == 0 and 256 <= p["enc_lanes"] <= 1024
            assert p["enc_lds"] == p["enc_tab"] + 148 * p["enc_lanes"] <= LDS_PER_CU, (K, P, p)
            # decoder: cum rows, P KiB of maps, the buckets and 72 B per lane
            assert p["dec_lanes"] % 64 == 0 and 256 <= p["dec_lanes"] <= 1024
            assert 1 <= p["dec_bits"] <= min(12, bl) and p["dec_shift"] == bl - p["dec_bits"]
            assert p["dec_lds"] == (K * (4 * 257 + (4 << p["dec_bits"])) + P * 1024 +
                                    72 * p["dec_lanes"])
            assert p["dec_lds"] <= LDS_PER_CU, (K, P, p)
            # both halves of a decoder map word fit 16 bits
            assert (K << p["dec_bits"]) < 65536 and p["dec_lds"] // 4 < 65536
            # a longer period never gets more lanes or finer buckets than a shorter one
            q = _plan(K, total, P // 2)
            assert p["enc_lanes"] <= q["enc_lanes"] and p["dec_bits"] <= q["dec_bits"]


def test_plan_table_of_the_design():
    """DESIGN.md section 9.12's table at total 65536: the encoder's plan at K = 8 has 2 KiB to
    spare at period 1, so it loses lanes from P = 4 on; K = 64 keeps the 512-lane encoder and
    the 768-lane decoder."""
    assert _plan(8, 65536, 1)["enc_lds"] == 161792
    assert [_plan(8, 65536, P)["enc_lanes"] for P in PERIODS] == [1024, 1024, 768, 768]
    assert [_plan(8, 65536, P)["enc_layout"] for P in PERIODS] == [1, 1, 0, 0]
    for P in (2, 4, 8):
        p = _plan(64, 65536, P)
        assert (p["enc_lanes"], p["enc_layout"], p["dec_lanes"]) == (512, 1, 768), (P, p)


def test_plan_rejects_what_the_check_rejects():
    out = (ctypes.c_uint32 * 8)()
    lib = N.load()
    assert lib.rc_model_order1_plan_periodic_(0, 65536, 4, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_periodic_(65, 65536, 4, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_periodic_(8, 255, 4, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_periodic_(8, 65537, 4, out) == N.RC_E_BAD_MODEL


# ---------------------------------------------------------------- the kernels
def test_periodic_kernels_use_no_scratch_and_128_vgprs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    res = isa_check.check_library(N.LIB_PATH)
    # (the periodic instantiations: the map policy is part of the mangled name)
    names = [k for k in res
             if ("k_encode_order1" in k or "k_decode_order1" in k) and "O1MapP" in k]
    assert len(names) == 6  # encoder: 2 divisions x 2 layouts; decoder: 2 divisions
    for k in names:
        assert res[k][0] == 128 and not res[k][2], (k, res[k])
        assert isa_check.SCRATCH.get(k, 0) == 0, k
    # (<true>, mangled ILb1EE: the instantiations with the period)
    assert any("k_histogram_pairsILb1EE" in k for k in res)
    assert any("k_ideal_bits_order1ILb1EE" in k for k in res)


# ---------------------------------------------------------------- refusals without a device
def test_containers_refuse_a_period():
    """pack() and compress() raise before they touch a device: RCB2 has no field for a period."""
    c = _rows(4, 64, 4096)
    cm = np.zeros((2, 64), np.uint8)
    m = rc.Order1ModelSet(c, None, 4096, ctx_map=cm, period=2)
    with pytest.raises(ValueError, match="period"):
        container.pack(m, None, None, None, None)
    with pytest.raises(ValueError, match="period"):
        container.compress(None, model=m)
    with pytest.raises(ValueError, match="period"):
        rc.compress(None, model=m, order=1, checksum=True)


def test_fit_refuses_a_phase_without_a_row():
    """fit_order1_set gives every phase n_models // period classes: fewer rows than phases is a
    ValueError, as is a period the kernels do not take, before any device work."""
    with pytest.raises(ValueError):
        rc.fit_order1_set(None, None, n_models=3, period=4)
    with pytest.raises(ValueError):
        rc.fit_order1_set(None, None, n_models=8, period=3)
