"""Lagged order-1 sets without a device: the reference's self-checks (lag_ref against
periodic_ref), what rc_model_create_order1_set_lagged accepts (rc_model_order1_check_lagged_),
the LDS plan (the periodic plan whatever the lag), the new kernels' registers, the refusals that
need no device (the ones that need a set on the device are in test_gpu_lag.py) and the fitted
cost that the lag buys on records."""
import ctypes
import os
import sys

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N, container

import joint_fit_ref
import lag_ref
import order1_ref
import periodic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_VALUES = (1, 2, 4, 8)  # periods and lags


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
@pytest.mark.parametrize("P", [1, 4])
def test_lag_1_reference_is_periodic_ref(P):
    rng = np.random.default_rng(10 + P)
    K, n, total = 5, 100, 40000
    c, cum = lag_ref.tables(order1_ref.markov_rows(rng, K, n, total))
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    chunks = []
    for L in (0, 1, 2, 17, 300):
        s = periodic_ref.draw_markov(rng, c, cm, 3, L)
        chunks.append(s)
        assert np.array_equal(lag_ref.derive_idx(cm, 3, s, n, 1),
                              periodic_ref.derive_idx(cm, 3, s, n))
        want = periodic_ref.encode_ref(c, cum, total, cm, 3, s)
        assert lag_ref.encode_ref(c, cum, total, cm, 3, s, 1) == want
        f, d = lag_ref.decode_ref(c, cum, total, cm, 3, want[1], L, 1)
        assert f == 0 and np.array_equal(d, s)
        assert lag_ref.ideal_bits(c, total, cm, 3, s, 1) == \
            periodic_ref.ideal_bits(c, total, cm, 3, s)
    for a, b in zip(lag_ref.pairs(chunks, P, 1), periodic_ref.pairs(chunks, P)):
        assert np.array_equal(a, b)
    # a garbage stream: the same flag and the same symbols before it
    code = rng.integers(0, 256, 120).astype(np.uint8).tobytes()
    f, d = lag_ref.decode_ref(c, cum, total, cm, 3, code, 150, 1)
    f1, d1 = periodic_ref.decode_ref(c, cum, total, cm, 3, code, 150)
    assert f == f1 and np.array_equal(d, d1)


@pytest.mark.parametrize("D", [2, 4, 8])
def test_the_lag_reaches_the_reference(D):
    """Two rows with disjoint supports, map: low symbols -> row 1, high symbols -> row 0, so a
    chunk must alternate the supports at distance D; the first D symbols take first_row 0.  The
    reference round-trips such a chunk and refuses one that alternates at distance 1."""
    n, total = 16, 4096
    rows = np.zeros((2, n), np.int64)
    rows[0, :8] = total // 8
    rows[1, 8:] = total // 8
    c, cum = lag_ref.tables(rows)
    cm = (np.arange(n) < 8).astype(np.uint8)[None]
    good = np.array([(i % 8) + 8 * ((i // D) & 1) for i in range(6 * D + 3)], np.uint8)
    assert np.array_equal(lag_ref.derive_idx(cm, 0, good, n, D), (np.arange(len(good)) // D) & 1)
    f, b = lag_ref.encode_ref(c, cum, total, cm, 0, good, D)
    assert f == 0
    f2, d = lag_ref.decode_ref(c, cum, total, cm, 0, b, len(good), D)
    assert f2 == 0 and np.array_equal(d, good)
    assert lag_ref.ideal_bits(c, total, cm, 0, good, D) == pytest.approx(3.0 * len(good))
    bad = np.array([(i % 8) + 8 * (i & 1) for i in range(6 * D + 3)], np.uint8)
    assert lag_ref.encode_ref(c, cum, total, cm, 0, bad, D)[0] == N.F_ZERO_FREQ
    assert lag_ref.ideal_bits(c, total, cm, 0, bad, D) == float("inf")
    pair, first = lag_ref.pairs([good, good[:D - 1], good[:0]], 1, D)
    assert int(first.sum()) == D + D - 1 and int(pair.sum()) == len(good) - D
    assert int(pair[0, :8, :8].sum()) == 0 and int(pair[0, 8:, 8:].sum()) == 0


# ---------------------------------------------------------------- creation
def test_python_set_carries_the_lag():
    c = _rows(64, 256, 65536)
    cm = (np.arange(8 * 256).reshape(8, 256) * 7 + np.arange(8)[:, None]) % 64
    m = rc.Order1ModelSet(c, None, 65536, ctx_map=cm, first_row=63, period=8, lag=4)
    assert (m.n_models, m.n_symbols, m.period, m.lag, m.first_row) == (64, 256, 8, 4, 63)
    s = (np.arange(40) * 37 % 256).astype(np.uint8)
    assert np.array_equal(m.derive_indexes(s), lag_ref.derive_idx(cm, 63, s, 256, 4))
    assert np.array_equal(m.derive_indexes(s[:3]), [63, 63, 63])
    m.close()  # (no device snapshot was made)
    # period 1 with a lag takes a flat map; lag 1 is the default
    flat = rc.Order1ModelSet(c, None, 65536, ctx_map=np.arange(256) % 64, lag=2)
    assert (flat.period, flat.lag) == (1, 2)
    assert np.array_equal(flat.derive_indexes(s),
                          lag_ref.derive_idx((np.arange(256) % 64)[None], 0, s, 256, 2))
    assert rc.Order1ModelSet(c, None, 65536, ctx_map=np.arange(256) % 64).lag == 1


def test_rejects_every_other_lag_and_period():
    K, n = 4, 64
    c = _rows(K, n, 4096)
    cum = lag_ref.tables(c)[1]
    lib = N.load()
    out = (ctypes.c_uint32 * 8)()
    cm8 = (np.arange(8 * n) % K).astype(np.uint8)
    for D in range(18):
        for P in (1, 2, 3, 4, 8):
            ok = D in OK_VALUES and P in OK_VALUES
            got = lib.rc_model_order1_check_lagged_(K, n, _p(c), _p(cum), 4096, P, D, _p(cm8), 0)
            assert got == (N.RC_OK if ok else N.RC_E_ARG), (P, D)
            assert lib.rc_model_order1_plan_lagged_(K, 4096, P, D, out) == \
                (N.RC_OK if ok else N.RC_E_ARG), (P, D)
        if D not in OK_VALUES:
            with pytest.raises(ValueError, match="lag"):
                rc.Order1ModelSet(c, None, 4096, ctx_map=cm8.reshape(8, n), period=8, lag=D)
            with pytest.raises(ValueError, match="lag"):
                rc.fit_order1_set(None, None, n_models=8, period=4, lag=D)


@pytest.mark.parametrize("D", [2, 4, 8])
@pytest.mark.parametrize("P", [1, 2, 8])
def test_rejects_a_bad_entry_in_each_slice_and_a_bad_first_row(P, D):
    K, n = 4, 64
    c = _rows(K, n, 4096)
    cum = lag_ref.tables(c)[1]
    lib = N.load()

    def check(cm, first_row, tab=c):
        return lib.rc_model_order1_check_lagged_(K, n, _p(tab), _p(cum), 4096, P, D, _p(cm),
                                                 first_row)

    good = (np.arange(P * n).reshape(P, n) % K).astype(np.uint8)
    assert check(good, K - 1) == N.RC_OK
    rc.Order1ModelSet(c, None, 4096, ctx_map=good, first_row=K - 1, period=P, lag=D)
    for ph in range(P):
        for s in (0, n - 1):
            bad = good.copy()
            bad[ph, s] = K
            assert check(bad, 0) == N.RC_E_BAD_MODEL, (ph, s)
            with pytest.raises(ValueError):
                rc.Order1ModelSet(c, None, 4096, ctx_map=bad, period=P, lag=D)
    assert check(good, K) == N.RC_E_BAD_MODEL
    with pytest.raises(ValueError):
        rc.Order1ModelSet(c, None, 4096, ctx_map=good, first_row=K, period=P, lag=D)
    # the set's own rules still hold: a row whose sum is not the total
    c2 = c.copy()
    c2[K - 1, n - 1] -= 1
    assert check(good, 0, c2) == N.RC_E_BAD_MODEL


def test_null_arguments_rejected():
    lib = N.load()
    h = ctypes.c_void_p()
    c = _rows(1, 16, 256)
    cum = lag_ref.tables(c)[1]
    cm = np.zeros(32, np.uint8)
    assert lib.rc_model_create_order1_set_lagged(None, 1, 16, _p(c), _p(cum), 256, 2, 2, _p(cm),
                                                 0, ctypes.byref(h)) == N.RC_E_ARG
    assert lib.rc_model_create_order1_set_lagged(None, 1, 16, None, None, 256, 2, 2, None, 0,
                                                 None) == N.RC_E_ARG
    assert lib.rc_model_order1_check_lagged_(1, 16, _p(c), _p(cum), 256, 2, 2, None,
                                             0) == N.RC_E_ARG
    assert lib.rc_model_order1_check_lagged_(1, 16, None, None, 256, 2, 2, _p(cm),
                                             0) == N.RC_E_ARG
    assert lib.rc_model_order1_plan_lagged_(8, 65536, 2, 2, None) == N.RC_E_ARG
    assert lib.rc_histogram_pairs_lagged(None, 2, 2, None, None, 0, None, None) == N.RC_E_ARG
    assert h.value is None


# ---------------------------------------------------------------- the LDS plan
@pytest.mark.parametrize("total", [256, 40000, 65536])
def test_plan_is_the_periodic_plan_for_every_lag(total):
    lib = N.load()
    for K in range(1, 65):
        for P in OK_VALUES:
            per = (ctypes.c_uint32 * 8)()
            assert lib.rc_model_order1_plan_periodic_(K, total, P, per) == N.RC_OK
            for D in OK_VALUES:
                out = (ctypes.c_uint32 * 8)()
                assert lib.rc_model_order1_plan_lagged_(K, total, P, D, out) == N.RC_OK
                assert list(out) == list(per), (K, P, D)
    out = (ctypes.c_uint32 * 8)()
    assert lib.rc_model_order1_plan_lagged_(0, total, 4, 4, out) == N.RC_E_BAD_MODEL
    assert lib.rc_model_order1_plan_lagged_(65, total, 4, 4, out) == N.RC_E_BAD_MODEL


# ---------------------------------------------------------------- the kernels
def test_lagged_kernels_use_no_scratch_and_128_vgprs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    res = isa_check.check_library(N.LIB_PATH)
    # (the lagged instantiations: the map policy, and so the lag, is part of the mangled name)
    for D in (2, 4, 8):
        tag = f"O1MapLagILi{D}EE"
        enc = [k for k in res if "k_encode_order1" in k and tag in k]
        dec = [k for k in res if "k_decode_order1" in k and tag in k]
        assert (len(enc), len(dec)) == (4, 2), D  # 2 divisions x 2 layouts; 2 divisions
        for k in enc + dec:
            assert res[k][0] == 128 and not res[k][2], (k, res[k])
            assert isa_check.SCRATCH.get(k, 0) == 0, k
        for name in (f"k_histogram_pairs_lagILi{D}EE", f"k_ideal_bits_order1_lagILi{D}EE"):
            ks = [k for k in res if name in k]
            assert len(ks) == 1, name
            assert res[ks[0]][0] <= 128 and not res[ks[0]][2], (ks[0], res[ks[0]])
            assert isa_check.SCRATCH.get(ks[0], 0) == 0, ks[0]


# ---------------------------------------------------------------- refusals without a device
def test_containers_refuse_a_lag():
    """pack() and compress() raise before they touch a device: RCB2 has no field for a lag."""
    c = _rows(4, 64, 4096)
    for P in (1, 2):
        m = rc.Order1ModelSet(c, None, 4096, ctx_map=np.zeros((P, 64), np.uint8), period=P, lag=2)
        with pytest.raises(ValueError, match="lag|period"):
            container.pack(m, None, None, None, None)
        with pytest.raises(ValueError, match="lag|period"):
            container.compress(None, model=m)
        with pytest.raises(ValueError, match="lag|period"):
            rc.compress(None, model=m, order=1, checksum=True)
    m = rc.Order1ModelSet(c, None, 4096, ctx_map=np.zeros(64, np.uint8), lag=8)
    with pytest.raises(ValueError, match="lag"):
        container.pack(m, None, None, None, None)


def test_fit_refuses_a_phase_without_a_row():
    with pytest.raises(ValueError):
        rc.fit_order1_set(None, None, n_models=3, period=4, lag=4)


# ---------------------------------------------------------------- the fitted cost
def walk_bytes():
    """2^16 int32 of a random walk with steps in [-50, 50], as 2^18 little-endian bytes."""
    rng = np.random.default_rng(1)
    return np.cumsum(rng.integers(-50, 51, 2 ** 16)).astype("<i4").view(np.uint8)


def bf16_bytes():
    """2^17 bf16 (the top 16 bits of float32) of a noisy sine, as 2^18 little-endian bytes."""
    rng = np.random.default_rng(1)
    t = np.arange(2 ** 17)
    x = (np.sin(t / 300) + 0.05 * rng.standard_normal(2 ** 17)).astype("<f4")
    return (x.view("<u4") >> 16).astype("<u2").view(np.uint8)


def fitted_cost(data, P, D, chunk=16384, K=8):
    """Bits per symbol of the joint clustering reference's K rows on pair counts taken at
    distance D, the first D symbols of each chunk being the start-of-chunk item."""
    chunks = [data[o:o + chunk] for o in range(0, len(data), chunk)]
    pair, first = lag_ref.pairs(chunks, P, D)
    assert int(pair.sum() + first.sum()) == len(data)
    cost = joint_fit_ref.cluster_joint_ref(pair, first, max_models=K, want_lead=False)[3]
    return cost / len(data)


@pytest.mark.parametrize("source,P", [(walk_bytes, 4), (bf16_bytes, 2)])
def test_the_records_own_lag_fits_cheaper_than_lag_1(source, P):
    """At the same K = 8 and the same period the context P bytes back (the same byte of the record
    before) gives a cheaper fit than the byte before (another field of the same number).  Measured:
    a ratio of 0.82 on the walk and 0.83 on the bf16 source; the assertion is the order alone."""
    data = source()
    assert len(data) == 1 << 18
    near, far = fitted_cost(data, P, 1), fitted_cost(data, P, P)
    print(f"{source.__name__}: lag 1 {near:.3f}, lag {P} {far:.3f} bits/symbol, "
          f"ratio {far / near:.3f}")
    assert far < near
