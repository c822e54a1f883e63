"""rc_cluster_contexts_dev on the GPU: against the host rc_cluster_contexts at period 1, merge for
merge against the numpy reference of joint_fit_ref at periods 2, 4 and 8 (fixtures whose lead
test_joint_fit_ref.py asserts on the CPU), tie-breaks that are exact by construction, all 2,049
items live, the edges and statuses of the interface, and fit_order1_set(joint=True) end to end.

Tolerances.  Maps, first_row and n_models are compared exactly.  The cost is a sum of at most 64
row costs, each one fixed-order f64 sum of 256 non-negative terms t * log2(n / t): with log2 and
the division within an ulp or two, both the device's and numpy's sums are within about
300 * 2^-52 = 7e-14 of the exact value, so rel 1e-9 leaves four orders of magnitude."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from range_coder_rust_amd import model_build as mb  # noqa: E402
from range_coder_rust_amd.api import _ptr  # noqa: E402
from gpu_helpers import dev  # noqa: E402
import joint_fit_ref as J  # noqa: E402
import order1_fit_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def cluster_dev(ctx, pair, first, n_symbols=256, max_models=64, want_cost=True, period=None):
    """rc_cluster_contexts_dev on uploaded counts: (status, maps[P, 256], first_row, k, cost)."""
    pair = np.asarray(pair)
    P = period or (1 if pair.ndim == 2 else pair.shape[0])
    pt = dev(np.ascontiguousarray(pair, np.int64))
    ft = dev(np.ascontiguousarray(first, np.int64))
    cm = np.full((P, 256), 0xEE, np.uint8)
    fr, k, cost = ctypes.c_uint32(99), ctypes.c_uint32(99), ctypes.c_double(-1.0)
    ctx.bind_stream()
    st = ctx._lib.rc_cluster_contexts_dev(ctx.handle, P, _ptr(pt), _ptr(ft), n_symbols, max_models,
                                          ctypes.c_void_p(cm.ctypes.data), ctypes.byref(fr),
                                          ctypes.byref(k),
                                          ctypes.byref(cost) if want_cost else None)
    return st, cm, int(fr.value), int(k.value), float(cost.value)


def cluster_host(pair, first, n_symbols, max_models):
    pair = np.ascontiguousarray(pair, np.uint64)
    first = np.ascontiguousarray(first, np.uint64)
    cm = np.zeros(256, np.uint8)
    fr, k, cost = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
    st = N.load().rc_cluster_contexts(ctypes.c_void_p(pair.ctypes.data),
                                      ctypes.c_void_p(first.ctypes.data), n_symbols, max_models,
                                      ctypes.c_void_p(cm.ctypes.data), ctypes.byref(fr),
                                      ctypes.byref(k), ctypes.byref(cost))
    return st, cm, int(fr.value), int(k.value), float(cost.value)


CASES = {name: (P, n, ks, counts) for name, P, n, ks, counts in J.merge_for_merge_cases()}
P1 = [(name, K) for name, (P, n, ks, _) in CASES.items() if P == 1 for K in ks]
PN = [(name, K) for name, (P, n, ks, _) in CASES.items() if P > 1 for K in ks]


# ---- period 1 against the host call ----

@pytest.mark.parametrize("name,K", P1)
def test_period_1_gives_the_host_calls_result(ctx, name, K):
    _, n, _, (pair, first) = CASES[name]
    hst, hm, hfr, hk, hcost = cluster_host(pair, first, n, K)
    st, cm, fr, k, cost = cluster_dev(ctx, pair, first, n, K)
    assert hst == N.RC_OK and st == N.RC_OK
    print(f"{name} K={K}: k {k}/{hk}, cost rel err {abs(cost - hcost) / hcost:.3e}")
    assert np.array_equal(cm[0], hm) and fr == hfr and k == hk
    assert cost == pytest.approx(hcost, rel=1e-9)


# ---- merge for merge against the reference ----

@pytest.mark.parametrize("name,K", PN)
def test_follows_the_reference_merge_for_merge(ctx, name, K):
    P, n, _, (pair, first) = CASES[name]
    maps, rfr, rk, rcost, _ = J.cluster_joint_ref(pair, first, n, K, want_lead=False)
    st, cm, fr, k, cost = cluster_dev(ctx, pair, first, n, K)
    assert st == N.RC_OK
    print(f"{name} K={K}: k {k}/{rk}, cost rel err {abs(cost - rcost) / rcost:.3e}")
    assert k == rk and fr == rfr and np.array_equal(cm, maps)
    assert cost == pytest.approx(rcost, rel=1e-9)
    assert (cm[:, n:] == 0).all()


# ---- tie-breaks, exact by construction ----

def test_ties_all_deltas_zero(ctx):
    """Every live row holds one symbol, the same one: every cost and every delta is exactly 0.0
    (log2(n / n) = 0), so the merge order is the tie-break alone: always the two lowest slots,
    and the K - 1 highest live items keep rows of their own."""
    P = 4
    pair = np.zeros((P, 256, 256), np.int64)
    where = [(0, 5), (0, 200), (1, 0), (1, 255), (2, 17), (3, 3), (3, 254)]
    for j, (ph, p) in enumerate(where):
        pair[ph, p, 9] = 3 + 2 * j
    first = np.zeros(256, np.int64)
    first[9] = 4
    live = [ph * 256 + p for ph, p in where] + [P * 256]
    for K in (1, 3, 7):
        st, cm, fr, k, cost = cluster_dev(ctx, pair, first, 256, K)
        assert st == N.RC_OK and k == K and cost == 0.0
        rows = np.concatenate([cm.ravel(), [fr]])[live]
        # 9 - K merges of the two lowest slots: the first 9 - K live items share row 0
        want = [max(0, j - (8 - K)) for j in range(8)]
        assert list(rows) == want, (K, list(rows))
        maps, rfr, rk, rcost, _ = J.cluster_joint_ref(pair, first, 256, K, want_lead=False)
        assert np.array_equal(cm, maps) and fr == rfr and rk == K and rcost == 0.0


def test_ties_duplicate_rows_in_later_phases(ctx):
    """Six distinct rows in phase 0 and bit-identical copies of them at other contexts of phase 1.
    cost(2 v) = 2 cost(v) exactly (doubling is exact in every term and every sum), so every pair
    of copies has delta exactly 0.0 and those merge first, in index order; a cluster's deltas
    with an original and with its copy come from identical merged counts and costs, and the
    earlier index wins.  (Three copies would not do: 3 t * x is not 3 (t * x) in f64.)"""
    rng = np.random.default_rng(21)
    rows = rng.integers(1, 40, (6, 256)) * (rng.random((6, 256)) < 0.3)
    pair = np.zeros((2, 256, 256), np.int64)
    c0 = [3, 50, 77, 130, 201, 255]
    c1 = [240, 10, 99, 0, 180, 64]  # (not in the order of c0)
    for j in range(6):
        pair[0, c0[j]] = rows[j]
        pair[1, c1[j]] = rows[j]
    first = np.zeros(256, np.int64)
    st, cm, fr, k, cost = cluster_dev(ctx, pair, first, 256, 8)
    assert st == N.RC_OK and k == 8
    # 12 live items, 4 merges, all at 0.0: (3, 256 + 240), (50, 256 + 10), (77, 256 + 99),
    # (130, 256 + 0); the copies of the last two rows stay apart
    assert cm[0, 3] == cm[1, 240] == 0 and cm[0, 50] == cm[1, 10] == 1
    assert cm[0, 77] == cm[1, 99] == 2 and cm[0, 130] == cm[1, 0] == 3
    assert (cm[0, 201], cm[0, 255], cm[1, 64], cm[1, 180]) == (4, 5, 6, 7)
    for K in (8, 6, 3, 1):
        maps, rfr, rk, rcost, _ = J.cluster_joint_ref(pair, first, 256, K, want_lead=False)
        st, cm, fr, k, cost = cluster_dev(ctx, pair, first, 256, K)
        assert st == N.RC_OK and k == rk == K and fr == rfr and np.array_equal(cm, maps)
        assert cost == pytest.approx(rcost, rel=1e-9)
    # at K = 6 every copy has joined its original
    st, cm, fr, k, _ = cluster_dev(ctx, pair, first, 256, 6)
    assert all(cm[0, c0[j]] == cm[1, c1[j]] == j for j in range(6))


# ---- all 2,049 items live ----

def test_all_items_live_recovers_the_planted_partition(ctx):
    """P = 8, every (phase, context) and the start of chunk live, rows drawn from 8 planted
    distributions (joint_fit_ref.planted_counts), max_models = 8: 2,041 merges over the full
    33.6-MB table, the lone last item 2,048 included.  The numpy reference, run once by hand on
    this fixture (about a minute), recovers the planted partition; only the planted truth is kept
    here."""
    pair, first, cls = J.planted_counts()
    assert (pair.sum(axis=2) > 0).all() and first.sum() > 0
    st, cm, fr, k, cost = cluster_dev(ctx, pair, first, 256, 8)
    assert st == N.RC_OK and k == 8
    truth = {frozenset(int(i) for i in np.flatnonzero(cls == j)) for j in range(8)}
    assert J.partition_joint(pair, first, cm, fr) == truth
    want = J.map_cost_joint(pair, first, cm, fr)
    print(f"all live: cost rel err {abs(cost - want) / want:.3e}")
    assert cost == pytest.approx(want, rel=1e-9)
    seen = []
    for r in np.concatenate([cm.ravel(), [fr]]):
        if r not in seen:
            seen.append(int(r))
    assert seen == sorted(seen) == list(range(8))


# ---- edges ----

def few_items():
    pair = np.zeros((2, 256, 256), np.int64)
    pair[0, 3, 5] = 10
    pair[1, 200, 7] = 4
    pair[1, 9, 5] = 1
    first = np.zeros(256, np.int64)
    first[1] = 2
    return pair, first


def test_no_merge_when_models_cover_the_live_items(ctx):
    pair, first = few_items()
    for K in (4, 64):
        st, cm, fr, k, cost = cluster_dev(ctx, pair, first, 256, K)
        assert st == N.RC_OK and k == 4  # items 3, 256 + 9, 256 + 200 and the start of chunk
        assert (cm[0, 3], cm[1, 9], cm[1, 200], fr) == (0, 1, 2, 3)
        assert cost == 0.0  # every row holds one symbol
        # an item without samples lands in the row with the largest total: row 0 (10 samples)
        rest = np.delete(cm.ravel(), [3, 256 + 9, 256 + 200])
        assert (rest == 0).all()


def test_items_without_samples_get_the_lowest_largest_row(ctx):
    pair = np.zeros((2, 256, 256), np.int64)
    pair[0, 10, 1] = 5
    pair[0, 20, 2] = 50
    pair[1, 30, 3] = 50  # as large as row 1, but a higher row
    pair[1, 40, 4] = 7
    st, cm, fr, k, _ = cluster_dev(ctx, pair, np.zeros(256, np.int64), 256, 64)
    assert st == N.RC_OK and k == 4
    assert (cm[0, 10], cm[0, 20], cm[1, 30], cm[1, 40]) == (0, 1, 2, 3)
    # no first symbols: the start of chunk is an item without samples
    assert fr == 1 and cm[0, 0] == 1 and cm[1, 255] == 1 and cm[0, 255] == 1


def test_one_live_item(ctx):
    pair = np.zeros((4, 256, 256), np.int64)
    pair[2, 100, 0] = 3
    pair[2, 100, 255] = 1
    st, cm, fr, k, cost = cluster_dev(ctx, pair, np.zeros(256, np.int64), 256, 1)
    assert st == N.RC_OK and k == 1 and fr == 0 and (cm == 0).all()
    assert cost == pytest.approx(float(R.cost(np.array([3, 1]))), rel=1e-12)
    first = np.zeros(256, np.int64)
    first[0] = 1  # only the start of chunk: the last item alone
    st, cm, fr, k, cost = cluster_dev(ctx, np.zeros((8, 256, 256), np.int64), first, 256, 8)
    assert st == N.RC_OK and k == 1 and fr == 0 and (cm == 0).all() and cost == 0.0


def test_a_phase_without_counts(ctx):
    pair, first = J.sparse_counts(4, 61)
    pair[2] = 0
    maps, rfr, rk, rcost, _ = J.cluster_joint_ref(pair, first, 256, 8, want_lead=False)
    st, cm, fr, k, cost = cluster_dev(ctx, pair, first, 256, 8)
    assert st == N.RC_OK and k == rk and fr == rfr and np.array_equal(cm, maps)
    assert cost == pytest.approx(rcost, rel=1e-9)
    assert len(set(cm[2])) == 1  # every entry of the empty phase: the largest row


def test_null_cost_repeat_and_inputs_untouched(ctx):
    pair, first = J.sparse_counts(2, 62)
    pt, ft = dev(pair.copy()), dev(first.copy())
    cm = np.zeros((2, 2, 256), np.uint8)
    fr, k = (ctypes.c_uint32(), ctypes.c_uint32()), (ctypes.c_uint32(), ctypes.c_uint32())
    cost = ctypes.c_double()
    ctx.bind_stream()
    call = ctx._lib.rc_cluster_contexts_dev
    assert call(ctx.handle, 2, _ptr(pt), _ptr(ft), 256, 5, ctypes.c_void_p(cm[0].ctypes.data),
                ctypes.byref(fr[0]), ctypes.byref(k[0]), None) == N.RC_OK  # cost_bits_out null
    assert call(ctx.handle, 2, _ptr(pt), _ptr(ft), 256, 5, ctypes.c_void_p(cm[1].ctypes.data),
                ctypes.byref(fr[1]), ctypes.byref(k[1]), ctypes.byref(cost)) == N.RC_OK
    assert np.array_equal(cm[0], cm[1]) and fr[0].value == fr[1].value
    assert k[0].value == k[1].value == 5
    st, cm3, fr3, k3, cost3 = cluster_dev(ctx, pair, first, 256, 5)
    assert np.array_equal(cm3, cm[0]) and cost3 == cost.value  # bit for bit
    torch.cuda.synchronize()
    assert np.array_equal(pt.cpu().numpy(), pair) and np.array_equal(ft.cpu().numpy(), first)


def test_counts_straight_from_the_pair_histogram(ctx):
    """64 chunks of 1 KiB through rc_histogram_pairs_periodic, clustered where they lie."""
    rng = np.random.default_rng(63)
    n, L, P = 64, 1024, 4
    rec = np.stack([rng.integers(0, 12, n * L // 4), rng.integers(0, 3, n * L // 4),
                    rng.integers(100, 104, n * L // 4), np.zeros(n * L // 4, np.int64)], axis=1)
    syms = dev(rec.astype(np.uint8).ravel())
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    pair_t, first_t = mb.histogram_pairs_periodic(syms, off, P, ctx=ctx)
    cm, fr, k, cost = mb.cluster_contexts_joint(pair_t, first_t, 6, ctx=ctx)
    pair, first = pair_t.cpu().numpy(), first_t.cpu().numpy()
    assert pair.sum() == n * (L - 1) and first.sum() == n
    maps, rfr, rk, rcost, _ = J.cluster_joint_ref(pair, first, 256, 6, want_lead=False)
    assert cm.shape == (P, 256) and cm.dtype == np.uint8
    assert np.array_equal(cm, maps) and (fr, k) == (rfr, rk)
    assert cost == pytest.approx(rcost, rel=1e-9)
    # [256, 256] in, [n_symbols] out; the wrapper's errors
    cm1, _, k1, _ = mb.cluster_contexts_joint(pair_t.sum(dim=0), first_t, 3, 104, ctx=ctx)
    assert cm1.shape == (104,) and k1 == 3
    with pytest.raises(ValueError, match="symbols >= 100 present"):
        mb.cluster_contexts_joint(pair_t, first_t, 6, 100, ctx=ctx)
    with pytest.raises(ValueError, match="empty counts"):
        mb.cluster_contexts_joint(torch.zeros_like(pair_t), torch.zeros_like(first_t), 6, ctx=ctx)
    with pytest.raises(ValueError):
        mb.cluster_contexts_joint(pair_t[:3].contiguous(), first_t, 6, ctx=ctx)


# ---- statuses ----

def test_statuses_from_the_device(ctx):
    pair, first = J.sparse_counts(4, 64, n=100)
    assert cluster_dev(ctx, pair, first, 100, 6)[0] == N.RC_OK
    for ph, p, s in ((1, 100, 0), (2, 0, 100), (3, 255, 255)):
        bad = pair.copy()
        bad[ph, p, s] = 1
        assert cluster_dev(ctx, bad, first, 100, 6)[0] == N.RC_E_BAD_SYMBOL, (ph, p, s)
    badf = first.copy()
    badf[100] = 1
    assert cluster_dev(ctx, pair, badf, 100, 6)[0] == N.RC_E_BAD_SYMBOL
    z = np.zeros_like(pair)
    assert cluster_dev(ctx, z, np.zeros(256, np.int64), 100, 6)[0] == N.RC_E_BAD_MODEL
    assert cluster_dev(ctx, pair, first, 100, 0)[0] == N.RC_E_ARG
    assert cluster_dev(ctx, pair, first, 100, 65)[0] == N.RC_E_ARG
    assert cluster_dev(ctx, pair, first, 0, 6)[0] == N.RC_E_ARG
    assert cluster_dev(ctx, pair, first, 257, 6)[0] == N.RC_E_ARG
    assert cluster_dev(ctx, pair[:3], first, 100, 6, period=3)[0] == N.RC_E_ARG
    big = np.zeros((2, 256, 256), np.int64)
    big[0, 1, 2] = big[1, 3, 4] = 1 << 62  # the sum reaches 2^63
    assert cluster_dev(ctx, big, np.zeros(256, np.int64), 256, 6)[0] == N.RC_E_ARG
    big[1, 3, 4] -= 1
    assert cluster_dev(ctx, big, np.zeros(256, np.int64), 256, 6)[0] == N.RC_OK
    # null pointers
    pt, ft = dev(pair), dev(first)
    cm = np.zeros((4, 256), np.uint8)
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    args = [ctx.handle, 4, _ptr(pt), _ptr(ft), 100, 6, ctypes.c_void_p(cm.ctypes.data),
            ctypes.byref(a), ctypes.byref(b), None]
    ctx.bind_stream()
    call = ctx._lib.rc_cluster_contexts_dev
    assert call(*args) == N.RC_OK
    for i in (0, 2, 3, 6, 7, 8):
        bad = list(args)
        bad[i] = None
        assert call(*bad) == N.RC_E_ARG, i


# ---- fit_order1_set(joint=True) ----

def _coded_bytes(o1, syms, sym_off, L):
    n = sym_off.numel() - 1
    cap = rc.slot_capacity(L, 17.0)
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    out_len, fl = rc.encode_batch_order1(o1, syms, sym_off, out, out_off)
    dec = torch.zeros_like(syms)
    fd = rc.decode_batch_order1(o1, out, out_off[:-1].contiguous(), out_len, dec, sym_off)
    torch.cuda.synchronize()
    assert int(fl.abs().sum()) == 0 and int(fd.abs().sum()) == 0
    assert torch.equal(dec, syms)  # the round trip is exact
    return int(out_len.sum())


def test_the_joint_fit_beats_the_per_phase_fit(ctx):
    """2^18 bytes of int32 uniform in [0, 3000) as 16-KiB chunks, period 4, 8 rows.  On this
    input the numpy references give the joint clustering a lower cost than the four per-phase
    clusterings of two rows each (test_joint_fit_ref.py asserts it on the CPU): the two always-zero
    bytes need one row between them, not four."""
    L = 16384
    syms = dev(J.int32_records())
    n = syms.numel() // L
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    joint = rc.fit_order1_set(syms, sym_off, n_models=8, period=4, joint=True)
    per = rc.fit_order1_set(syms, sym_off, n_models=8, period=4)
    assert joint.period == 4 and joint.n_models == 8 and joint.ctx_map.shape == (4, 256)
    b_joint = _coded_bytes(joint, syms, sym_off, L)
    b_per = _coded_bytes(per, syms, sym_off, L)
    ideal = float(rc.ideal_bits_order1(joint, syms, sym_off).sum())
    print(f"joint {b_joint} B, per phase {b_per} B, ratio {b_joint / b_per:.4f}; ideal bits "
          f"{ideal:.0f}, payload / ideal {8 * b_joint / ideal:.5f}")
    assert np.isfinite(ideal) and ideal <= 8 * b_joint <= 1.02 * ideal
    assert b_joint < b_per
    # fewer rows than phases: joint only
    two = rc.fit_order1_set(syms, sym_off, n_models=2, period=4, joint=True)
    assert two.n_models == 2 and _coded_bytes(two, syms, sym_off, L) > b_joint
    with pytest.raises(ValueError):
        rc.fit_order1_set(syms, sym_off, n_models=2, period=4)
    for m in (joint, per, two):
        m.close()


def test_joint_fit_at_period_1_equals_the_host_fit(ctx):
    chunks = R.markov_chunks(4, 16, 2048)
    syms = dev(np.concatenate(chunks))
    off = torch.arange(17, dtype=torch.int64, device="cuda") * 2048
    a = rc.fit_order1_set(syms, off, n_models=4, joint=True)
    b = rc.fit_order1_set(syms, off, n_models=4)
    assert a.period == 1 and a.n_models == b.n_models == 4 and a.first_row == b.first_row
    assert np.array_equal(a.ctx_map, b.ctx_map) and np.array_equal(a.c, b.c)
    a.close()
    b.close()
