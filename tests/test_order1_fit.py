"""rc_cluster_contexts (host only) against the numpy reference of order1_fit_ref: recovery of the
true context partition of the K-state Markov source, the reported cost, the
monotonicity and determinism of the greedy merge, and the edge cases of the interface."""
import ctypes
import time

import numpy as np
import pytest

from range_coder_rust_amd import _native as N
from range_coder_rust_amd import model_build as mb
import order1_fit_ref as R

SHAPES = [(4, 16, 2048), (8, 32, 2048), (8, 64, 4096)]


def cluster(pair, first, n_symbols=256, max_models=64, want_cost=True):
    """rc_cluster_contexts through ctypes: (status, ctx_map[256], first_row, n_models, cost)."""
    pair = np.ascontiguousarray(pair, np.uint64)
    first = np.ascontiguousarray(first, np.uint64)
    cm = np.full(256, 0xEE, np.uint8)
    fr, k, cost = ctypes.c_uint32(99), ctypes.c_uint32(99), ctypes.c_double(-1.0)
    st = N.load().rc_cluster_contexts(ctypes.c_void_p(pair.ctypes.data),
                                      ctypes.c_void_p(first.ctypes.data), n_symbols, max_models,
                                      ctypes.c_void_p(cm.ctypes.data), ctypes.byref(fr),
                                      ctypes.byref(k), ctypes.byref(cost) if want_cost else None)
    return st, cm, int(fr.value), int(k.value), float(cost.value)


@pytest.fixture(scope="module")
def counts():
    """{(K, chunks, L): (pair, first)} of the recovery shapes, drawn once."""
    return {sh: R.pair_counts_ref(R.markov_chunks(*sh)) for sh in SHAPES}


@pytest.mark.parametrize("shape", SHAPES)
def test_recovers_the_true_partition(counts, shape):
    K = shape[0]
    pair, first = counts[shape]
    _, true_map, true_first = R.markov_source(K)
    truth = R.partition(pair, first, true_map, true_first)
    true_cost = R.map_cost(pair, first, true_map, true_first)
    # the reference on its own seeded data: the true partition at the true map's cost, the
    # start of chunk in the class of context 0
    m, fr, k, cost = R.cluster_ref(pair, first, 256, K)
    assert k == K and R.partition(pair, first, m, fr) == truth
    assert cost == pytest.approx(true_cost, rel=1e-12)
    assert fr == m[0]
    # the library: the same partition
    st, cm, cfr, ck, _ = cluster(pair, first, 256, K)
    assert st == N.RC_OK and ck == K
    assert R.partition(pair, first, cm, cfr) == truth
    assert cfr == cm[0]
    # rows are numbered by ascending smallest member
    seen = []
    for r in cm:
        if r not in seen:
            seen.append(int(r))
    assert seen == sorted(seen)


def test_cost_is_the_cost_of_the_returned_map(counts):
    pair, first = counts[SHAPES[1]]
    for K in (1, 3, 8, 20, 64):
        st, cm, fr, k, cost = cluster(pair, first, 256, K)
        assert st == N.RC_OK and k == K
        assert cost == pytest.approx(R.map_cost(pair, first, cm, fr), rel=1e-9)
    st, cm2, fr2, k2, _ = cluster(pair, first, 256, 8, want_cost=False)  # cost_bits_out null
    assert st == N.RC_OK and k2 == 8


def test_cost_falls_with_more_models(counts):
    pair, first = counts[SHAPES[0]]
    costs = [cluster(pair, first, 256, K)[4] for K in range(1, 17)]
    for K in range(2, 17):
        assert costs[K - 1] <= costs[K - 2]


def test_two_calls_agree_and_the_call_is_quick(counts):
    pair, first = counts[SHAPES[2]]
    t0 = time.perf_counter()
    a = cluster(pair, first, 256, 2)
    dt = time.perf_counter() - t0
    b = cluster(pair, first, 256, 2)
    assert a[0] == N.RC_OK and b[0] == N.RC_OK
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert dt < 5.0  # about 250 merges from a table of deltas; a recompute of all pairs per merge
    #                  would take minutes


def test_follows_the_reference_on_unstructured_counts():
    """Random sparse counts with no planted structure: the same merges as the reference."""
    rng = np.random.default_rng(7)
    pair = np.zeros((256, 256), np.int64)
    live = rng.choice(256, 40, replace=False)
    pair[live] = rng.integers(0, 50, (40, 256)) * (rng.random((40, 256)) < 0.2)
    first = rng.integers(0, 5, 256)
    for K in (1, 5, 17):
        m, fr, k, cost = R.cluster_ref(pair, first, 256, K)
        st, cm, cfr, ck, ccost = cluster(pair, first, 256, K)
        assert st == N.RC_OK and ck == k
        assert np.array_equal(cm, m) and cfr == fr
        assert ccost == pytest.approx(cost, rel=1e-9)


def test_fewer_live_contexts_than_models():
    pair = np.zeros((256, 256), np.int64)
    pair[3, 5] = 10
    pair[200, 7] = 4
    pair[9, 5] = 1
    first = np.zeros(256, np.int64)
    first[1] = 2
    st, cm, fr, k, cost = cluster(pair, first, 256, 64)
    assert st == N.RC_OK and k == 4  # items 3, 9, 200 and the start of chunk
    assert (cm[3], cm[9], cm[200], fr) == (0, 1, 2, 3)
    # a context without samples lands in the row with the largest total count
    rest = np.delete(cm, [3, 9, 200])
    assert (rest == 0).all()
    assert cost == 0.0  # every row holds one symbol
    # no first symbols at all: the start of chunk is a context without samples
    st, cm, fr, k, _ = cluster(pair, np.zeros(256, np.int64), 256, 64)
    assert st == N.RC_OK and k == 3 and fr == 0


def test_largest_row_is_by_total_count():
    pair = np.zeros((256, 256), np.int64)
    pair[10, 1] = 5
    pair[20, 2] = 50
    pair[30, 3] = 7
    st, cm, fr, k, _ = cluster(pair, np.zeros(256, np.int64), 256, 64)
    assert st == N.RC_OK and k == 3
    assert cm[20] == 1 and cm[0] == 1 and cm[255] == 1 and fr == 1


def test_small_alphabet():
    rng = np.random.default_rng(3)
    pair = np.zeros((256, 256), np.int64)
    pair[:100, :100] = rng.integers(0, 9, (100, 100))
    first = np.zeros(256, np.int64)
    first[:100] = 1
    st, cm, fr, k, _ = cluster(pair, first, 100, 6)
    assert st == N.RC_OK and k == 6 and (cm[100:] == 0).all() and cm[:100].max() == 5
    m, rfr, _, _ = R.cluster_ref(pair, first, 100, 6)
    assert np.array_equal(cm, m) and fr == rfr
    for p, s in ((100, 0), (0, 100), (255, 255)):
        bad = pair.copy()
        bad[p, s] = 1
        assert cluster(bad, first, 100, 6)[0] == N.RC_E_BAD_SYMBOL
    badf = first.copy()
    badf[100] = 1
    assert cluster(pair, badf, 100, 6)[0] == N.RC_E_BAD_SYMBOL
    with pytest.raises(ValueError, match="symbols >= 100 present"):
        mb.cluster_contexts(pair, badf, 6, 100)


def test_refusals(counts):
    pair, first = counts[SHAPES[0]]
    z2, z1 = np.zeros((256, 256), np.int64), np.zeros(256, np.int64)
    assert cluster(z2, z1, 256, 8)[0] == N.RC_E_BAD_MODEL
    assert cluster(pair, first, 256, 0)[0] == N.RC_E_ARG
    assert cluster(pair, first, 256, 65)[0] == N.RC_E_ARG
    assert cluster(pair, first, 0, 8)[0] == N.RC_E_ARG
    assert cluster(pair, first, 257, 8)[0] == N.RC_E_ARG
    lib = N.load()
    p = np.ascontiguousarray(pair, np.uint64)
    f = np.ascontiguousarray(first, np.uint64)
    cm = np.zeros(256, np.uint8)
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    args = [ctypes.c_void_p(p.ctypes.data), ctypes.c_void_p(f.ctypes.data), 256, 8,
            ctypes.c_void_p(cm.ctypes.data), ctypes.byref(a), ctypes.byref(b), None]
    assert lib.rc_cluster_contexts(*args) == N.RC_OK
    for i in (0, 1, 4, 5, 6):
        bad = list(args)
        bad[i] = None
        assert lib.rc_cluster_contexts(*bad) == N.RC_E_ARG, i
    assert N.status_string(N.RC_E_BAD_SYMBOL) != "unknown status"


def test_one_model_is_an_all_zero_map(counts):
    pair, first = counts[SHAPES[0]]
    st, cm, fr, k, cost = cluster(pair, first, 256, 1)
    assert st == N.RC_OK and k == 1 and fr == 0 and (cm == 0).all()
    assert cost == pytest.approx(float(R.cost(pair.sum(axis=0) + first)), rel=1e-12)


def test_python_wrapper_and_null_context(counts):
    pair, first = counts[SHAPES[1]]
    cm, fr, k, cost = mb.cluster_contexts(pair, first, 8)
    st, want, wfr, wk, wcost = cluster(pair, first, 256, 8)
    assert cm.dtype == np.uint8 and np.array_equal(cm, want) and (fr, k, cost) == (wfr, wk, wcost)
    with pytest.raises(ValueError):
        mb.cluster_contexts(np.zeros((256, 256)), np.zeros(256), 8)
    lib = N.load()
    assert lib.rc_histogram_pairs(None, None, None, 0, None, None) == N.RC_E_ARG
    assert lib.rc_ideal_bits_order1(None, None, None, None, 0, None) == N.RC_E_ARG


def test_pair_counts_reference():
    """The reference's pair counts on a case small enough to count by hand."""
    pair, first = R.pair_counts_ref([[1, 2, 1, 2], [], [2], [2, 1]])
    assert first[1] == 1 and first[2] == 2 and first.sum() == 3
    assert pair[1, 2] == 2 and pair[2, 1] == 2 and pair.sum() == 4
