"""The numpy reference of the joint clustering (joint_fit_ref) on the CPU: at one phase it is
order1_fit_ref.cluster_ref and the host rc_cluster_contexts; a 9-item case worked by hand; rows
shared between phases; and the conditions on the inputs that the GPU tests of
test_gpu_joint_fit.py rest on: the lead of every fixture compared merge for merge, and the joint
cost below the per-phase cost on the fit's input."""
import ctypes

import numpy as np
import pytest

from range_coder_rust_amd import _native as N
import joint_fit_ref as J
import order1_fit_ref as R

SHAPES = [(4, 16, 2048), (8, 32, 2048), (8, 64, 4096)]  # test_order1_fit.py's recovery shapes


def cluster_host(pair, first, n_symbols=256, max_models=64):
    pair = np.ascontiguousarray(pair, np.uint64)
    first = np.ascontiguousarray(first, np.uint64)
    cm = np.full(256, 0xEE, np.uint8)
    fr, k, cost = ctypes.c_uint32(99), ctypes.c_uint32(99), ctypes.c_double(-1.0)
    st = N.load().rc_cluster_contexts(ctypes.c_void_p(pair.ctypes.data),
                                      ctypes.c_void_p(first.ctypes.data), n_symbols, max_models,
                                      ctypes.c_void_p(cm.ctypes.data), ctypes.byref(fr),
                                      ctypes.byref(k), ctypes.byref(cost))
    assert st == N.RC_OK
    return cm, int(fr.value), int(k.value), float(cost.value)


def check_period_1(pair, first, n, K):
    maps, fr, k, cost, _ = J.cluster_joint_ref(pair, first, n, K, want_lead=False)
    m, rfr, rk, rcost = R.cluster_ref(pair, first, n, K)
    assert maps.shape == (1, 256) and np.array_equal(maps[0], m) and (fr, k) == (rfr, rk)
    assert cost == pytest.approx(rcost, rel=1e-9)
    cm, hfr, hk, hcost = cluster_host(pair, first, n, K)
    assert np.array_equal(maps[0], cm) and (fr, k) == (hfr, hk)
    assert cost == pytest.approx(hcost, rel=1e-9)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_phase_is_the_existing_reference_and_the_host_call(shape):
    pair, first = R.pair_counts_ref(R.markov_chunks(*shape))
    check_period_1(pair, first, 256, shape[0])


def test_one_phase_on_unstructured_counts():
    pair, first = J.unstructured_p1()
    for K in (1, 5, 17):
        check_period_1(pair, first, 256, K)
    check_period_1(*J.small_alphabet_p1(), 100, 6)
    # a 3-D array with one phase is the same input
    a = J.cluster_joint_ref(pair[None], first, 256, 5, want_lead=False)
    b = J.cluster_joint_ref(pair, first, 256, 5, want_lead=False)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_nine_items_by_hand():
    """P = 2, n_symbols = 4: items 0..3 (phase 0), 256..259 (phase 1), 512 (start of chunk).

        item   0: [4 0 0 0]   cost 0        item 256: [8 0 0 0]   cost 0
        item   1: [0 4 0 0]   cost 0        item 257: [1 1 0 0]   cost 2
        item   2: [2 2 0 0]   cost 4        item 259: [0 0 0 6]   cost 0
        item 512: [0 2 0 0]   cost 0        items 3 and 258: no samples

    Three pairs have delta exactly 0: (0, 256) -> [12 0 0 0], (1, 512) -> [0 6 0 0] and (2, 257)
    -> [3 3 0 0] (cost 6 = 4 + 2); every other delta is positive.  They merge in lexicographic
    order.  Then, among 0: [12 0 0 0], 1: [0 6 0 0], 2: [3 3 0 0] (cost 6) and 259: [0 0 0 6]:
        (1, 2) -> [3 9 0 0]: 3 * 2 + 9 log2(4/3) - 6 = 3.735, the smallest ((0, 2): 5.700,
        (1, 259) and (2, 259): 12, (0, 1) and (0, 259): 16.529);
    then, among 0, 1: [3 9 0 0] (cost 9.735) and 259:
        (0, 1) -> [15 9 0 0]: 15 log2(1.6) + 9 log2(8/3) - 9.735 = 13.171, the smallest (the other
        two: 16.529)."""
    pair = np.zeros((2, 256, 256), np.int64)
    pair[0, 0, :4] = (4, 0, 0, 0)
    pair[0, 1, :4] = (0, 4, 0, 0)
    pair[0, 2, :4] = (2, 2, 0, 0)
    pair[1, 0, :4] = (8, 0, 0, 0)
    pair[1, 1, :4] = (1, 1, 0, 0)
    pair[1, 3, :4] = (0, 0, 0, 6)
    first = np.zeros(256, np.int64)
    first[1] = 2
    cB = 6 + 9 * np.log2(4 / 3)
    # K: (phase 0's map, phase 1's map, first_row, cost); an item without samples takes the
    # lowest row with the largest total
    want = {
        7: ([0, 1, 2, 3], [3, 4, 3, 5], 6, 4.0 + 2.0),     # no merge; largest: 256 (8), row 3
        6: ([0, 1, 2, 0], [0, 3, 0, 4], 5, 6.0),           # (0, 256): 12 samples
        5: ([0, 1, 2, 0], [0, 3, 0, 4], 1, 6.0),           # (1, 512)
        4: ([0, 1, 2, 0], [0, 2, 0, 3], 1, 6.0),           # (2, 257)
        3: ([0, 1, 1, 0], [0, 1, 0, 2], 1, cB),            # (1, 2): 12 samples too, but row 1
        2: ([0, 0, 0, 0], [0, 0, 0, 1], 0, 15 * np.log2(1.6) + 9 * np.log2(8 / 3)),  # (0, 1)
    }
    for K, (m0, m1, fr, cost) in want.items():
        maps, rfr, k, rcost, _ = J.cluster_joint_ref(pair, first, 4, K, want_lead=False)
        assert k == K and rfr == fr, K
        assert list(maps[0, :4]) == m0 and list(maps[1, :4]) == m1, (K, maps[:, :4])
        assert (maps[:, 4:] == 0).all()
        assert rcost == pytest.approx(cost, rel=1e-12), K
        assert rcost == pytest.approx(J.map_cost_joint(pair, first, maps, rfr), rel=1e-12)
    assert J.cluster_joint_ref(pair, first, 4, 4)[4] == 0.0  # exact ties: no lead


def test_phases_share_the_rows():
    """Phases 1..3 each hold one context that has only seen symbol 0: the three merge first, at
    delta exactly 0.0, into one row, and phase 0 gets the other seven: its map is the one-phase
    clustering of its counts with 7 classes, which four rows a phase cannot give it."""
    pair, first = J.shared_rows_counts()
    maps, fr, k, cost, _ = J.cluster_joint_ref(pair, first, 256, 8, want_lead=False)
    assert k == 8 and maps[1, 10] == maps[2, 20] == maps[3, 30] == 7
    live0 = pair[0].sum(axis=1) > 0
    assert sorted(set(maps[0][live0]) | {fr}) == list(range(7))
    m7, fr7, k7, cost7 = R.cluster_ref(pair[0], first, 256, 7)
    assert np.array_equal(maps[0][live0], m7[live0]) and fr == fr7
    assert cost == pytest.approx(cost7, rel=1e-12)  # the shared row costs nothing
    # the first two merges, alone: 28 live items, 26 rows
    maps, fr, k, cost26, _ = J.cluster_joint_ref(pair, first, 256, 26, want_lead=False)
    assert k == 26 and maps[1, 10] == maps[2, 20] == maps[3, 30]
    assert cost26 == J.cluster_joint_ref(pair, first, 256, 28, want_lead=False)[3]  # delta 0.0


def test_lead_of_every_fixture_compared_merge_for_merge():
    """A condition on the inputs of test_gpu_joint_fit.py, not a measurement: a device delta
    carries at most about 300 * 2^-52 = 7e-14 of cost(a + b) in rounding, so a lead of 1e-9
    leaves four orders of magnitude."""
    cases = [(name, n, K, counts) for name, P, n, ks, counts in J.merge_for_merge_cases()
             for K in (min(ks),)]  # the smallest K runs every merge of the larger ones
    nophase = J.sparse_counts(4, 61)
    nophase[0][2] = 0
    cases += [("no phase 2", 256, 8, nophase), ("repeat", 256, 5, J.sparse_counts(2, 62))]
    for name, n, K, (pair, first) in cases:
        lead = J.cluster_joint_ref(pair, first, n, K)[4]
        print(f"{name}: K = {K}, lead {lead:.3e}")
        assert lead >= 1e-9, name


def test_joint_cost_is_below_the_per_phase_cost_on_the_fits_input():
    """2^18 bytes of int32 uniform in [0, 3000), 16-KiB chunks, period 4, 8 rows: the four
    per-phase clusterings of two rows each against the joint one, both by the references."""
    b = J.int32_records()
    pair, first = J.periodic_pair_counts_ref(b.reshape(-1, 16384), 4)
    per = sum(R.cluster_ref(pair[ph], first if ph == 0 else np.zeros(256, np.int64), 256, 2)[3]
              for ph in range(4))
    maps, fr, k, joint, _ = J.cluster_joint_ref(pair, first, 256, 8, want_lead=False)
    print(f"per phase {per:.1f} bits, joint {joint:.1f} bits")
    assert k == 8 and joint < per
    assert joint == pytest.approx(J.map_cost_joint(pair, first, maps, fr), rel=1e-12)


def test_planted_fixture_is_what_the_gpu_test_takes_it_for():
    pair, first, cls = J.planted_counts()
    assert pair.shape == (8, 256, 256) and len(cls) == 2049
    assert (pair.sum(axis=2) > 0).all() and first.sum() > 0
    sizes = np.bincount(cls, minlength=8)
    assert sizes.min() >= 200  # eight classes of about 256 items
    # the planted maps cost less than any coarser pooling of two classes
    maps, fr = cls[:-1].reshape(8, 256), int(cls[-1])
    c8 = J.map_cost_joint(pair, first, maps, fr)
    assert c8 < J.map_cost_joint(pair, first, np.where(maps == 7, 6, maps), min(fr, 6))
