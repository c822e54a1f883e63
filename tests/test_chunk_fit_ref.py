"""The NumPy reference of the chunk-set fit (tests/chunk_fit_ref.py) on seeded mixtures: the cost
never rises over the Lloyd rounds, one row is the pooled table, and the two-source mixture is
taken apart into its sources.  No device needed: the quantiser is rc_quantize_counts (host)."""
import numpy as np

from range_coder_rust_amd import model_build as MB
import chunk_fit_cases as C
import chunk_fit_ref as R

TOTAL = 1 << 16


def quant(counts):
    return MB.quantize_counts(np.asarray(counts, np.uint64), TOTAL, all_symbols=True)[0]


def ideal_bytes(hists, rows, cls):
    cost = R.chunk_costs(hists, [R.cost_table(r, TOTAL) for r in rows])
    return int(cost[np.arange(len(cost)), cls].sum(dtype=np.uint64)) / 65536.0 / 8.0


def test_cost_never_rises():
    for chunks, _ in (C.two_source(), C.four_source()):
        h = C.histograms(chunks)
        for K in (2, 4, 8):
            trace = []
            R.fit(h, K, TOTAL, 8, quant, trace=trace)
            assert len(trace) >= 1
            assert all(b <= a for a, b in zip(trace, trace[1:])), (K, trace)


def test_one_row_is_the_pooled_table():
    chunks, _ = C.two_source()
    h = C.histograms(chunks)
    rows, cls = R.fit(h, 1, TOTAL, 8, quant)
    assert rows.shape == (1, 256) and not cls.any()
    assert np.array_equal(rows[0], quant(h.sum(axis=0)))  # build_model's table


def test_two_sources_are_recovered():
    """96 chunks of 1,024 symbols, 40 % Zipf(1.2) and 60 % its mirror image (default_rng(7)).
    Measured with rc_quantize_counts: 74,239 ideal bytes with one row, 65,014 with two (0.8757),
    64,963 with four.  The bound is that ratio plus 0.01."""
    chunks, labels = C.two_source()
    h = C.histograms(chunks)
    rows1, cls1 = R.fit(h, 1, TOTAL, 8, quant)
    rows2, cls2 = R.fit(h, 2, TOTAL, 8, quant)
    rows4, cls4 = R.fit(h, 4, TOTAL, 8, quant)
    assert len(rows2) == 2
    # the partition is the sources', up to the names of the classes
    assert np.array_equal(cls2, labels) or np.array_equal(cls2, 1 - labels)
    b1, b2, b4 = (ideal_bytes(h, r, c) for r, c in ((rows1, cls1), (rows2, cls2), (rows4, cls4)))
    print(f"ideal bytes: K=1 {b1:.0f}, K=2 {b2:.0f} ({b2 / b1:.4f}), K=4 {b4:.0f}")
    assert b2 / b1 <= 0.8757 + 0.01
    assert b4 <= b2


def test_more_rows_than_sources():
    """K = 8 on four sources: whatever rows survive, every one has a member, the ids are
    compacted, and the fit costs no more than the pooled table"""
    chunks, _ = C.four_source()
    h = C.histograms(chunks)
    rows, cls = R.fit(h, 8, TOTAL, 8, quant)
    assert 1 <= len(rows) <= 8 and cls.max() == len(rows) - 1
    assert set(np.unique(cls)) == set(range(len(rows)))
    rows1, cls1 = R.fit(h, 1, TOTAL, 8, quant)
    assert ideal_bytes(h, rows, cls) <= ideal_bytes(h, rows1, cls1)


def test_cost_helpers():
    h = np.zeros((3, 256), np.uint64)
    h[0, 5] = 4
    h[1, 7] = 1
    t = [np.full(256, 10, np.uint32), np.full(256, 10, np.uint32)]
    t[0][7] = R.COST_NONE
    cost = R.chunk_costs(h, t)
    assert cost.tolist() == [[40, 40], [np.iinfo(np.uint64).max, 10], [0, 0]]
    best, bc = R.assign(h, t)
    assert best.tolist() == [0, 1, 0] and bc.tolist() == [40, 10, 0]  # ties: the lowest row
    assert R.by_class(h, np.array([0, 1, 9]), 2)[:, [5, 7]].tolist() == [[4, 0], [0, 1]]
