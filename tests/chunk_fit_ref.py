"""The fit of a static chunk set, written once in plain NumPy: the rule that
range_coder_rust_amd.model_build.fit_chunk_set follows on the GPU.

Costs are integers in units of 2^-16 bit.  A row's cost table is round(65536 log2(total / c)); a
chunk's cost under a row is the dot product of its histogram with that table in 64 bits; its class
is the row of least cost, ties to the lowest row.

  start   row 0 = the pooled histogram, quantised with all_symbols, so every row codes every chunk
  split   until there are K rows: the chunk with the highest cost under its best row (ties: the
          lowest chunk id) seeds a new row from its own histogram; reassign; re-estimate every
          non-empty class from its members' summed histograms.  (A chunk that costs nothing ends
          the splitting: there is nothing left to gain.)
  Lloyd   at most `iters` rounds of reassign and re-estimate, stopping when the assignment repeats
  end     the chunks' classes under the final rows; rows without a member are dropped and the
          class ids compacted

`quantize` and `cost_table` are parameters so that a test can pin the exact equality of the GPU
fit with the library's own host functions (rc_quantize_counts, rc_cost_table), which may differ
from NumPy's log2 by one unit where the double sits on a rounding boundary."""
import numpy as np

COST_NONE = 0xFFFFFFFF


def cost_table(c, total):
    """round(65536 log2(total / c)) per symbol, COST_NONE where c == 0 (NumPy)"""
    c = np.asarray(c, dtype=np.uint64)
    out = np.full(len(c), COST_NONE, dtype=np.uint64)
    nz = c > 0
    out[nz] = np.rint(65536.0 * np.log2(float(total) / c[nz].astype(np.float64))).astype(np.uint64)
    return out.astype(np.uint32)


def chunk_costs(hists, tables):
    """[n, R] uint64: chunk k under row r; UINT64_MAX where the chunk counts a symbol the row
    cannot code"""
    h = np.asarray(hists, dtype=np.uint64).reshape(-1, 256)
    t = np.zeros((len(tables), 256), dtype=np.uint64)
    t[:] = COST_NONE
    for r, row in enumerate(tables):
        t[r, :len(row)] = row
    finite = np.where(t == COST_NONE, 0, t)
    cost = h @ finite.T  # (uint64 products and sums, wrapping like the kernel's)
    hit = (h != 0).astype(np.uint64) @ (t == COST_NONE).astype(np.uint64).T
    cost[hit > 0] = np.iinfo(np.uint64).max
    return cost


def assign(hists, tables):
    """(best row per chunk, its cost): argmin with ties to the lowest row"""
    cost = chunk_costs(hists, tables)
    best = np.argmin(cost, axis=1).astype(np.uint8)  # (the first minimum)
    return best, cost[np.arange(len(cost)), best]


def by_class(hists, class_of, K):
    """[K, 256] uint64: the members' histograms summed per class; ids >= K skipped"""
    out = np.zeros((K, 256), dtype=np.uint64)
    h = np.asarray(hists, dtype=np.uint64).reshape(-1, 256)
    cls = np.asarray(class_of).astype(np.int64)
    ok = cls < K
    np.add.at(out, cls[ok], h[ok])
    return out


def fit(hists, n_models, target_total, iters, quantize, cost_table=cost_table, trace=None):
    """hists: [n, 256] chunk histograms.  quantize(counts) -> c (uint32[256], every c >= 1,
    summing to target_total).  Returns (rows [K', 256] uint32, class_of uint8[n]); trace, a list,
    receives the summed best cost after every reassignment of the Lloyd rounds."""
    h = np.asarray(hists, dtype=np.uint64).reshape(-1, 256)
    n = len(h)
    rows = [np.asarray(quantize(h.sum(axis=0)), dtype=np.uint32)]

    def tables():
        return [cost_table(r, target_total) for r in rows]

    def reestimate(cls):
        sums = by_class(h, cls, len(rows))
        for r in range(len(rows)):
            if sums[r].any():
                rows[r] = np.asarray(quantize(sums[r]), dtype=np.uint32)

    cls = np.zeros(n, dtype=np.uint8)
    while len(rows) < n_models and n:
        cls, best = assign(h, tables())
        seed = int(np.argmax(best))  # (the first maximum: the lowest chunk id)
        if best[seed] == 0:
            break
        rows.append(np.asarray(quantize(h[seed]), dtype=np.uint32))
        cls, _ = assign(h, tables())
        reestimate(cls)
    for _ in range(iters):
        new, best = assign(h, tables())
        if trace is not None:
            trace.append(int(best.sum(dtype=np.uint64)))
        same = np.array_equal(new, cls)
        cls = new
        if same:
            break
        reestimate(cls)
    if n:
        cls, _ = assign(h, tables())
    used = [r for r in range(len(rows)) if (cls == r).any()] or [0]
    remap = np.zeros(len(rows), dtype=np.uint8)
    remap[used] = np.arange(len(used), dtype=np.uint8)
    return np.stack([rows[r] for r in used]), remap[cls]
