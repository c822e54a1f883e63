"""Expected results of rc_cluster_contexts_dev in plain numpy: order1_fit_ref.cluster_ref over the
256 P + 1 items of periodic pair counts (item ph * 256 + p is row [ph][p], item 256 P the start of
chunk), with the delta taken as cost(a + b) - (cost(a) + cost(b)), and the `lead` of a fixture:
how far the chosen merge was ahead of its closest rival that is not an exact tie, relative to the
cost the deltas are differences of.  Fixtures and helpers the CPU and the GPU tests share."""
import numpy as np

import order1_fit_ref as R


def items(pair, first):
    """(V[I, 256] f64, P): the count rows of the items."""
    pair = np.asarray(pair)
    if pair.ndim == 2:
        pair = pair[None]
    P = pair.shape[0]
    assert pair.shape == (P, 256, 256)
    return np.concatenate([pair.reshape(P * 256, 256).astype(np.float64),
                           np.asarray(first, np.float64)[None, :]]), P


def cluster_joint_ref(pair, first, n_symbols=256, max_models=64, want_lead=True):
    """(maps[P, 256], first_row, n_models, cost_bits, lead).  The rule of cluster_ref: one cluster
    per item with samples in the slot of its smallest member; while more than max_models remain
    the pair (a, b), a < b, with the smallest delta is merged, the first minimum in row-major
    order; rows by ascending smallest member; an item without samples gets the lowest row with
    the largest total; map entries from n_symbols on are 0.

    lead: the smallest, over the merges, of (d2 - d1) / max(1, C), d1 the chosen delta, d2 the
    smallest delta of a live pair that is not an exact tie of the chosen pair (one whose merged
    counts and whose two costs are the chosen pair's: such pairs get the same delta from any
    implementation of the formula, and the tie-break decides), C the larger of the two pairs'
    merged costs.  inf when no merge had a rival."""
    V, P = items(pair, first)
    I = 256 * P + 1
    tot = V.sum(axis=1)
    live = tot > 0
    assert live.any()
    slot = np.where(live, np.arange(I), I)
    c = R.cost(V)
    D = np.full((I, I), np.inf)

    def refresh(a):
        x = np.flatnonzero(live)
        x = x[x != a]
        d = R.cost(V[x] + V[a]) - (c[x] + c[a])
        lo = x < a
        D[x[lo], a] = d[lo]
        D[a, x[~lo]] = d[~lo]

    def rival(a, b):
        """(d2, merged cost of that pair) of the closest pair that is no exact tie of (a, b)."""
        idx = np.flatnonzero(live)
        sub = D[np.ix_(idx, idx)].ravel()
        k = min(len(sub), 64)
        while True:
            cand = np.argpartition(sub, k - 1)[:k] if k < len(sub) else np.arange(len(sub))
            cand = cand[np.argsort(sub[cand], kind="stable")]
            merged = V[a] + V[b]
            costs = sorted((c[a], c[b]))
            for f in cand:
                if not np.isfinite(sub[f]):
                    return None
                x, y = idx[f // len(idx)], idx[f % len(idx)]
                if (x, y) == (a, b):
                    continue
                if np.array_equal(V[x] + V[y], merged) and sorted((c[x], c[y])) == costs:
                    continue
                return float(sub[f]), float(R.cost(V[x] + V[y]))
            if k == len(sub):
                return None
            k = min(len(sub), 8 * k)

    lead = np.inf
    if live.sum() > max_models:
        for a in np.flatnonzero(live):
            refresh(a)
    while live.sum() > max_models:
        a, b = divmod(int(np.argmin(D)), I)
        if want_lead:
            r = rival(a, b)
            if r is not None:
                big = max(1.0, r[1], float(R.cost(V[a] + V[b])))
                lead = min(lead, (r[0] - float(D[a, b])) / big)
        V[a] += V[b]
        tot[a] += tot[b]
        c[a] = R.cost(V[a])
        live[b] = False
        D[b, :] = np.inf
        D[:, b] = np.inf
        slot[slot == b] = a
        refresh(a)
    slots = np.flatnonzero(live)
    row = np.zeros(I + 1, np.int64)
    row[slots] = np.arange(len(slots))
    row[I] = int(np.argmax(tot[slots]))
    m = row[slot]
    maps = np.zeros((P, 256), np.uint8)
    maps[:, :n_symbols] = m[:P * 256].reshape(P, 256)[:, :n_symbols]
    return maps, int(m[P * 256]), len(slots), float(c[slots].sum()), float(lead)


def map_cost_joint(pair, first, maps, first_row):
    """The cost of given maps: the sum of cost(row) over the rows they pool the items into."""
    V, P = items(pair, first)
    rows = np.concatenate([np.asarray(maps, np.int64).reshape(P, -1)[:, :256].ravel(),
                           [int(first_row)]])
    return float(sum(R.cost(V[rows == j].sum(axis=0)) for j in np.unique(rows)))


def partition_joint(pair, first, maps, first_row):
    """order1_fit_ref.partition over the 256 P + 1 items: the partition the maps make of the items
    with samples, a set of frozensets of item numbers."""
    V, P = items(pair, first)
    tot = V.sum(axis=1)
    rows = np.concatenate([np.asarray(maps, np.int64).reshape(P, -1)[:, :256].ravel(),
                           [int(first_row)]])
    return {frozenset(int(i) for i in np.flatnonzero((rows == j) & (tot > 0)))
            for j in np.unique(rows[tot > 0])}


# ---- fixtures shared by test_joint_fit_ref.py (the lead, on the CPU) and the GPU tests ----

def sparse_counts(P, seed, n_live=24, n=256, scale=1):
    """Random sparse counts without planted structure: about n_live live contexts per phase among
    the first n, a fifth of their symbols (below n) counted, first symbols 0..4."""
    rng = np.random.default_rng(seed)
    pair = np.zeros((P, 256, 256), np.int64)
    for ph in range(P):
        live = rng.choice(n, n_live, replace=False)
        pair[ph, live, :n] = rng.integers(0, 50, (n_live, n)) * (rng.random((n_live, n)) < 0.2)
    first = np.zeros(256, np.int64)
    first[:n] = rng.integers(0, 5, n)
    return pair * scale, first * scale


def unstructured_p1():
    """test_order1_fit.py's unstructured sparse counts (40 live contexts)."""
    rng = np.random.default_rng(7)
    pair = np.zeros((256, 256), np.int64)
    live = rng.choice(256, 40, replace=False)
    pair[live] = rng.integers(0, 50, (40, 256)) * (rng.random((40, 256)) < 0.2)
    return pair, rng.integers(0, 5, 256)


def small_alphabet_p1():
    """test_order1_fit.py's n_symbols = 100 case."""
    rng = np.random.default_rng(3)
    pair = np.zeros((256, 256), np.int64)
    pair[:100, :100] = rng.integers(0, 9, (100, 100))
    first = np.zeros(256, np.int64)
    first[:100] = 1
    return pair, first


# (name, P, n_symbols, the K compared, counts): every case the GPU tests compare merge for merge
def merge_for_merge_cases():
    out = [("unstructured", 1, 256, (1, 5, 17), unstructured_p1()),
           ("alphabet100", 1, 100, (6,), small_alphabet_p1()),
           ("markov4", 1, 256, (4,), R.pair_counts_ref(R.markov_chunks(4, 16, 2048)))]
    for P in (2, 4, 8):
        ks = tuple(sorted({1, 8, 64} | ({P - 1} if P > 1 else set())))
        out.append((f"sparse_p{P}", P, 256, ks, sparse_counts(P, 40 + P)))
    out.append(("sparse_2p40", 2, 256, (8,), sparse_counts(2, 51, scale=(1 << 40) // 50)))
    out.append(("sparse_n100", 4, 100, (8,), sparse_counts(4, 52, n=100)))
    return out


def planted_counts(P=8, K=8, seed=5, per_row=4000):
    """Every one of the 256 P + 1 items live: item i draws per_row symbols from distribution
    (i * 2654435761 >> 7) % K, a Zipf(1.2) table rotated by 256 / K per distribution.  Returns
    (pair, first, cls[I])."""
    rng = np.random.default_rng(seed)
    I = 256 * P + 1
    w = 1.0 / np.arange(1, 257) ** 1.2
    w /= w.sum()
    cls = ((np.arange(I, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(K)
    cls = cls.astype(np.int64)
    V = np.stack([rng.multinomial(per_row, np.roll(w, (int(j) * 256) // K)) for j in cls])
    return V[:-1].reshape(P, 256, 256).astype(np.int64), V[-1].astype(np.int64), cls


def int32_records():
    """DESIGN.md §9.12's integer input: 2^16 int32 uniform in [0, 3000), as 2^18 bytes."""
    rng = np.random.default_rng(7)
    return rng.integers(0, 3000, 1 << 16).astype(np.int32).view(np.uint8)


def periodic_pair_counts_ref(chunks, P):
    """(pair[P, 256, 256], first[256]): pair[ph][p][s] counts the positions i >= 1 of a chunk with
    i % P == ph, sym[i-1] = p and sym[i] = s."""
    pair = np.zeros((P, 65536), np.int64)
    first = np.zeros(256, np.int64)
    for ch in chunks:
        s = np.asarray(ch, np.uint8).astype(np.int64)
        if len(s):
            first[s[0]] += 1
            ph = np.arange(1, len(s)) % P
            key = s[:-1] * 256 + s[1:]
            for q in range(P):
                pair[q] += np.bincount(key[ph == q], minlength=65536)
    return pair.reshape(P, 256, 256), first


def shared_rows_counts(P=4, seed=71):
    """Phase 0 holds 24 unstructured contexts; every later phase holds one context that has only
    ever seen symbol 0 (an always-zero byte of a record)."""
    pair, first = sparse_counts(P, seed)
    pair[1:] = 0
    for ph in range(1, P):
        pair[ph, 10 * ph, 0] = 1000 * ph
    return pair, first
