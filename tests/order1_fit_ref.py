"""Expected results of fitting an order-1 set (rc_histogram_pairs, rc_cluster_contexts,
rc_ideal_bits_order1), in plain numpy: the pair counts, the greedy agglomerative clustering under
the empirical-entropy cost with the library's merge rule and tie-break, the cost of a given map,
the ideal bits of a chunk, and the K-state Markov source of DESIGN.md §9.7 that the recovery tests
draw from."""
import numpy as np

from range_coder_rust_amd import synth

ITEMS = 257  # the 256 contexts and the pseudo-context 256, "start of chunk"


def pair_counts_ref(chunks):
    """(pair[256, 256], first[256]) of a list of uint8 chunks: pair[p][s] counts the positions
    i >= 1 of a chunk with sym[i-1] = p and sym[i] = s, first[s] the non-empty chunks that begin
    with s.  Chunk boundaries reset the context."""
    pair = np.zeros(65536, np.int64)
    first = np.zeros(256, np.int64)
    for ch in chunks:
        s = np.asarray(ch, np.uint8).astype(np.int64)
        if len(s):
            first[s[0]] += 1
            pair += np.bincount(s[:-1] * 256 + s[1:], minlength=65536)
    return pair.reshape(256, 256), first


def cost(v):
    """sum over v_s > 0 of v_s * log2(sum(v) / v_s), f64; rows of a 2-D array at once."""
    v = np.asarray(v, np.float64)
    n = v.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(v > 0, v * np.log2(n / v), 0.0)
    return t.sum(axis=-1)


def cluster_ref(pair, first, n_symbols=256, max_models=64):
    """The greedy clustering: (ctx_map[256], first_row, n_models, cost_bits).  One cluster per
    item with samples, kept in the slot of its smallest member; while more than max_models
    remain, the pair (a, b), a < b, with the smallest cost(a + b) - cost(a) - cost(b) is merged
    (np.argmin over the slots in row-major order: the first minimum is the lexicographically
    smallest pair); rows by ascending smallest member; items without samples get the row with the
    largest total (the lowest on ties); map entries from n_symbols on are 0."""
    V = np.concatenate([np.asarray(pair, np.float64), np.asarray(first, np.float64)[None, :]])
    tot = V.sum(axis=1)
    live = tot > 0
    assert live.any()
    slot = np.where(live, np.arange(ITEMS), ITEMS)
    c = cost(V)
    D = np.full((ITEMS, ITEMS), np.inf)

    def refresh(a):
        x = np.flatnonzero(live)
        x = x[x != a]
        d = cost(V[x] + V[a]) - c[x] - c[a]
        lo = x < a
        D[x[lo], a] = d[lo]
        D[a, x[~lo]] = d[~lo]

    if live.sum() > max_models:
        for a in np.flatnonzero(live):
            refresh(a)
    while live.sum() > max_models:
        a, b = divmod(int(np.argmin(D)), ITEMS)
        V[a] += V[b]
        tot[a] += tot[b]
        c[a] = cost(V[a])
        live[b] = False
        D[b, :] = np.inf
        D[:, b] = np.inf
        slot[slot == b] = a
        refresh(a)
    slots = np.flatnonzero(live)
    row = np.zeros(ITEMS + 1, np.int64)
    row[slots] = np.arange(len(slots))
    row[ITEMS] = int(np.argmax(tot[slots]))
    m = row[slot]
    ctx_map = np.zeros(256, np.uint8)
    ctx_map[:n_symbols] = m[:n_symbols]
    return ctx_map, int(m[256]), len(slots), float(c[slots].sum())


def map_cost(pair, first, ctx_map, first_row):
    """The cost of a given map: the sum of cost(row) over the rows the map pools the items into."""
    V = np.concatenate([np.asarray(pair, np.float64), np.asarray(first, np.float64)[None, :]])
    rows = np.concatenate([np.asarray(ctx_map, np.int64)[:256], [int(first_row)]])
    return float(sum(cost(V[rows == j].sum(axis=0)) for j in np.unique(rows)))


def partition(pair, first, ctx_map, first_row):
    """The partition a map makes of the items that have samples (256 = start of chunk): a set of
    frozensets, independent of the rows' numbering."""
    tot = np.concatenate([np.asarray(pair).sum(axis=1), [np.asarray(first).sum()]])
    rows = np.concatenate([np.asarray(ctx_map, np.int64)[:256], [int(first_row)]])
    return {frozenset(int(i) for i in np.flatnonzero((rows == j) & (tot > 0)))
            for j in np.unique(rows[tot > 0])}


def markov_source(K):
    """(rows[K, 256], ctx_map[256], first_row) of the K-state source: row j is the Zipf(1.2)
    table over 256 symbols (total 65536) rotated by j * 256 / K, symbol s selects row
    s * K >> 8, every chunk starts in row 0."""
    c, _, total = synth.zipf_table()
    assert total == 65536
    rows = np.stack([np.roll(np.asarray(c, np.int64), (j * 256) // K) for j in range(K)])
    return rows, ((np.arange(256) * K) >> 8).astype(np.uint8), 0


def markov_chunks(K, n_chunks, L, seed=1):
    """n_chunks chunks of L symbols of markov_source(K): one uniform vector per chunk from
    numpy.random.default_rng(seed), inverse-CDF sampling from the row the previous symbol picks."""
    rows, ctx_map, first_row = markov_source(K)
    edges = np.cumsum(rows, axis=1).astype(np.float64) / 65536.0
    rng = np.random.default_rng(seed)
    u = np.stack([rng.random(L) for _ in range(n_chunks)])
    s = np.zeros((n_chunks, L), np.uint8)
    row = np.full(n_chunks, first_row, np.int64)
    for i in range(L):  # one step of every chunk's chain at a time
        s[:, i] = np.minimum((edges[row] <= u[:, i, None]).sum(axis=1), 255)
        row = ctx_map[s[:, i]].astype(np.int64)
    return list(s)


def ideal_bits_ref(chunks, c_rows, total, ctx_map, first_row):
    """Per chunk the f64 sum of (ln total - ln c[row_i][s_i]) / ln 2, row_0 = first_row and
    row_i = ctx_map[s_(i-1)] (row 0 after a symbol outside the alphabet, as the coders stage the
    map); +inf where a term has c == 0 or a symbol >= n; 0.0 for an empty chunk."""
    c = np.asarray(c_rows, np.float64)
    K, n = c.shape
    icl = np.full((K, 256), np.inf)
    with np.errstate(divide="ignore"):
        icl[:, :n] = np.where(c > 0, (np.log(float(total)) - np.log(c)) / np.log(2.0), np.inf)
    m = np.zeros(256, np.int64)
    m[:n] = np.asarray(ctx_map, np.int64)[:n]
    out = []
    for ch in chunks:
        s = np.asarray(ch, np.uint8).astype(np.int64)
        if not len(s):
            out.append(0.0)
            continue
        rows = np.concatenate([[int(first_row)], m[s[:-1]]])
        out.append(float(np.sum(icl[rows, s])))
    return np.array(out, np.float64)
