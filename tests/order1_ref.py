"""Expected results of the order-1 batch coders (the previous symbol picks the model), from the
CPU oracle as it stands: row_0 = first_row, row_i = ctx_map[sym[i-1]].  The encoder is the
indexed reference fed the derived index stream; the decoder is the stream decoder, one symbol per
call, the row of each call taken from the symbol the call before returned."""
import numpy as np

import indexed_ref
from oracle import cpu

tables = indexed_ref.tables


def derive_idx(ctx_map, first_row, syms, n):
    """The index stream of one chunk: first_row, then ctx_map[previous symbol]; row 0 after a
    symbol outside the alphabet (such a chunk is flagged: what follows is unspecified)."""
    syms = np.asarray(syms, np.int64)
    m = np.zeros(256, np.uint8)
    cm = np.asarray(ctx_map, np.uint8)[:n]
    m[:len(cm)] = cm
    idx = np.empty(len(syms), np.uint8)
    if len(syms):
        idx[0] = first_row
        idx[1:] = m[syms[:-1]]
    return idx


def encode_ref(c, cum, total, ctx_map, first_row, syms):
    """One chunk: (flags, bytes); indexed_ref.encode_ref on the derived indexes."""
    idx = derive_idx(ctx_map, first_row, syms, c.shape[1])
    return indexed_ref.encode_ref(c, cum, total, syms, idx)


def decode_ref(c, cum, total, ctx_map, first_row, code, count):
    """One chunk: (flags, symbols decoded before the first flag)."""
    st = cpu.Stream.fresh()
    # Decoder::new runs even for an empty chunk (a stream under 8 bytes is TRUNCATED)
    f, _ = cpu.stream_decode(st, c[first_row], cum[first_row], total, code, 0)
    out = np.zeros(count, np.uint8)
    row, i = int(first_row), 0
    while not f and i < count:
        f, s = cpu.stream_decode(st, c[row], cum[row], total, code, 1)
        if f:
            break
        out[i] = s[0]
        row = int(ctx_map[int(s[0])])
        i += 1
    return f, out[:i]


def markov_rows(rng, K, n, total, shape=1.2):
    """K rows over n symbols, every c >= 1, heavy-tailed and different per row."""
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        w = rng.pareto(shape, n) + 0.01
        rows[j] += rng.multinomial(total - n, w / w.sum())
    return rows


def draw_markov(rng, c, ctx_map, first_row, L):
    """L symbols of the chain the model describes: symbol i from the row its predecessor picks
    (inverse-CDF sampling from the rows' cumulative counts)."""
    c = np.asarray(c, np.int64)
    edges = np.cumsum(c, axis=1)
    u = rng.integers(0, int(edges[0, -1]), L)
    s = np.zeros(L, np.uint8)
    row = int(first_row)
    for i in range(L):
        s[i] = np.searchsorted(edges[row], u[i], side="right")
        row = int(ctx_map[s[i]])
    return s
