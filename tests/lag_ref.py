"""Expected results of the order-1 batch coders on a lagged set (the context is the symbol D
positions back), from the CPU oracle as it stands: row_i = first_row for i < D, row_i =
ctx_map[i mod P][sym[i-D]] for i >= D, i counted from the chunk's first symbol.  This is
periodic_ref with the lag in derive_idx, in the decoder's row choice, in ideal_bits and in pairs:
the encoder is the indexed reference fed the derived index stream; the decoder is the stream
decoder, one symbol per call, the row of each call taken from the position and the symbol the
call D calls before returned."""
import numpy as np

import indexed_ref
import periodic_ref
from oracle import cpu

tables = indexed_ref.tables
maps256 = periodic_ref.maps256


def derive_idx(ctx_map, first_row, syms, n, lag):
    """The index stream of one chunk: first_row `lag` times, then ctx_map[i mod P][sym[i-lag]]."""
    syms = np.asarray(syms, np.int64)
    m = maps256(ctx_map, n)
    D = int(lag)
    idx = np.empty(len(syms), np.uint8)
    idx[:D] = first_row
    if len(syms) > D:
        idx[D:] = m[np.arange(D, len(syms)) % len(m), syms[:-D]]
    return idx


def encode_ref(c, cum, total, ctx_map, first_row, syms, lag):
    """One chunk: (flags, bytes); indexed_ref.encode_ref on the derived indexes."""
    idx = derive_idx(ctx_map, first_row, syms, c.shape[1], lag)
    return indexed_ref.encode_ref(c, cum, total, syms, idx)


def decode_ref(c, cum, total, ctx_map, first_row, code, count, lag):
    """One chunk: (flags, symbols decoded before the first flag)."""
    cm = np.asarray(ctx_map)
    P, D = len(cm), int(lag)
    st = cpu.Stream.fresh()
    # Decoder::new runs even for an empty chunk (a stream under 8 bytes is TRUNCATED)
    f, _ = cpu.stream_decode(st, c[first_row], cum[first_row], total, code, 0)
    out = np.zeros(count, np.uint8)
    i = 0
    while not f and i < count:
        row = int(first_row) if i < D else int(cm[i % P][int(out[i - D])])
        f, s = cpu.stream_decode(st, c[row], cum[row], total, code, 1)
        if f:
            break
        out[i] = s[0]
        i += 1
    return f, out[:i]


def draw_markov(rng, c, ctx_map, first_row, L, lag):
    """L symbols of the chain the lagged model describes: symbol i from the row that its position
    and the symbol `lag` before it pick (inverse-CDF sampling from the rows' cumulative counts)."""
    c = np.asarray(c, np.int64)
    cm = np.asarray(ctx_map)
    P, D = len(cm), int(lag)
    edges = np.cumsum(c, axis=1)
    u = rng.integers(0, int(edges[0, -1]), L)
    s = np.zeros(L, np.uint8)
    for i in range(L):
        row = int(first_row) if i < D else int(cm[i % P][s[i - D]])
        s[i] = np.searchsorted(edges[row], u[i], side="right")
    return s


def ideal_bits(c, total, ctx_map, first_row, syms, lag):
    """sum over the chunk of log2(total / c[row_i][sym_i]) in f64, inf where c == 0 or the
    symbol lies outside the alphabet."""
    n = c.shape[1]
    syms = np.asarray(syms, np.int64)
    if not len(syms):
        return 0.0
    if (syms >= n).any():
        return float("inf")
    idx = derive_idx(ctx_map, first_row, syms, n, lag).astype(np.int64)
    cc = c[idx, syms].astype(np.float64)
    if (cc == 0).any():
        return float("inf")
    return float(np.sum((np.log(float(total)) - np.log(cc)) / np.log(2.0)))


def pairs(chunks, P, lag):
    """(pair[P, 256, 256], first[256]) of a list of uint8 chunks, exactly: pairs `lag` apart, the
    first `lag` symbols of every chunk in `first`."""
    D = int(lag)
    pair = np.zeros((P, 256, 256), np.int64)
    first = np.zeros(256, np.int64)
    for ch in chunks:
        ch = np.asarray(ch, np.int64)
        np.add.at(first, ch[:D], 1)
        if len(ch) > D:
            np.add.at(pair, (np.arange(D, len(ch)) % P, ch[:-D], ch[D:]), 1)
    return pair, first
