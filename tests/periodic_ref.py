"""Expected results of the order-1 batch coders on a periodic set (the position in a record joins
the context), from the CPU oracle as it stands: row_0 = first_row, row_i =
ctx_map[i mod P][sym[i-1]], i counted from the chunk's first symbol.  This is order1_ref with the
phase in derive_idx and in the decoder's row choice: the encoder is the indexed reference fed the
derived index stream; the decoder is the stream decoder, one symbol per call, the row of each
call taken from the position and the symbol the call before returned."""
import numpy as np

import indexed_ref
from oracle import cpu

tables = indexed_ref.tables


def maps256(ctx_map, n):
    """[P, 256] rows from a [P, >= n] map: entries from n on are row 0, as the kernels stage them
    (a chunk that meets one is flagged: what follows is unspecified)."""
    cm = np.asarray(ctx_map, np.uint8)
    assert cm.ndim == 2
    m = np.zeros((cm.shape[0], 256), np.uint8)
    m[:, :n] = cm[:, :n]
    return m


def derive_idx(ctx_map, first_row, syms, n):
    """The index stream of one chunk: first_row, then ctx_map[i mod P][previous symbol]."""
    syms = np.asarray(syms, np.int64)
    m = maps256(ctx_map, n)
    idx = np.empty(len(syms), np.uint8)
    if len(syms):
        idx[0] = first_row
        idx[1:] = m[np.arange(1, len(syms)) % len(m), syms[:-1]]
    return idx


def encode_ref(c, cum, total, ctx_map, first_row, syms):
    """One chunk: (flags, bytes); indexed_ref.encode_ref on the derived indexes."""
    idx = derive_idx(ctx_map, first_row, syms, c.shape[1])
    return indexed_ref.encode_ref(c, cum, total, syms, idx)


def decode_ref(c, cum, total, ctx_map, first_row, code, count):
    """One chunk: (flags, symbols decoded before the first flag)."""
    cm = np.asarray(ctx_map)
    P = len(cm)
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
        i += 1
        row = int(cm[i % P][int(s[0])])
    return f, out[:i]


def draw_markov(rng, c, ctx_map, first_row, L):
    """L symbols of the chain the periodic model describes: symbol i from the row that its
    position and its predecessor pick (inverse-CDF sampling from the rows' cumulative counts)."""
    c = np.asarray(c, np.int64)
    cm = np.asarray(ctx_map)
    P = len(cm)
    edges = np.cumsum(c, axis=1)
    u = rng.integers(0, int(edges[0, -1]), L)
    s = np.zeros(L, np.uint8)
    row = int(first_row)
    for i in range(L):
        s[i] = np.searchsorted(edges[row], u[i], side="right")
        row = int(cm[(i + 1) % P][s[i]])
    return s


def ideal_bits(c, total, ctx_map, first_row, syms):
    """sum over the chunk of log2(total / c[row_i][sym_i]) in f64, inf where c == 0 or the
    symbol lies outside the alphabet."""
    n = c.shape[1]
    syms = np.asarray(syms, np.int64)
    if not len(syms):
        return 0.0
    if (syms >= n).any():
        return float("inf")
    idx = derive_idx(ctx_map, first_row, syms, n).astype(np.int64)
    cc = c[idx, syms].astype(np.float64)
    if (cc == 0).any():
        return float("inf")
    return float(np.sum((np.log(float(total)) - np.log(cc)) / np.log(2.0)))


def pairs(chunks, P):
    """(pair[P, 256, 256], first[256]) of a list of uint8 chunks, exactly."""
    pair = np.zeros((P, 256, 256), np.int64)
    first = np.zeros(256, np.int64)
    for ch in chunks:
        ch = np.asarray(ch, np.int64)
        if len(ch):
            first[ch[0]] += 1
            np.add.at(pair, (np.arange(1, len(ch)) % P, ch[:-1], ch[1:]), 1)
    return pair, first
