"""Expected results of the indexed batch coders (a model chosen per symbol), from the CPU
oracle as it stands: the reference's encoder.encode(&models[idx[i]], sym[i]) is the stream
encoder fed the triple of row idx[i]; decoder.decode(&models[idx[i]]) is the stream decoder,
one call per run of equal indexes (the state carries over between calls)."""
import numpy as np

from oracle import cpu

F_BAD_SYMBOL = cpu.F_BAD_SYMBOL
F_BAD_MODEL = cpu.F_BAD_MODEL


def tables(c_rows):
    """(c, cum) as K x n uint32 arrays from rows of frequencies."""
    c = np.ascontiguousarray(c_rows, dtype=np.uint32)
    cum = np.zeros_like(c)
    cum[:, 1:] = np.cumsum(c.astype(np.uint64), axis=1)[:, :-1].astype(np.uint32)
    return c, cum


def encode_ref(c, cum, total, syms, idx):
    """One chunk: (flags, bytes).  The first error wins: at a symbol the model is looked up
    first (an index >= K: BAD_MODEL), then the symbol in it (>= n_symbols: BAD_SYMBOL), then its
    frequency (ZERO_FREQ, from the oracle).  A flagged chunk's bytes are unspecified: b""."""
    syms = np.asarray(syms, np.int64)
    idx = np.asarray(idx, np.int64)
    assert len(syms) == len(idx)
    K, n = c.shape
    bad = np.flatnonzero((idx >= K) | (syms >= n))
    stop = int(bad[0]) if len(bad) else len(syms)
    j, s = idx[:stop], syms[:stop]
    tri = np.stack([c[j, s], cum[j, s], np.full(stop, total, np.uint32)], axis=1)
    f, b, _ = cpu.stream_encode(cpu.Stream.fresh(), tri.astype(np.uint32), finish=True)
    if f:
        return f, b""
    if stop < len(syms):
        return (F_BAD_MODEL if idx[stop] >= K else F_BAD_SYMBOL), b""
    return 0, b


def decode_ref(c, cum, total, code, idx):
    """One chunk: (flags, symbols decoded before the first error)."""
    idx = np.asarray(idx, np.int64)
    K = c.shape[0]
    st = cpu.Stream.fresh()
    # Decoder::new runs even for an empty chunk (a stream under 8 bytes is TRUNCATED)
    f, _ = cpu.stream_decode(st, c[0], cum[0], total, code, 0)
    out = []
    i = 0
    while not f and i < len(idx):
        if idx[i] >= K:
            f = F_BAD_MODEL
            break
        e = i
        while e < len(idx) and idx[e] == idx[i]:
            e += 1
        f, s = cpu.stream_decode(st, c[idx[i]], cum[idx[i]], total, code, e - i)
        out.append(s)
        i = e
    return f, (np.concatenate(out) if out else np.zeros(0, np.uint8))
