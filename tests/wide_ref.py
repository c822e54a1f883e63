"""Expected results of the wide batch coders (16-bit symbols, one static table of up to 4096
symbols), from the CPU oracles as they stand: the C oracle's batch calls code bytes, so the
encoder is its stream encoder fed each symbol's (c, cum, total) triple (alphabet-agnostic), and
the decoder is the literal port of the reference (oracle/ref_literal.py), whose FreqTable takes
any alphabet, with its panics mapped onto the project's flags."""
import numpy as np

from oracle import cpu, ref_literal as ref

F_BAD_SYMBOL = cpu.F_BAD_SYMBOL
F_ZERO_FREQ = cpu.F_ZERO_FREQ
F_TRUNCATED = cpu.F_TRUNCATED
F_CORRUPT = cpu.F_CORRUPT


def table(c_freq):
    """(c, cum, total) as uint32 arrays and an int from a list of frequencies."""
    c = np.ascontiguousarray(c_freq, dtype=np.uint32)
    cum = np.zeros_like(c)
    cum[1:] = np.cumsum(c.astype(np.uint64))[:-1].astype(np.uint32)
    return c, cum, int(c.astype(np.uint64).sum())


def encode_ref(c, cum, total, syms):
    """One chunk: (flags, bytes).  The first error wins: a symbol >= n_symbols is BAD_SYMBOL, a
    symbol with c == 0 ZERO_FREQ (from the oracle).  A flagged chunk's bytes are unspecified:
    b""."""
    syms = np.asarray(syms, np.int64)
    n = len(c)
    bad = np.flatnonzero(syms >= n)
    stop = int(bad[0]) if len(bad) else len(syms)
    s = syms[:stop]
    tri = np.stack([c[s], cum[s], np.full(stop, total, np.uint32)], axis=1)
    f, b, _ = cpu.stream_encode(cpu.Stream.fresh(), tri.astype(np.uint32), finish=True)
    if f:
        return f, b""
    if stop < len(syms):
        return F_BAD_SYMBOL, b""
    return 0, b


def literal_table(c):
    return ref.FreqTable.from_counts([int(x) for x in c])


def decode_ref(c, cum, total, code, n, lit=None):
    """One chunk: (flags, symbols decoded before the first error), uint16.  The reference's
    panics and its endless loop become flags: pop_front on an empty buffer (Decoder::new or
    shift_left_buffer) is TRUNCATED, a renormalisation that does not terminate (a symbol with
    c == 0 was selected) is CORRUPT.  The literal decoder stops at the first of them, so an
    over-read that came first wins."""
    lit = lit or literal_table(c)
    assert lit.total == total and list(lit.cum) == [int(x) for x in cum]
    out = []
    f = 0
    try:
        dec = ref.Decoder(bytes(code))
        for _ in range(n):
            out.append(dec.decode(lit))
    except ref.ReferencePanic as e:
        msg = str(e)
        if "pop_front" in msg:
            f = F_TRUNCATED
        elif "does not terminate" in msg:
            f = F_CORRUPT
        else:
            raise
    return f, np.array(out, dtype=np.uint16)
