"""The expected result of rc_stream_decode_rows / rc_stream_encode_rows, from the CPU oracle, and
the tables and streams the row tests share.

decode_rows: oracle.cpu.stream_decode of ONE symbol per call on one Stream, each call with the
table of that symbol's row, after Decoder::new on a fresh state; a row index >= n_rows is
RC_F_BAD_MODEL before the symbol.  encode_rows: oracle.cpu.stream_encode on the triples gathered
from the rows, cut before the first symbol whose row index is >= n_rows (RC_F_BAD_MODEL) or whose
value is >= n_symbols (RC_F_BAD_SYMBOL)."""
import numpy as np

from oracle import cpu

F_BAD_MODEL = cpu.F_BAD_MODEL
F_BAD_SYMBOL = cpu.F_BAD_SYMBOL

SIZES = (1, 2, 63, 64, 65, 128, 129, 255, 256)
N_ROWS = 37


def decode_rows(st, c, cum, total, row_of, code, n=None):
    """st (cpu.Stream) advances over row_of[:n]; returns (flags, decoded symbols)."""
    row_of = np.asarray(row_of, np.uint32)
    n = len(row_of) if n is None else n
    out = []
    if st.flags:
        return int(st.flags), np.zeros(0, np.uint8)
    if st.stage == 0:  # Decoder::new, whatever the first symbol's row is
        f, _ = cpu.stream_decode(st, c[0], cum[0], int(total[0]), code, 0)
        if f:
            return f, np.zeros(0, np.uint8)
    for i in range(n):
        r = int(row_of[i])
        if r >= len(total):
            st.flags = F_BAD_MODEL
            break
        f, s = cpu.stream_decode(st, c[r], cum[r], int(total[r]), code, 1)
        if f:
            break
        out.append(int(s[0]))
    return int(st.flags), np.array(out, np.uint8)


def gather(c, cum, total, row_of, syms):
    """(flag, index) of the first symbol the two new checks stop at (0, len) if none, and the
    triples of the symbols before it."""
    row_of = np.asarray(row_of, np.uint32).astype(np.int64)
    syms = np.asarray(syms, np.uint8).astype(np.int64)
    bad_r = row_of >= len(total)
    bad_s = ~bad_r & (syms >= c.shape[1])
    bad = np.flatnonzero(bad_r | bad_s)
    e = int(bad[0]) if len(bad) else len(syms)
    flag = 0 if e == len(syms) else (F_BAD_MODEL if bad_r[e] else F_BAD_SYMBOL)
    r, s = row_of[:e], syms[:e]
    trip = np.stack([c[r, s], cum[r, s], total[r]], axis=1).astype(np.uint32) if e else \
        np.zeros((0, 3), np.uint32)
    return flag, e, trip


def encode_rows(st, c, cum, total, row_of, syms, finish=False, cap=None):
    """st advances; returns (flags, new bytes, per-symbol byte counts)."""
    flag, e, trip = gather(c, cum, total, row_of, syms)
    if cap is None:
        cap = 12 * len(syms) + (8 if finish else 0)
    f, b, nb = cpu.stream_encode(st, trip, finish=finish and not flag, cap=cap)
    if not f and flag:
        st.flags = flag
    return int(st.flags) if not f else f, b, nb


# ---- tables -------------------------------------------------------------------------------

def cum_of(c):
    c = np.asarray(c, np.uint64)
    run = np.cumsum(c, axis=1, dtype=np.uint64)
    cum = np.zeros_like(run)
    cum[:, 1:] = run[:, :-1]
    return cum.astype(np.uint32), run[:, -1]


def mixed_table(n_symbols, seed, n_rows=N_ROWS):
    """About 70% live symbols, counts up to 2^19, totals not powers of two.  Row 0 of every
    table has total 2^32 - 1 where the alphabet allows it (two symbols or more), row 1 total 1."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 1 << 19, (n_rows, n_symbols)).astype(np.uint64)
    c[rng.random((n_rows, n_symbols)) > 0.7] = 0
    c[np.arange(n_rows), rng.integers(0, n_symbols, n_rows)] |= 1  # a live symbol in every row
    tot = c.sum(axis=1)
    c[:, 0] += np.where((tot & (tot - 1)) == 0, np.where(tot == 1, 2, 1), 0).astype(np.uint64)
    if n_symbols >= 2:
        c[0, :] = np.maximum(c[0, :], 1)
        c[0, -1] += (1 << 32) - 1 - c[0].sum()
    c[1, :] = 0
    c[1, n_symbols // 2] = 1
    cum, total = cum_of(c)
    return c.astype(np.uint32), cum, total.astype(np.uint32)


def rare_table(n_symbols, seed, n_rows=N_ROWS):
    """c = 1 symbols beside one of 2^31: totals near 2^31, so a rare symbol leaves a range below
    2^48 and range_reduction_expansion fires."""
    rng = np.random.default_rng(seed)
    c = np.ones((n_rows, n_symbols), np.uint64)
    c[rng.random((n_rows, n_symbols)) > 0.8] = 0
    c[np.arange(n_rows), rng.integers(0, n_symbols, n_rows)] = 1 << 31
    cum, total = cum_of(c)
    return c.astype(np.uint32), cum, total.astype(np.uint32)


def shuffled_table(n_symbols, seed, n_rows=N_ROWS):
    """An inconsistent table: the mixed table's cum entries permuted inside each row (not
    monotone), its totals kept, and every c_freq at least 1, so that whatever symbol the bisection
    ends at can be coded and a stream goes on past its first symbols."""
    c, cum, total = mixed_table(n_symbols, seed, n_rows)
    rng = np.random.default_rng(seed + 1)
    cum = np.stack([rng.permutation(row) for row in cum])
    return np.maximum(c, 1), cum, total


def live_symbols(c, row_of, rng, rare_bias=False):
    """One symbol with c > 0 per entry of row_of (rare_bias: mostly the c == 1 ones)."""
    out = np.zeros(len(row_of), np.uint8)
    for i, r in enumerate(row_of):
        live = np.flatnonzero(c[r])
        if rare_bias and len(live) > 1 and rng.random() < 0.6:
            live = live[c[r][live] == c[r][live].min()]
        out[i] = live[rng.integers(0, len(live))]
    return out


def garbage_streams(seed, n=32):
    """The garbage set of one table: random streams of 72 B, of 2,400 B, and all-0xFF ones."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 3 == 0:
            out.append(rng.integers(0, 256, 72).astype(np.uint8).tobytes())
        elif k % 3 == 1:
            out.append(rng.integers(0, 256, 2400).astype(np.uint8).tobytes())
        else:
            out.append(b"\xff" * int(rng.integers(8, 200)))
    return out


GARBAGE_SYMBOLS = 120  # symbols asked of every garbage stream


def garbage_rows(seed, n_streams=32, n_rows=N_ROWS):
    rng = np.random.default_rng(seed + 7)
    return rng.integers(0, n_rows, (n_streams, GARBAGE_SYMBOLS)).astype(np.uint32)
