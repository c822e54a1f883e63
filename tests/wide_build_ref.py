"""Expected results of wide model construction (rc_histogram_wide, rc_ideal_bits_wide), from
numpy and the CPU oracle (oracle/model_build.py) as they stand: the oracle's ideal_bits is fixed
to 256 bins, so ideal_bits_ref restates it for any alphabet (test_wide_build.py pins the two to
each other on 256-bin data)."""
import math

import numpy as np

from oracle import model_build as O


def hist_ref(syms, n_bins):
    """(counts[n_bins], out-of-range count) of uint16 symbols: symbols >= n_bins are counted in
    no bin."""
    s = np.asarray(syms, np.uint16).astype(np.int64)
    full = np.bincount(s, minlength=n_bins)
    return full[:n_bins].astype(np.int64), int(full[n_bins:].sum())


def ideal_bits_ref(chunks, c, total):
    """Per chunk (an array of symbols): the sum over bins in order of count *
    O.ideal_code_length(c[i], total); +inf where the chunk holds a symbol with c == 0 or a
    symbol >= len(c).  An empty chunk is 0.0."""
    n = len(c)
    icl = [O.ideal_code_length(int(c[i]), total) for i in range(n)]
    out = []
    for ch in chunks:
        counts, stray = hist_ref(ch, n)
        acc = math.inf if stray else 0.0
        for i in np.flatnonzero(counts):
            acc = acc + float(int(counts[i])) * icl[i] if icl[i] is not None else math.inf
        out.append(acc)
    return np.array(out, dtype=np.float64)


def zipf_counts(n, s=1.2, total=1 << 16):
    """Zipf(s) over n symbols quantised to `total` with every symbol kept (the oracle's rule)."""
    p = 1.0 / np.arange(1, n + 1, dtype=np.float64) ** s
    counts = np.maximum(1, np.round(p / p.sum() * (1 << 30))).astype(np.uint64)
    c, cum, t = O.quantize_counts(counts, total, O.Q_ALL_SYMBOLS)
    return np.array(c, np.uint32), np.array(cum, np.uint32), t
