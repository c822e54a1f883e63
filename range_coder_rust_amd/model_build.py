"""Model construction on the GPU — the step before encode.

The reference builds its model by counting (FreqTable::new + add_alphabet_freq per symbol,
examples/sample_impl.rs:49-60) and scanning (calc_cum, :61-69); PModel::ideal_code_length
(src/pmodel.rs:14-40) prices one symbol.  Here:

  histogram(syms, sym_off)        rc_histogram: per-chunk and/or batch symbol counts (HIP)
  quantize_counts(counts, T)      rc_quantize_counts: counts -> (c, cum, total) table
  quantize_counts_wide(counts, T) the same for up to 4096 symbols (wide static models)
  build_model(syms, sym_off, T)   histogram -> table -> StaticModel, in one call
  ideal_bits(model, chunk_hist)   rc_ideal_bits: per-chunk sum of ideal code lengths (HIP)
  histogram_order1(syms, sym_off, ctx_map, first_row)   rc_histogram_order1: symbol counts by
                                  context class, the previous symbol picking the class (HIP)
  build_order1_set(syms, sym_off, ctx_map)   those counts -> Order1ModelSet, in one call
  histogram_pairs_periodic(syms, sym_off, P) rc_histogram_pairs_periodic: the pair histogram per
                                  position in a record of P bytes (HIP); lag=D takes the pairs
                                  D symbols apart (rc_histogram_pairs_lagged)
  histogram_pairs(syms, sym_off)  rc_histogram_pairs: the full 256 x 256 pair histogram and the
                                  histogram of the chunks' first symbols (HIP)
  cluster_contexts(pair, first, K)           rc_cluster_contexts: those counts -> a context map
                                  of at most K classes and a first_row (host)
  cluster_contexts_joint(pair, first, K)     rc_cluster_contexts_dev: the same on the device, over
                                  the (phase, context) items of periodic pair counts (HIP)
  fit_order1_set(syms, sym_off, K)           pairs -> map -> class counts -> Order1ModelSet
  ideal_bits_order1(model, syms, sym_off)    rc_ideal_bits_order1: per-chunk ideal bits of an
                                  order-1 set, straight from the symbols (HIP)
  histogram_wide(syms, sym_off, n_bins)      rc_histogram_wide: the counts of 16-bit symbols (HIP)
  build_wide_model(syms, sym_off, n)         those counts -> WideStaticModel, in one call
  histogram16(syms, sym_off)                 the exact 65536-bin histogram of 16-bit symbols (HIP)
  build_wide16_model(syms, sym_off)          those counts -> Wide16StaticModel, in one call
                                             (target_total > 65536: a Wide16FineModel)
  ideal_bits_wide(model, syms, sym_off)      rc_ideal_bits_wide: per-chunk ideal bits of a wide
                                  model, straight from the symbols (HIP)
  cost_table(c, total)            rc_cost_table: a row's integer costs, 2^-16 bit units (host)
  chunk_set_costs(chunk_hist, cost_rows)     rc_chunk_set_costs: every chunk's cost under every
                                  row, and its cheapest row (HIP)
  histogram_by_class(chunk_hist, class_of, K)  rc_histogram_by_class: rc_histogram's rows summed
                                  per class (HIP)
  fit_chunk_set(syms, sym_off, K) histograms -> K classes by cost -> (ChunkModelSet, class_of)
"""
import ctypes

import numpy as np

from . import _native as N
from .api import (ChunkModelSet, Order1ModelSet, StaticModel, Wide16FineModel, Wide16StaticModel, WideStaticModel, _check_dev, _ptr, _sym16, _torch,
                  default_context)


def quantize_counts(counts, target_total=0, all_symbols=False, _entry="rc_quantize_counts"):
    """rc_quantize_counts (host): counts (len n <= 256) -> (c, cum, total).

    target_total 0 keeps calc_cum's exact table; otherwise counts are scaled to that total
    (each modelled symbol keeps c >= 1).  all_symbols gives absent symbols c >= 1 too."""
    L = N.load()
    cnt = np.ascontiguousarray(counts, dtype=np.uint64)
    n = len(cnt)
    c = np.zeros(max(n, 1), np.uint32)
    cum = np.zeros(max(n, 1), np.uint32)
    total = ctypes.c_uint32()
    rc = getattr(L, _entry)(ctypes.c_void_p(cnt.ctypes.data), n, int(target_total),
                            N.Q_ALL_SYMBOLS if all_symbols else 0,
                            ctypes.c_void_p(c.ctypes.data), ctypes.c_void_p(cum.ctypes.data),
                            ctypes.byref(total))
    if rc == N.RC_E_BAD_MODEL:
        raise ValueError("no frequency table for these counts and target")
    N.check(rc, _entry)
    return c[:n], cum[:n], int(total.value)


def quantize_counts_wide(counts, target_total=0, all_symbols=False):
    """rc_quantize_counts_wide (host): quantize_counts for the alphabets of wide static models
    (len n <= 4096)."""
    return quantize_counts(counts, target_total, all_symbols, _entry="rc_quantize_counts_wide")


def quantize_counts_wide16(counts, target_total=0, all_symbols=False):
    """rc_quantize_counts_wide16 (host): quantize_counts for the alphabets of wide16 static models
    (len n <= 65536).  all_symbols with more symbols than a nonzero target_total is a
    ValueError."""
    if all_symbols and target_total and len(counts) > target_total:
        raise ValueError("all_symbols needs target_total >= the number of symbols")
    return quantize_counts(counts, target_total, all_symbols, _entry="rc_quantize_counts_wide16")


def quantize_counts_wide16_fine(counts, target_total=1 << 20, all_symbols=False):
    """rc_quantize_counts_wide16_fine (host): quantize_counts for wide16 fine models (len n <=
    65536, 65536 < target_total <= 2^24; any other target is a ValueError)."""
    if not 65536 < int(target_total) <= N.MAX_WIDE16_FINE_TOTAL:
        raise ValueError("a wide16 fine model's target_total lies in 65537..16777216")
    return quantize_counts(counts, target_total, all_symbols,
                           _entry="rc_quantize_counts_wide16_fine")


def histogram(syms, sym_off, per_chunk=False, batch=True, ctx=None):
    """rc_histogram on torch tensors (async, torch's current stream).

    Returns (hist, chunk_hist): hist int64[256] (the batch) or None, chunk_hist int32[n, 256]
    (one row per chunk) or None."""
    torch = _torch()
    _check_dev(syms, "syms", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    ctx = ctx or default_context(syms.device.index)
    n = sym_off.numel() - 1
    hist = torch.zeros(256, dtype=torch.int64, device=syms.device) if batch else None
    chunk_hist = (torch.empty((max(n, 1), 256), dtype=torch.int32, device=syms.device)
                  if per_chunk else None)
    ctx.bind_stream()
    N.check(ctx._lib.rc_histogram(ctx.handle, _ptr(syms), _ptr(sym_off), n, _ptr(chunk_hist),
                                  _ptr(hist)), "rc_histogram")
    return hist, (chunk_hist[:n] if per_chunk else None)


def build_model(syms, sym_off, target_total=1 << 16, n_symbols=256, all_symbols=True, ctx=None):
    """Histogram of the batch on the GPU, then a StaticModel of its (scaled) table."""
    hist, _ = histogram(syms, sym_off, ctx=ctx)
    counts = hist.cpu().numpy().astype(np.uint64)
    if n_symbols < 256 and counts[n_symbols:].any():
        raise ValueError(f"symbols >= {n_symbols} present")
    c, cum, total = quantize_counts(counts[:n_symbols], target_total, all_symbols)
    return StaticModel(c, cum, total, ctx=ctx or default_context(syms.device.index))


def _ctx_map256(ctx_map):
    cm = np.asarray(ctx_map)
    if cm.ndim != 1 or len(cm) > 256 or len(cm) < 1:
        raise ValueError("ctx_map: 1..256 rows, one per previous symbol")
    if (cm < 0).any() or (cm > 255).any():
        raise ValueError("ctx_map entries are rows of the set")
    m = np.zeros(256, np.uint8)  # (symbols past the map: row 0)
    m[:len(cm)] = cm
    return m


def histogram_order1(syms, sym_off, ctx_map, first_row=0, n_models=None, hist=None, ctx=None):
    """rc_histogram_order1 on torch tensors (async, torch's current stream): int64[K, 256], row j
    = the counts of the symbols whose context row is j (first_row for a chunk's first symbol,
    ctx_map[previous symbol] otherwise).  ctx_map: up to 256 rows (missing entries are row 0);
    K = n_models (default: the largest row named + 1).  hist: counts are added into it."""
    torch = _torch()
    _check_dev(syms, "syms", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    m = _ctx_map256(ctx_map)
    K = int(n_models) if n_models is not None else max(int(m.max()), int(first_row)) + 1
    if not 1 <= K <= N.MAX_SET_MODELS or int(m.max()) >= K or not 0 <= int(first_row) < K:
        raise ValueError(f"ctx_map and first_row must name rows 0..{K - 1} of at most "
                         f"{N.MAX_SET_MODELS}")
    ctx = ctx or default_context(syms.device.index)
    n = sym_off.numel() - 1
    if hist is None:
        hist = torch.zeros((K, 256), dtype=torch.int64, device=syms.device)
    else:
        _check_dev(hist, "hist", (torch.int64, torch.uint64))
        if tuple(hist.shape) != (K, 256):
            raise ValueError(f"hist must be [{K}, 256]")
    ctx.bind_stream()
    N.check(ctx._lib.rc_histogram_order1(ctx.handle, K, ctypes.c_void_p(m.ctypes.data),
                                         int(first_row), _ptr(syms), _ptr(sym_off), n,
                                         _ptr(hist)), "rc_histogram_order1")
    return hist


def _ctx_maps256(ctx_map, period):
    """[period, 256] uint8 from a [period, n] map (symbols past it: row 0)."""
    cm = np.asarray(ctx_map)
    if cm.ndim != 2 or cm.shape[0] != period:
        raise ValueError(f"ctx_map must be [{period}, n]: one map per phase")
    return np.stack([_ctx_map256(r) for r in cm])


def _class_counts(pair, first, maps, first_row, n_models):
    """The counts of the rows of a periodic set from periodic pair counts (host): row j collects
    pair[ph][p] of every (ph, p) with maps[ph][p] == j, and first_row the first symbols (at a
    lag: the first `lag` symbols of every chunk, as histogram_pairs_periodic counts them)."""
    counts = np.zeros((n_models, 256), np.uint64)
    for ph in range(len(pair)):
        np.add.at(counts, maps[ph].astype(np.int64), pair[ph].astype(np.uint64))
    counts[first_row] += first.astype(np.uint64)
    return counts


def build_order1_set(syms, sym_off, ctx_map, first_row=0, target_total=1 << 16, n_symbols=256,
                     n_models=None, ctx=None, period=1, lag=1):
    """Pair counts of the batch on the GPU, then an Order1ModelSet of the rows quantised from
    them (every symbol kept encodable in every row).  period > 1: ctx_map is [period, n] and
    the rows' counts are summed on the host from histogram_pairs_periodic's.  lag > 1: the pairs
    are taken at that distance (a flat map is accepted at period 1), counted the same way."""
    ctx = ctx or default_context(syms.device.index)
    period, lag = int(period), int(lag)
    if period != 1 or lag != 1:
        if period == 1 and np.asarray(ctx_map).ndim == 1:
            ctx_map = np.asarray(ctx_map)[None]
        maps = _ctx_maps256(ctx_map, period)
        K = int(n_models) if n_models is not None else max(int(maps.max()), int(first_row)) + 1
        if not 1 <= K <= N.MAX_SET_MODELS or int(maps.max()) >= K or not 0 <= int(first_row) < K:
            raise ValueError(f"ctx_map and first_row must name rows 0..{K - 1} of at most "
                             f"{N.MAX_SET_MODELS}")
        pair, first = histogram_pairs_periodic(syms, sym_off, period, ctx=ctx, lag=lag)
        counts = _class_counts(pair.cpu().numpy(), first.cpu().numpy(), maps, int(first_row), K)
        if n_symbols < 256 and counts[:, n_symbols:].any():
            raise ValueError(f"symbols >= {n_symbols} present")
        return Order1ModelSet.from_counts(counts[:, :n_symbols], maps[:, :n_symbols], first_row,
                                          target_total, ctx=ctx, period=period, lag=lag)
    hist = histogram_order1(syms, sym_off, ctx_map, first_row, n_models=n_models, ctx=ctx)
    counts = hist.cpu().numpy().astype(np.uint64)
    if n_symbols < 256 and counts[:, n_symbols:].any():
        raise ValueError(f"symbols >= {n_symbols} present")
    return Order1ModelSet.from_counts(counts[:, :n_symbols], _ctx_map256(ctx_map)[:n_symbols],
                                      first_row, target_total, ctx=ctx)


def histogram_pairs(syms, sym_off, pair_hist=None, first_hist=None, ctx=None):
    """rc_histogram_pairs on torch tensors (async, torch's current stream).

    Returns (pair_hist, first_hist): int64[256, 256], [p][s] = the positions i >= 1 of a chunk
    with sym[i-1] = p and sym[i] = s, and int64[256], [s] = the non-empty chunks whose symbol 0
    is s.  Chunk boundaries reset the context.  Given arrays are added into."""
    torch = _torch()
    _check_dev(syms, "syms", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    ctx = ctx or default_context(syms.device.index)
    n = sym_off.numel() - 1
    for name, t, shape in (("pair_hist", pair_hist, (256, 256)), ("first_hist", first_hist, (256,))):
        if t is not None:
            _check_dev(t, name, (torch.int64, torch.uint64))
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}")
    if pair_hist is None:
        pair_hist = torch.zeros((256, 256), dtype=torch.int64, device=syms.device)
    if first_hist is None:
        first_hist = torch.zeros(256, dtype=torch.int64, device=syms.device)
    ctx.bind_stream()
    N.check(ctx._lib.rc_histogram_pairs(ctx.handle, _ptr(syms), _ptr(sym_off), n,
                                        _ptr(pair_hist), _ptr(first_hist)), "rc_histogram_pairs")
    return pair_hist, first_hist


def histogram_pairs_periodic(syms, sym_off, period, pair_hist=None, first_hist=None, ctx=None,
                             lag=1):
    """rc_histogram_pairs_lagged on torch tensors (async, torch's current stream); at lag 1 that
    is rc_histogram_pairs_periodic.

    Returns (pair_hist, first_hist): int64[period, 256, 256], [ph][p][s] = the positions i >= 1
    of a chunk with i % period == ph, sym[i-1] = p and sym[i] = s (i counted from the chunk's
    start), and int64[256] as histogram_pairs gives it.  Chunk boundaries reset the context.
    Given arrays are added into.  period: 1, 2, 4 or 8.

    lag (1, 2, 4 or 8): the pairs are taken at that
    distance, [ph][p][s] = the positions i >= lag with sym[i-lag] = p, and first_hist counts the
    positions i < lag of every chunk, so that the two sum to the number of symbols."""
    torch = _torch()
    _check_dev(syms, "syms", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    period = int(period)
    if period not in (1, 2, 4, 8):
        raise ValueError("period must be 1, 2, 4 or 8")
    lag = int(lag)
    if lag not in (1, 2, 4, 8):
        raise ValueError("lag must be 1, 2, 4 or 8")
    ctx = ctx or default_context(syms.device.index)
    n = sym_off.numel() - 1
    for name, t, shape in (("pair_hist", pair_hist, (period, 256, 256)),
                           ("first_hist", first_hist, (256,))):
        if t is not None:
            _check_dev(t, name, (torch.int64, torch.uint64))
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}")
    if pair_hist is None:
        pair_hist = torch.zeros((period, 256, 256), dtype=torch.int64, device=syms.device)
    if first_hist is None:
        first_hist = torch.zeros(256, dtype=torch.int64, device=syms.device)
    ctx.bind_stream()
    N.check(ctx._lib.rc_histogram_pairs_lagged(ctx.handle, period, lag, _ptr(syms), _ptr(sym_off),
                                               n, _ptr(pair_hist), _ptr(first_hist)),
            "rc_histogram_pairs_lagged")
    return pair_hist, first_hist


def cluster_contexts(pair_hist, first_hist, n_models=64, n_symbols=256):
    """rc_cluster_contexts (host): pair counts [256, 256] and first-symbol counts [256] -> a
    context map of at most n_models classes, by greedy agglomerative clustering under the
    empirical-entropy cost.

    Returns (ctx_map, first_row, n_models, cost_bits): ctx_map uint8[n_symbols], the class of
    every previous symbol; first_row, the class of a chunk's start; the number of classes found
    (fewer than asked for when fewer contexts occur); cost_bits, the ideal bits of the counted
    symbols under the classes' exact rows."""
    L = N.load()
    pair = np.ascontiguousarray(pair_hist, dtype=np.uint64)
    first = np.ascontiguousarray(first_hist, dtype=np.uint64)
    if pair.shape != (256, 256) or first.shape != (256,):
        raise ValueError("pair_hist must be [256, 256] and first_hist [256]")
    cm = np.zeros(256, np.uint8)
    first_row, k, cost = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
    rc = L.rc_cluster_contexts(ctypes.c_void_p(pair.ctypes.data),
                               ctypes.c_void_p(first.ctypes.data), int(n_symbols), int(n_models),
                               ctypes.c_void_p(cm.ctypes.data), ctypes.byref(first_row),
                               ctypes.byref(k), ctypes.byref(cost))
    if rc == N.RC_E_BAD_SYMBOL:
        raise ValueError(f"symbols >= {int(n_symbols)} present")
    if rc == N.RC_E_BAD_MODEL:
        raise ValueError("no context map for empty counts")
    N.check(rc, "rc_cluster_contexts")
    return cm[:int(n_symbols)], int(first_row.value), int(k.value), float(cost.value)


def cluster_contexts_joint(pair_hist, first_hist, n_models=64, n_symbols=256, ctx=None):
    """rc_cluster_contexts_dev: cluster_contexts on the device, jointly over the (phase, context)
    items of periodic pair counts, so that the phases share the n_models rows.

    pair_hist: a device tensor int64/uint64 [P, 256, 256] (P = 1, 2, 4 or 8) as
    histogram_pairs_periodic gives it, or [256, 256] for P = 1; first_hist: [256].  Neither is
    written.  Returns (ctx_map, first_row, n_models, cost_bits) as cluster_contexts does, with
    ctx_map uint8[P, n_symbols] ([n_symbols] for a [256, 256] input).  The call waits for the
    stream."""
    torch = _torch()
    _check_dev(pair_hist, "pair_hist", (torch.int64, torch.uint64))
    _check_dev(first_hist, "first_hist", (torch.int64, torch.uint64))
    flat = pair_hist.dim() == 2
    shape = tuple(pair_hist.shape)
    period = 1 if flat else (shape[0] if len(shape) == 3 else 0)
    if period not in (1, 2, 4, 8) or shape[-2:] != (256, 256) or tuple(first_hist.shape) != (256,):
        raise ValueError("pair_hist must be [P, 256, 256] (P = 1, 2, 4 or 8) or [256, 256], "
                         "and first_hist [256]")
    ctx = ctx or default_context(pair_hist.device.index)
    cm = np.zeros((period, 256), np.uint8)
    first_row, k, cost = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
    ctx.bind_stream()
    rc = ctx._lib.rc_cluster_contexts_dev(ctx.handle, period, _ptr(pair_hist), _ptr(first_hist),
                                          int(n_symbols), int(n_models),
                                          ctypes.c_void_p(cm.ctypes.data), ctypes.byref(first_row),
                                          ctypes.byref(k), ctypes.byref(cost))
    if rc == N.RC_E_BAD_SYMBOL:
        raise ValueError(f"symbols >= {int(n_symbols)} present")
    if rc == N.RC_E_BAD_MODEL:
        raise ValueError("no context map for empty counts")
    N.check(rc, "rc_cluster_contexts_dev")
    cm = cm[:, :int(n_symbols)]
    return (cm[0] if flat else cm), int(first_row.value), int(k.value), float(cost.value)


def fit_order1_set(syms, sym_off, n_models=64, target_total=1 << 16, n_symbols=256, ctx=None,
                   period=1, joint=False, lag=1):
    """An Order1ModelSet fitted to the batch: pair counts on the GPU (histogram_pairs), a context
    map of at most n_models classes from them (cluster_contexts), the classes' counts on the GPU
    (histogram_order1 with the map found) and their quantised rows.  The set's ctx_map and
    first_row are the ones found; it has as many rows as classes were found.

    period > 1 (2, 4 or 8) fits a periodic set: periodic pair counts on the GPU
    (histogram_pairs_periodic), then cluster_contexts once per phase with n_models // period
    classes (phase 0 gets the start-of-chunk counts as its pseudo-context, the others none;
    ValueError if n_models < period), phase ph's rows numbered after those of the phases before
    it, the classes' counts summed on the host from the pair counts (no second pass over the
    symbols) and the rows quantised.  That is `period` runs of the host clustering, about 0.17 s
    each, and without `joint` the phases cannot share a row: every phase gets
    the same number of classes whether it needs them or not.

    joint=True clusters on the device instead (cluster_contexts_joint), on the
    pair counts where they lie: all the (phase, context) items at once, so the n_models rows are
    shared by the phases as the data asks, and n_models < period is allowed.  The classes'
    counts are summed on the host from the pair counts as above.  At period 1 only the
    clustering moves to the device; the rest is as without `joint`.

    lag > 1 (2, 4 or 8) fits a lagged set: the pair counts are taken at that
    distance (histogram_pairs_periodic with the lag), the start-of-chunk item is the first `lag`
    symbols of every chunk, and the clustering, the class counts and the rows are those of a
    periodic fit, whatever the period (period 1 included).  lag=1 is the code above unchanged."""
    period, lag = int(period), int(lag)
    if period not in (1, 2, 4, 8):
        raise ValueError("period must be 1, 2, 4 or 8")
    if lag not in (1, 2, 4, 8):
        raise ValueError("lag must be 1, 2, 4 or 8")
    if int(n_models) < period and not joint:
        raise ValueError(f"n_models = {n_models} leaves a phase of period {period} no row")
    ctx = ctx or default_context(syms.device.index)
    if joint and (period != 1 or lag != 1):
        pair_t, first_t = histogram_pairs_periodic(syms, sym_off, period, ctx=ctx, lag=lag)
        cm, first_row, k, _ = cluster_contexts_joint(pair_t, first_t, n_models, n_symbols, ctx=ctx)
        maps = np.zeros((period, 256), np.uint8)
        maps[:, :cm.shape[1]] = cm
        counts = _class_counts(pair_t.cpu().numpy(), first_t.cpu().numpy(), maps, first_row, k)
        return Order1ModelSet.from_counts(counts[:, :n_symbols], maps[:, :n_symbols], first_row,
                                          target_total, ctx=ctx, period=period, lag=lag)
    if joint:
        pair, first = histogram_pairs(syms, sym_off, ctx=ctx)
        cm, first_row, k, _ = cluster_contexts_joint(pair, first, n_models, n_symbols, ctx=ctx)
        return build_order1_set(syms, sym_off, cm, first_row, target_total, n_symbols, n_models=k,
                                ctx=ctx)
    if period != 1 or lag != 1:
        pair_t, first_t = histogram_pairs_periodic(syms, sym_off, period, ctx=ctx, lag=lag)
        pair, first = pair_t.cpu().numpy(), first_t.cpu().numpy()
        maps = np.zeros((period, 256), np.uint8)
        first_row, rows = 0, 0
        for ph in range(period):
            if ph and not pair[ph].any():
                continue  # (no chunk reaches this phase: its map is never read, row 0 will do)
            cm, fr, k, _ = cluster_contexts(pair[ph], first if ph == 0 else np.zeros(256),
                                            int(n_models) // period, n_symbols)
            maps[ph, :len(cm)] = cm + rows
            if ph == 0:
                first_row = fr
            rows += k
        counts = _class_counts(pair, first, maps, first_row, rows)
        return Order1ModelSet.from_counts(counts[:, :n_symbols], maps[:, :n_symbols], first_row,
                                          target_total, ctx=ctx, period=period, lag=lag)
    pair, first = histogram_pairs(syms, sym_off, ctx=ctx)
    cm, first_row, k, _ = cluster_contexts(pair.cpu().numpy(), first.cpu().numpy(), n_models,
                                           n_symbols)
    return build_order1_set(syms, sym_off, cm, first_row, target_total, n_symbols, n_models=k,
                            ctx=ctx)


def ideal_bits_order1(model, syms, sym_off):
    """rc_ideal_bits_order1: float64[n] tensor, per chunk the sum of log2(total / c[row_i][s_i])
    over its symbols, row_0 = first_row and row_i = ctx_map[s_(i-1)], straight from the symbols
    (inf if a term has c == 0 or a symbol >= model.n_symbols; 0.0 for an empty chunk).  model:
    an Order1ModelSet."""
    torch = _torch()
    _check_dev(syms, "syms", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    n = sym_off.numel() - 1
    bits = torch.empty(max(n, 1), dtype=torch.float64, device=syms.device)
    ctx = model.ctx
    ctx.bind_stream()
    N.check(ctx._lib.rc_ideal_bits_order1(ctx.handle, model.handle, _ptr(syms), _ptr(sym_off), n,
                                          _ptr(bits)), "rc_ideal_bits_order1")
    return bits[:n]


def histogram_wide(syms, sym_off, n_bins, per_chunk=False, batch=True, ctx=None):
    """rc_histogram_wide on torch tensors (async, torch's current stream): histogram for 16-bit
    symbols (uint16, or int16 taken as uint16) over bins 0 .. n_bins - 1, n_bins <= 4096.

    Returns (hist, chunk_hist, oob): hist int64[n_bins] (the batch) or None, chunk_hist
    int32[n, n_bins] (one row per chunk) or None, oob an int64 scalar tensor: the number of
    symbols >= n_bins, which are counted nowhere else."""
    torch = _torch()
    syms = _sym16(syms, "syms")
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    n_bins = int(n_bins)
    if not 1 <= n_bins <= N.MAX_WIDE_SYMBOLS:
        raise ValueError(f"n_bins must be 1..{N.MAX_WIDE_SYMBOLS}")
    ctx = ctx or default_context(syms.device.index)
    n = sym_off.numel() - 1
    hist = torch.zeros(n_bins, dtype=torch.int64, device=syms.device) if batch else None
    chunk_hist = (torch.empty((max(n, 1), n_bins), dtype=torch.int32, device=syms.device)
                  if per_chunk else None)
    oob = torch.zeros((), dtype=torch.int64, device=syms.device)
    ctx.bind_stream()
    N.check(ctx._lib.rc_histogram_wide(ctx.handle, _ptr(syms), _ptr(sym_off), n, n_bins,
                                       _ptr(chunk_hist), _ptr(hist), _ptr(oob)),
            "rc_histogram_wide")
    return hist, (chunk_hist[:n] if per_chunk else None), oob


def build_wide_model(syms, sym_off, n_symbols, target_total=1 << 16, all_symbols=True, ctx=None):
    """Histogram of the batch on the GPU, then a WideStaticModel of its (scaled) table over
    n_symbols symbols.  ValueError if the batch holds a symbol >= n_symbols."""
    ctx = ctx or default_context(syms.device.index)
    hist, _, oob = histogram_wide(syms, sym_off, n_symbols, ctx=ctx)
    stray = int(oob.item())
    if stray:
        raise ValueError(f"{stray} symbols >= {int(n_symbols)} present")
    counts = hist.cpu().numpy().astype(np.uint64)
    c, cum, total = quantize_counts_wide(counts, target_total, all_symbols)
    return WideStaticModel(c, cum, total, ctx=ctx)


def histogram16(syms, sym_off, ctx=None):
    """The exact histogram of 16-bit symbols over all 65536 values: int64[65536] tensor (async,
    torch's current stream).  syms uint16 / int16 on the device, sym_off in symbols.

    No kernel of its own: the pair histogram of period 2 over the symbols' bytes (byte offsets
    2 * sym_off) counts at phase 1 the pairs (low byte, high byte) of one symbol each, and phase 1
    never crosses a chunk start, so on a little-endian host slice [1][lo][hi] is the count of
    symbol hi << 8 | lo."""
    import sys
    torch = _torch()
    _sym16(syms, "syms")
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    if sys.byteorder != "little":
        raise NotImplementedError("histogram16 reads the symbols' bytes in little-endian order")
    pair, _ = histogram_pairs_periodic(syms.view(torch.uint8), sym_off * 2, 2, ctx=ctx)
    return pair[1].t().contiguous().view(-1)


def build_wide16_model(syms, sym_off, n_symbols=None, target_total=1 << 16, ctx=None):
    """histogram16 of the batch, then a Wide16StaticModel of its table scaled to target_total (a
    Wide16FineModel when target_total lies above 65536, up to 2^24) over
    n_symbols symbols (None: the largest symbol that occurs, plus one).  Every symbol that occurs
    gets c >= 1; one that does not may get 0 and is then not encodable.  Raises ValueError when a
    symbol >= n_symbols occurs, when nothing occurs, or when more distinct symbols occur than
    target_total.  Synchronises (the counts are quantized on the host)."""
    counts = histogram16(syms, sym_off, ctx=ctx).cpu().numpy().astype(np.uint64)
    used = np.flatnonzero(counts)
    if used.size == 0:
        raise ValueError("no symbols to model")
    if n_symbols is None:
        n_symbols = int(used[-1]) + 1
    n_symbols = int(n_symbols)
    if not 1 <= n_symbols <= N.MAX_WIDE16_SYMBOLS:
        raise ValueError(f"n_symbols must be 1..{N.MAX_WIDE16_SYMBOLS}")
    if used[-1] >= n_symbols:
        raise ValueError(f"symbol {int(used[-1])} >= n_symbols in the data")
    if target_total and used.size > target_total:
        raise ValueError(f"{used.size} distinct symbols occur: more than target_total")
    if target_total and target_total > 65536:  # a fine model's total
        c, cum, total = quantize_counts_wide16_fine(counts[:n_symbols], target_total,
                                                    all_symbols=False)
        return Wide16FineModel(c, cum, total, ctx=ctx)
    c, cum, total = quantize_counts_wide16(counts[:n_symbols], target_total, all_symbols=False)
    return Wide16StaticModel(c, cum, total, ctx=ctx)


def ideal_bits_wide(model, syms, sym_off):
    """rc_ideal_bits_wide: float64[n] tensor, per chunk the sum of log2(total / c[s]) over its
    16-bit symbols, straight from the symbols (inf if the chunk holds a symbol with c == 0 or
    one >= model.n_symbols; 0.0 for an empty chunk).  model: a WideStaticModel."""
    torch = _torch()
    syms = _sym16(syms, "syms")
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    n = sym_off.numel() - 1
    bits = torch.empty(max(n, 1), dtype=torch.float64, device=syms.device)
    ctx = model.ctx
    ctx.bind_stream()
    N.check(ctx._lib.rc_ideal_bits_wide(ctx.handle, model.handle, _ptr(syms), _ptr(sym_off), n,
                                        _ptr(bits)), "rc_ideal_bits_wide")
    return bits[:n]


def ideal_bits(model, chunk_hist):
    """rc_ideal_bits: float64[n] tensor, per chunk sum of log2(total / c[s]) over its symbols
    (inf if the chunk holds a symbol with c == 0).  model: a StaticModel (its host table)."""
    torch = _torch()
    _check_dev(chunk_hist, "chunk_hist", (torch.int32,))
    n = chunk_hist.shape[0] if chunk_hist.dim() == 2 else 0
    if chunk_hist.dim() != 2 or chunk_hist.shape[1] != 256:
        raise ValueError("chunk_hist must be [n_chunks, 256]")
    bits = torch.empty(max(n, 1), dtype=torch.float64, device=chunk_hist.device)
    ctx = model.ctx
    ctx.bind_stream()
    c = np.ascontiguousarray(model.c, dtype=np.uint32)
    N.check(ctx._lib.rc_ideal_bits(ctx.handle, ctypes.c_void_p(c.ctypes.data), len(c),
                                   model.total, _ptr(chunk_hist), n, _ptr(bits)),
            "rc_ideal_bits")
    return bits[:n]


# ---------------------------------------------------------------------- static chunk sets
def cost_table(c, total):
    """rc_cost_table (host): uint32[len(c)], round(65536 log2(total / c)) per symbol and
    0xFFFFFFFF where c == 0."""
    cc = np.ascontiguousarray(c, dtype=np.uint32)
    out = np.zeros(max(len(cc), 1), np.uint32)
    N.check(N.load().rc_cost_table(ctypes.c_void_p(cc.ctypes.data), len(cc), int(total),
                                   ctypes.c_void_p(out.ctypes.data)), "rc_cost_table")
    return out[:len(cc)]


def chunk_set_costs(chunk_hist, cost_rows, all_costs=False, ctx=None):
    """rc_chunk_set_costs on torch tensors (torch's current stream): chunk_hist int32[n, 256]
    (histogram's per-chunk rows), cost_rows [K, <= 256] uint32 on the host (cost_table's; the
    entries past a row's alphabet count as 0xFFFFFFFF).  Returns (best_row uint8[n], best_cost
    int64[n], costs int64[n, K] or None); a cost of -1 is UINT64_MAX, a chunk the row cannot
    code."""
    torch = _torch()
    _check_dev(chunk_hist, "chunk_hist", (torch.int32,))
    rows = np.atleast_2d(np.asarray(cost_rows, dtype=np.uint32))
    K = rows.shape[0]
    if not 1 <= K <= N.MAX_SET_MODELS or rows.shape[1] > 256 or rows.shape[1] < 1:
        raise ValueError(f"cost_rows must be [1..{N.MAX_SET_MODELS}, 1..256]")
    tab = np.full((K, 256), 0xFFFFFFFF, np.uint32)
    tab[:, :rows.shape[1]] = rows
    if chunk_hist.dim() != 2 or chunk_hist.shape[1] != 256 or not chunk_hist.is_contiguous():
        raise ValueError("chunk_hist must be a contiguous [n, 256]")
    n = chunk_hist.shape[0]
    dev = chunk_hist.device
    ctx = ctx or default_context(dev.index)
    best_row = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    best_cost = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    costs = torch.empty((max(n, 1), K), dtype=torch.int64, device=dev) if all_costs else None
    ctx.bind_stream()
    N.check(ctx._lib.rc_chunk_set_costs(ctx.handle, _ptr(chunk_hist), n,
                                        ctypes.c_void_p(tab.ctypes.data), K, _ptr(best_row),
                                        _ptr(best_cost), _ptr(costs)), "rc_chunk_set_costs")
    return best_row[:n], best_cost[:n], (costs[:n] if all_costs else None)


def histogram_by_class(chunk_hist, class_of, n_models, class_hist=None, ctx=None):
    """rc_histogram_by_class on torch tensors (async, torch's current stream): int64[K, 256], row
    c = the sum of the chunk_hist rows of the chunks with class_of[k] == c (a class id >= K is
    skipped).  class_hist: the sums are added into it."""
    torch = _torch()
    _check_dev(chunk_hist, "chunk_hist", (torch.int32,))
    _check_dev(class_of, "class_of", (torch.uint8,))
    K = int(n_models)
    if not 1 <= K <= N.MAX_SET_MODELS:
        raise ValueError(f"n_models must be 1..{N.MAX_SET_MODELS}")
    if chunk_hist.dim() != 2 or chunk_hist.shape[1] != 256 or not chunk_hist.is_contiguous():
        raise ValueError("chunk_hist must be a contiguous [n, 256]")
    n = chunk_hist.shape[0]
    if class_of.numel() < n:
        raise ValueError("class_of must hold one class per chunk")
    if class_hist is None:
        class_hist = torch.zeros((K, 256), dtype=torch.int64, device=chunk_hist.device)
    else:
        _check_dev(class_hist, "class_hist", (torch.int64, torch.uint64))
        if tuple(class_hist.shape) != (K, 256):
            raise ValueError(f"class_hist must be [{K}, 256]")
    ctx = ctx or default_context(chunk_hist.device.index)
    ctx.bind_stream()
    N.check(ctx._lib.rc_histogram_by_class(ctx.handle, _ptr(chunk_hist), _ptr(class_of), n, K,
                                           _ptr(class_hist)), "rc_histogram_by_class")
    return class_hist


def fit_chunk_set(syms, sym_off, n_models=8, target_total=1 << 16, iters=8, ctx=None):
    """A ChunkModelSet of at most n_models rows fitted to the batch, and the chunks' classes
    (uint8[n] device tensor): the rule of tests/chunk_fit_ref.py.  Row 0 starts
    as the pooled table; the dearest chunk under its best row seeds each further row; then at most
    `iters` rounds of reassigning the chunks and re-estimating the rows, until the assignment
    repeats.  Rows that end without a member are dropped.  The histogram, the costs, the sums by
    class (all HIP) and rc_quantize_counts do the work; torch is glue."""
    torch = _torch()
    K = int(n_models)
    if not 1 <= K <= N.MAX_SET_MODELS:
        raise ValueError(f"n_models must be 1..{N.MAX_SET_MODELS}")
    ctx = ctx or default_context(syms.device.index)
    hist, ch = histogram(syms, sym_off, per_chunk=True, ctx=ctx)
    n = ch.shape[0]

    def quant(counts):
        return quantize_counts(np.asarray(counts, dtype=np.uint64), target_total, True)[0]

    rows = [quant(hist.cpu().numpy())]

    def assign():
        best, cost, _ = chunk_set_costs(ch, [cost_table(r, target_total) for r in rows], ctx=ctx)
        return best, cost

    def reestimate(cls):
        sums = histogram_by_class(ch, cls, len(rows), ctx=ctx).cpu().numpy()
        for r in range(len(rows)):
            if sums[r].any():
                rows[r] = quant(sums[r])

    cls = torch.zeros(max(n, 1), dtype=torch.uint8, device=syms.device)[:n]
    while len(rows) < K and n:
        cls, cost = assign()
        top = cost.max()
        if int(top) == 0:
            break
        seed = int(torch.nonzero(cost == top)[0])  # (the lowest chunk id among the dearest)
        rows.append(quant(ch[seed].cpu().numpy()))
        cls, _ = assign()
        reestimate(cls)
    for _ in range(int(iters)):
        new, _ = assign()
        same = torch.equal(new, cls)
        cls = new
        if same:
            break
        reestimate(cls)
    if n:
        cls, _ = assign()
    members = torch.bincount(cls.to(torch.int64), minlength=len(rows)).cpu().numpy()
    used = [r for r in range(len(rows)) if members[r]] or [0]
    remap = np.zeros(len(rows), np.uint8)
    remap[used] = np.arange(len(used), dtype=np.uint8)
    cls = torch.from_numpy(remap).to(syms.device)[cls.to(torch.int64)]
    c = np.stack([rows[r] for r in used])
    return ChunkModelSet(c, None, int(target_total), ctx=ctx), cls
