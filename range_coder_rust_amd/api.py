"""Host-side API of the MI355X range coder, mirroring the reference crate's public surface.

Reference surface (diegodox/range_coder_rust, src/lib.rs:1-13) and what replaces it here:

  trait PModel (src/pmodel.rs:4-41)        -> class PModel (same method names/meaning)
  FreqTable example model (sample_impl.rs)  -> class FreqTable
  Encoder::{new, encode, finish, peek_code} -> class Encoder: encode() reads the model at the
    (src/encoder.rs:14-46)                     call and stages the triple; the resumable stream
                                               kernel codes staged symbols when a result is needed
  Decoder::{new, decode, range_coder, data} -> class Decoder(code): decode() reads the model at
    (src/decoder.rs:14-54)                     the call; symbols are decoded ahead on the GPU while
                                               the table is unchanged; a PModel with its own
                                               find_index is called per symbol (see Decoder)
  error::RangeCoderError (src/error.rs)     -> RangeCoderError and subclasses (raised where
                                               the reference panics or never terminates), with
                                               LowerBoundOverflow / UpperBoundOverflow payloads

The hot path proper is the batch API (encode_batch / decode_batch / encode_chunks /
decode_chunks): many independent chunks per launch, one chunk per GPU lane, through the C ABI
of librc_amd.so (include/range_coder.h).  Tensors are torch CUDA(HIP) tensors; PyTorch is
used only for device memory and streams.  There is no CPU fallback.
"""
import ctypes
import struct
import math

import numpy as np

from . import _native as N

M64 = (1 << 64) - 1

__all__ = [
    "Context", "StaticModel", "PModel", "FreqTable", "Encoder", "Decoder", "RangeCoderError",
    "ZeroFrequencyError", "BadSymbolError", "TruncatedStreamError", "CorruptStreamError",
    "CapacityError", "ChunkTooLongError", "BadModelError", "FinishedError", "RangeCoder",
    "LowerBoundOverflow", "UpperBoundOverflow",
    "ByteCount", "encode_host_multi", "decode_host_multi", "stream_states", "stream_encode_batch", "stream_decode_batch", "encode_batch", "decode_batch", "encode_chunks", "decode_chunks",
    "default_context", "flag_names", "slot_capacity",
    "StaticModelSet", "encode_batch_indexed", "decode_batch_indexed", "encode_chunks_indexed",
    "decode_chunks_indexed",
    "Order1ModelSet", "encode_batch_order1", "decode_batch_order1", "encode_chunks_order1",
    "decode_chunks_order1",
    "RowTable", "stream_decode_rows_batch", "stream_encode_rows_batch", "encode_chunks_rows",
    "decode_chunks_rows",
]


# ----------------------------------------------------------------------------- errors
class RangeCoderError(Exception):
    """src/error.rs:3-13 analogue; raised where the reference returns Err / panics."""


class ZeroFrequencyError(RangeCoderError):
    """Encoding a c_freq == 0 symbol (the reference never terminates: range_coder.rs:83-85)."""


class BadSymbolError(RangeCoderError):
    """Symbol index >= alphabet size (the reference panics: sample_impl.rs:19)."""


class TruncatedStreamError(RangeCoderError):
    """Decoder ran out of code bytes (the reference panics: decoder.rs:33)."""


class CorruptStreamError(RangeCoderError):
    """Decoder selected a zero-frequency symbol (the reference never terminates)."""


class CapacityError(RangeCoderError):
    """An encoded chunk did not fit its output slot."""


class BadModelError(RangeCoderError):
    """A (c_freq, cum_freq, total_freq) on which the reference panics: total 0 (division by
    zero, range_coder.rs:38-40), LowerBoundOverflow (:68-81) or UpperBoundOverflow
    (upper_bound().unwrap(), :138-146)."""


class LowerBoundOverflow(BadModelError):
    """RangeCoderError::LowerBoundOverflow (error.rs:5-10): lower_bound + add_val overflowed in
    param_update (range_coder.rs:68-81).  range is the narrowed range, as the reference reports
    it (self.range was updated first, :65)."""

    def __init__(self, msg, lower_bound, add_val, range_):
        super().__init__(msg)
        self.lower_bound, self.add_val, self.range = lower_bound, add_val, range_


class UpperBoundOverflow(BadModelError):
    """RangeCoderError::UpperBoundOverflow (error.rs:11): lower_bound + range overflowed in
    upper_bound() (range_coder.rs:138-146), which no_carry_expansion unwraps (a panic)."""

    def __init__(self, msg, lower_bound, range_):
        super().__init__(msg)
        self.lower_bound, self.range = lower_bound, range_


class FinishedError(RangeCoderError):
    """encode() after finish(): Encoder::finish takes the encoder by value (encoder.rs:40)."""


class ChunkTooLongError(RangeCoderError):
    """A batch chunk of more than RC_MAX_CHUNK_SYMBOLS (2^25) symbols (32-bit in-chunk stream
    positions; the stream API -- Encoder / Decoder -- has no such limit)."""


_FLAG_ERRORS = [
    (N.F_ZERO_FREQ, ZeroFrequencyError), (N.F_BAD_SYMBOL, BadSymbolError),
    (N.F_CAPACITY, CapacityError), (N.F_TRUNCATED, TruncatedStreamError),
    (N.F_CORRUPT, CorruptStreamError), (N.F_TOO_LONG, ChunkTooLongError),
    (N.F_BAD_MODEL, BadModelError), (N.F_FINISHED, FinishedError),
]


def flag_names(f):
    names = {N.F_ZERO_FREQ: "ZERO_FREQ", N.F_BAD_SYMBOL: "BAD_SYMBOL", N.F_CAPACITY: "CAPACITY",
             N.F_TRUNCATED: "TRUNCATED", N.F_CORRUPT: "CORRUPT", N.F_TOO_LONG: "TOO_LONG",
             N.F_BAD_MODEL: "BAD_MODEL", N.F_FINISHED: "FINISHED"}
    return [v for k, v in names.items() if f & k]


def _raise_for_flag(f, where):
    for bit, exc in _FLAG_ERRORS:
        if f & bit:
            raise exc(f"{where}: {'|'.join(flag_names(f))}")


def _raise_bad_model(low, range_, c, cum, total, where):
    """The reference's error for a flagged (RC_F_BAD_MODEL) symbol, with its payload.  The stream
    kernels stop before the failing symbol, so (low, range) is the state param_update started
    from; the payload is param_update's own arithmetic (range_coder.rs:53-81, :138-146), u64
    products wrapping as in a release build."""
    if total == 0:
        raise BadModelError(f"{where}: range_par_total: attempt to divide by zero")
    r = range_ // total
    nr = (r * c) & M64
    add = (r * cum) & M64
    if low + add > M64:
        raise LowerBoundOverflow(
            f"{where}: Overflow happend while lower_bound uppdating {low} + {add} , {nr}",
            low, add, nr)
    nl = low + add
    if nl + nr > M64:
        raise UpperBoundOverflow(
            f"{where}: Overflow happend when calc upper_bound {nl} + {nr}", nl, nr)
    raise BadModelError(f"{where}: BAD_MODEL")


# ----------------------------------------------------------------------------- torch glue
def _torch():
    import torch
    return torch


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _check_dev(t, name, dtype=None):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TypeError(f"{name} must be a torch tensor on a HIP device")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype not in dtype:
        raise TypeError(f"{name}: dtype {t.dtype} not in {dtype}")


class Context:
    """rc_ctx: one device, launches on the current torch stream of that device."""

    def __init__(self, device=0):
        self._lib = N.load()
        torch = _torch()
        if not torch.cuda.is_available():
            raise N.RCError(N.RC_E_NO_DEVICE, "rc_ctx_create")
        self.device = int(device)
        h = ctypes.c_void_p()
        N.check(self._lib.rc_ctx_create(self.device, ctypes.byref(h)), "rc_ctx_create")
        self.handle = h

    def bind_stream(self):
        """Point the context at torch's current stream for this device (stream-ordered)."""
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        N.check(self._lib.rc_ctx_set_stream(self.handle, ctypes.c_void_p(s)), "rc_ctx_set_stream")

    def synchronize(self):
        N.check(self._lib.rc_ctx_synchronize(self.handle), "rc_ctx_synchronize")

    def info(self):
        buf = ctypes.create_string_buffer(256)
        N.check(self._lib.rc_device_info(self.device, buf, 256), "rc_device_info")
        return buf.value.decode()

    def close(self):
        if getattr(self, "handle", None):
            self._lib.rc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=None):
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device()
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


# ----------------------------------------------------------------------------- models
class PModel:
    """trait PModel (src/pmodel.rs:4-41)."""

    def c_freq(self, index):  # pmodel.rs:6
        raise NotImplementedError

    def cum_freq(self, index):  # pmodel.rs:8
        raise NotImplementedError

    def total_freq(self):  # pmodel.rs:10
        raise NotImplementedError

    def find_index(self, decoder):  # pmodel.rs:12
        """Not overridden: the decoder runs FreqTable::find_index (sample_impl.rs:27-45) itself,
        on the GPU.  Override it to decode with your own rule: Decoder.decode then calls it at
        every symbol with the decoder (range_coder() / data()), as decoder.rs:40 does, and
        applies param_update to the index it returns.  A subclass that overrides it but keeps
        FreqTable's binary-search semantics can set canonical_find_index = True to keep the
        decode-ahead path."""
        raise NotImplementedError

    def ideal_code_length(self, index):  # pmodel.rs:14-40
        p = float(self.c_freq(index))
        if p == 0.0:
            raise RangeCoderError("code length is undefind when probability is zero")
        if math.isnan(p) or math.isinf(p):
            raise RangeCoderError(
                f"code length is undefind when probability is nan or infinite as {p!r}")
        if p < 0:
            raise RangeCoderError(f"code length is undefind when probability is negative as {p}")
        return (math.log(float(self.total_freq())) - math.log(p)) / math.log(2.0)

    def alphabet_count(self):
        """Alphabet size.  Not a trait method in the reference (FreqTable::alphabet_count,
        sample_impl.rs:55-57); the GPU snapshot needs it."""
        raise NotImplementedError


class FreqTable(PModel):
    """The static frequency table of examples/sample_impl.rs:4-70."""

    def __init__(self, alphabet_count):  # FreqTable::new, :49-54
        self.total = 0
        self.c = [0] * int(alphabet_count)
        self.cum = [0] * int(alphabet_count)

    @classmethod
    def from_counts(cls, counts):
        t = cls(len(counts))
        t.c = [int(x) for x in counts]
        t.calc_cum()
        return t

    def alphabet_count(self):  # :55-57
        return len(self.c)

    def add_alphabet_freq(self, index):  # :58-60
        self.c[index] += 1

    def calc_cum(self):  # :61-69
        t = 0
        for i, ci in enumerate(self.c):
            self.cum[i] = t
            t += ci
        self.total = t

    def c_freq(self, index):  # :18-20
        if not 0 <= index < len(self.c):
            raise BadSymbolError(f"index {index} out of alphabet ({len(self.c)})")
        return self.c[index]

    def cum_freq(self, index):  # :21-23
        if not 0 <= index < len(self.cum):
            raise BadSymbolError(f"index {index} out of alphabet ({len(self.cum)})")
        return self.cum[index]

    def total_freq(self):  # :24-26
        return self.total

    def find_index(self, decoder):  # :27-45 — evaluated by the GPU decoders themselves
        raise NotImplementedError("FreqTable.find_index runs inside the GPU decode kernel")

    def _rc_table(self):
        """(c, cum, total) as read through c_freq / cum_freq / total_freq (fast path)."""
        return tuple(self.c), tuple(self.cum), self.total


class StaticModel:
    """rc_model: device snapshot of a PModel's (c_freq, cum_freq, total_freq) table."""

    def __init__(self, c_freq, cum_freq=None, total_freq=None, ctx=None):
        self.ctx = ctx or default_context()
        c = np.ascontiguousarray(c_freq, dtype=np.uint32)
        if cum_freq is None:
            cum = np.concatenate([[0], np.cumsum(c, dtype=np.uint64)[:-1]]).astype(np.uint32)
        else:
            cum = np.ascontiguousarray(cum_freq, dtype=np.uint32)
        if total_freq is None:
            total_freq = int(np.sum(c, dtype=np.uint64))
        if len(c) != len(cum):
            raise ValueError("c_freq and cum_freq differ in length")
        self.c = c
        self.cum = cum
        self.total = int(total_freq)
        self.n_symbols = len(c)
        h = ctypes.c_void_p()
        rc = self.ctx._lib.rc_model_create_static(
            self.ctx.handle, self.n_symbols, ctypes.c_void_p(c.ctypes.data),
            ctypes.c_void_p(cum.ctypes.data), ctypes.c_uint32(self.total & 0xFFFFFFFF),
            ctypes.byref(h))
        if rc == N.RC_E_BAD_MODEL:
            raise ValueError("frequency table rejected: need 1..256 symbols, cum[0] == 0, "
                             "cum[i+1] == cum[i] + c[i], total == sum(c) < 2^32")
        N.check(rc, "rc_model_create_static")
        self.handle = h

    @classmethod
    def from_pmodel(cls, pmodel, n_symbols=None, ctx=None):
        """Snapshot any PModel via c_freq/cum_freq/total_freq (pmodel.rs:6-10)."""
        n = pmodel.alphabet_count() if n_symbols is None else int(n_symbols)
        c = [pmodel.c_freq(i) for i in range(n)]
        cum = [pmodel.cum_freq(i) for i in range(n)]
        return cls(c, cum, pmodel.total_freq(), ctx=ctx)

    def max_bits_per_symbol(self):
        nz = self.c[self.c > 0]
        return math.log2(self.total / float(nz.min()))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx._lib.rc_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# config C4's adaptive model parameters (include/range_coder.h, rc_model_create_adaptive)
ADAPTIVE_DEFAULTS = dict(increment=32, limit=57343, period=256)


class AdaptiveModel:
    """rc_model of the build-defined adaptive order-0 model: per chunk,
    c[i] = 1 initially; after the i-th coded symbol s, c[s] += increment and, every period-th
    symbol, all counts are halved (rounding up) if the total exceeds limit.  Each chunk starts
    from the initial counts, on the GPU as in the oracle (orc_encode_adaptive)."""

    def __init__(self, n_symbols=256, increment=32, limit=57343, period=256, ctx=None):
        self.ctx = ctx or default_context()
        self.n_symbols, self.increment = int(n_symbols), int(increment)
        self.limit, self.period = int(limit), int(period)
        h = ctypes.c_void_p()
        rc = self.ctx._lib.rc_model_create_adaptive(self.ctx.handle, self.n_symbols,
                                                    self.increment, self.limit, self.period,
                                                    ctypes.byref(h))
        if rc == N.RC_E_BAD_MODEL:
            raise ValueError("adaptive model rejected: need 1..256 symbols, increment >= 1, "
                             "period a power of two, n + increment*period <= limit <= "
                             "65535 - increment*period")
        N.check(rc, "rc_model_create_adaptive")
        self.handle = h

    def max_bits_per_symbol(self):
        # the rarest symbol has c >= 1 of a total < 2^16
        return 16.0

    close = StaticModel.close
    __del__ = StaticModel.__del__


class StaticModelSet:
    """rc_model_create_static_set: K static tables (rows) over one alphabet and one total_freq,
    for the indexed batch calls, which take one row index per symbol (the reference's
    encode(&models[idx[i]], sym[i]) / decode(&models[idx[i]])).

    c_rows / cum_rows: K x n_symbols.  The rows are validated on the host at construction
    (ValueError); the device snapshot is made on first use, so a set can be built and inspected
    without a device."""

    def __init__(self, c_rows, cum_rows=None, total_freq=None, ctx=None):
        c = np.ascontiguousarray(c_rows, dtype=np.uint32)
        if c.ndim != 2:
            raise ValueError("c_rows must be K x n_symbols")
        if cum_rows is None:
            cum = np.zeros_like(c)
            if c.shape[1] > 1:
                cum[:, 1:] = np.cumsum(c.astype(np.uint64), axis=1)[:, :-1].astype(np.uint32)
        else:
            cum = np.ascontiguousarray(cum_rows, dtype=np.uint32)
        if cum.shape != c.shape:
            raise ValueError("c_rows and cum_rows differ in shape")
        if total_freq is None:
            total_freq = int(np.sum(c[0], dtype=np.uint64)) if c.size else 0
        self.c, self.cum, self.total = c, cum, int(total_freq)
        self.n_models, self.n_symbols = int(c.shape[0]), int(c.shape[1])
        self._ctx = ctx
        self._handle = None
        rc = N.load().rc_model_set_check_(self.n_models, self.n_symbols,
                                          ctypes.c_void_p(c.ctypes.data),
                                          ctypes.c_void_p(cum.ctypes.data),
                                          ctypes.c_uint32(self.total & 0xFFFFFFFF))
        if rc != N.RC_OK or self.total > 0xFFFFFFFF:
            raise ValueError(
                f"model set rejected: need 1..{N.MAX_SET_MODELS} rows of 1..256 symbols, one "
                "total_freq in 256..65536, and in every row cum[0] == 0, cum[i+1] == cum[i] + "
                "c[i], sum(c) == total_freq")

    @classmethod
    def from_counts(cls, count_rows, target_total=65536, ctx=None):
        """One row per histogram, each scaled to target_total with every symbol kept
        encodable (rc_quantize_counts with RC_Q_ALL_SYMBOLS)."""
        from .model_build import quantize_counts
        rows = [quantize_counts(r, target_total, all_symbols=True) for r in count_rows]
        return cls([r[0] for r in rows], [r[1] for r in rows], int(target_total), ctx=ctx)

    @classmethod
    def from_pmodels(cls, pmodels, n_symbols=None, ctx=None):
        """Snapshot PModels (pmodel.rs:6-10) of one alphabet and one total_freq."""
        pmodels = list(pmodels)
        if not pmodels:
            raise ValueError("no models")
        n = pmodels[0].alphabet_count() if n_symbols is None else int(n_symbols)
        c = [[p.c_freq(i) for i in range(n)] for p in pmodels]
        cum = [[p.cum_freq(i) for i in range(n)] for p in pmodels]
        totals = {int(p.total_freq()) for p in pmodels}
        if len(totals) != 1:
            raise ValueError(f"the models of a set share one total_freq, got {sorted(totals)}")
        return cls(c, cum, totals.pop(), ctx=ctx)

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    @property
    def handle(self):
        if self._handle is None:
            h = ctypes.c_void_p()
            N.check(self.ctx._lib.rc_model_create_static_set(
                self.ctx.handle, self.n_models, self.n_symbols,
                ctypes.c_void_p(self.c.ctypes.data), ctypes.c_void_p(self.cum.ctypes.data),
                ctypes.c_uint32(self.total), ctypes.byref(h)), "rc_model_create_static_set")
            self._handle = h
        return self._handle

    def max_bits_per_symbol(self):
        nz = self.c[self.c > 0]
        return math.log2(self.total / float(nz.min()))

    def close(self):
        if getattr(self, "_handle", None):
            self._ctx._lib.rc_model_destroy(self._handle)
            self._handle = None

    __del__ = StaticModel.__del__


class ChunkModelSet(StaticModelSet):
    """rc_model_create_chunk_set: K static tables (rows) over one alphabet and one total_freq,
    for the chunk-set batch calls, which take one row per CHUNK: chunk k is coded exactly as
    encode_batch / decode_batch code it with StaticModel(row class_of[k]).

    Construction, the checks (rc_chunk_set_check_: the static set's rules) and the attributes c,
    cum, total, n_models, n_symbols and max_bits_per_symbol() are StaticModelSet's; the device
    snapshot is another (per row what a StaticModel builds), so the two kinds do not mix."""

    @property
    def handle(self):
        if self._handle is None:
            h = ctypes.c_void_p()
            N.check(self.ctx._lib.rc_model_create_chunk_set(
                self.ctx.handle, self.n_models, self.n_symbols,
                ctypes.c_void_p(self.c.ctypes.data), ctypes.c_void_p(self.cum.ctypes.data),
                ctypes.c_uint32(self.total), ctypes.byref(h)), "rc_model_create_chunk_set")
            self._handle = h
        return self._handle


class Order1ModelSet:
    """rc_model_create_order1_set: the K rows of a StaticModelSet plus a context map, for the
    order-1 batch calls, in which the previous symbol of the chunk picks the row: symbol 0 of
    every chunk is coded with row first_row, symbol i > 0 with row ctx_map[sym[i-1]] (the
    reference's encode(&models[row_i], sym[i]) / decode(&models[row_i])).

    c_rows / cum_rows: K x n_symbols; ctx_map: at least n_symbols entries, each < K.  Rows, map
    and first_row are validated on the host at construction (ValueError); the device snapshot is
    made on first use, so a set can be built and inspected without a device.

    period (1, 2, 4 or 8; rc_model_create_order1_set_periodic): the position in a record joins
    the context.  ctx_map is then [period, n_symbols] and symbol i > 0 is coded with row
    ctx_map[i % period, sym[i-1]], i counted from the chunk's start (for period 1 a flat map is
    still accepted).  The order-1 batch calls and ideal_bits_order1 take such a set as they are;
    a container cannot frame a period, so pack() and compress() raise for period > 1.

    lag (1, 2, 4 or 8; rc_model_create_order1_set_lagged): the context is the symbol `lag`
    positions back, the same byte of the record before when lag is the record's size.  Symbol
    i >= lag is coded with row ctx_map[i % period, sym[i-lag]] and every symbol i < lag with
    first_row.  Period and lag are independent; lag 1 is the set without one.  A container
    cannot frame a lag either."""

    def __init__(self, c_rows, cum_rows=None, total_freq=None, ctx_map=None, first_row=0,
                 ctx=None, period=1, lag=1):
        c = np.ascontiguousarray(c_rows, dtype=np.uint32)
        if c.ndim != 2:
            raise ValueError("c_rows must be K x n_symbols")
        if cum_rows is None:
            cum = np.zeros_like(c)
            if c.shape[1] > 1:
                cum[:, 1:] = np.cumsum(c.astype(np.uint64), axis=1)[:, :-1].astype(np.uint32)
        else:
            cum = np.ascontiguousarray(cum_rows, dtype=np.uint32)
        if cum.shape != c.shape:
            raise ValueError("c_rows and cum_rows differ in shape")
        if total_freq is None:
            total_freq = int(np.sum(c[0], dtype=np.uint64)) if c.size else 0
        if ctx_map is None:
            raise ValueError("ctx_map is required: one row per previous symbol")
        cm = np.asarray(ctx_map)
        self.n_models, self.n_symbols = int(c.shape[0]), int(c.shape[1])
        period = int(period)
        if period not in (1, 2, 4, 8):
            raise ValueError("period must be 1, 2, 4 or 8")
        lag = int(lag)
        if lag not in (1, 2, 4, 8):
            raise ValueError("lag must be 1, 2, 4 or 8")
        if cm.ndim == 2 and cm.shape[0] == period and cm.shape[1] >= self.n_symbols:
            cm = cm[:, :self.n_symbols].astype(np.int64)
            if period == 1:
                cm = cm[0]
        elif period == 1 and cm.ndim == 1 and len(cm) >= self.n_symbols:
            cm = cm[:self.n_symbols].astype(np.int64)
        elif period == 1:
            raise ValueError(f"ctx_map needs {self.n_symbols} entries, one per symbol")
        else:
            raise ValueError(f"ctx_map must be [{period}, {self.n_symbols}]: one map per phase")
        first_row = int(first_row)
        if ((cm < 0) | (cm >= self.n_models)).any() or not 0 <= first_row < max(self.n_models, 1):
            raise ValueError(f"ctx_map entries and first_row must be rows of the set "
                             f"(0..{self.n_models - 1})")
        self.c, self.cum, self.total = c, cum, int(total_freq)
        self.ctx_map = np.ascontiguousarray(cm, dtype=np.uint8)
        self.first_row = first_row
        self.period = period
        self.lag = lag
        self._ctx = ctx
        self._handle = None
        tables = (self.n_models, self.n_symbols, ctypes.c_void_p(c.ctypes.data),
                  ctypes.c_void_p(cum.ctypes.data), ctypes.c_uint32(self.total & 0xFFFFFFFF))
        rc = N.load().rc_model_order1_check_lagged_(
            *tables, ctypes.c_uint32(period), ctypes.c_uint32(lag),
            ctypes.c_void_p(self.ctx_map.ctypes.data), ctypes.c_uint32(self.first_row))
        if rc != N.RC_OK or self.total > 0xFFFFFFFF:
            raise ValueError(
                f"order-1 set rejected: need 1..{N.MAX_SET_MODELS} rows of 1..256 symbols, one "
                "total_freq in 256..65536, in every row cum[0] == 0, cum[i+1] == cum[i] + c[i], "
                "sum(c) == total_freq, and a ctx_map and first_row that name rows of the set")

    @classmethod
    def from_counts(cls, count_rows, ctx_map, first_row=0, target_total=65536, ctx=None,
                    period=1, lag=1):
        """One row per context class from its histogram (rc_histogram_order1's rows), each scaled
        to target_total with every symbol kept encodable (rc_quantize_counts with
        RC_Q_ALL_SYMBOLS)."""
        from .model_build import quantize_counts
        rows = [quantize_counts(r, target_total, all_symbols=True) for r in count_rows]
        return cls([r[0] for r in rows], [r[1] for r in rows], int(target_total),
                   ctx_map=ctx_map, first_row=first_row, ctx=ctx, period=period, lag=lag)

    def derive_indexes(self, syms):
        """The index stream the indexed calls would take for one chunk of symbols (host)."""
        s = _u8_chunk(syms)
        idx = np.empty(len(s), np.uint8)
        if len(s):
            m = np.zeros((self.period, 256), np.uint8)
            m[:, :self.n_symbols] = self.ctx_map.reshape(self.period, self.n_symbols)
            D = self.lag
            idx[:D] = self.first_row
            idx[D:] = m[np.arange(D, len(s)) % self.period, s[:-D]]
        return idx

    ctx = StaticModelSet.ctx

    @property
    def handle(self):
        if self._handle is None:
            h = ctypes.c_void_p()
            N.check(self.ctx._lib.rc_model_create_order1_set_lagged(
                self.ctx.handle, self.n_models, self.n_symbols,
                ctypes.c_void_p(self.c.ctypes.data), ctypes.c_void_p(self.cum.ctypes.data),
                ctypes.c_uint32(self.total), ctypes.c_uint32(self.period),
                ctypes.c_uint32(self.lag), ctypes.c_void_p(self.ctx_map.ctypes.data),
                ctypes.c_uint32(self.first_row), ctypes.byref(h)),
                "rc_model_create_order1_set_lagged")
            self._handle = h
        return self._handle

    max_bits_per_symbol = StaticModelSet.max_bits_per_symbol
    close = StaticModelSet.close
    __del__ = StaticModel.__del__


class WideStaticModel:
    """rc_model_create_static_wide: one static table over an alphabet of up to 4096 16-bit
    symbols (the reference's PModel is indexed with usize), for the wide batch calls, which code
    uint16 symbols exactly as encode(&table, sym[i]) / decode(&table).

    The table is validated on the host at construction (ValueError); the device snapshot is made
    on first use, so a model can be built and inspected without a device."""
    # (the native calls and the cap, which Wide16StaticModel replaces)
    _CHECK = "rc_model_wide_check_"
    _CREATE = "rc_model_create_static_wide"
    _MAX = N.MAX_WIDE_SYMBOLS
    _WHAT = "wide"
    _TOTALS = "256..65536"

    def __init__(self, c_freq, cum_freq=None, total_freq=None, ctx=None):
        c = np.ascontiguousarray(c_freq, dtype=np.uint32)
        if c.ndim != 1:
            raise ValueError("c_freq must be one-dimensional")
        if cum_freq is None:
            cum = np.zeros_like(c)
            if len(c) > 1:
                cum[1:] = np.cumsum(c, dtype=np.uint64)[:-1].astype(np.uint32)
        else:
            cum = np.ascontiguousarray(cum_freq, dtype=np.uint32)
        if cum.shape != c.shape:
            raise ValueError("c_freq and cum_freq differ in length")
        if total_freq is None:
            total_freq = int(np.sum(c, dtype=np.uint64))
        self.c, self.cum, self.total = c, cum, int(total_freq)
        self.n_symbols = len(c)
        self._ctx = ctx
        self._handle = None
        rc = getattr(N.load(), self._CHECK)(self.n_symbols, ctypes.c_void_p(c.ctypes.data),
                                            ctypes.c_void_p(cum.ctypes.data),
                                            ctypes.c_uint32(self.total & 0xFFFFFFFF))
        if rc != N.RC_OK or self.total > 0xFFFFFFFF:
            raise ValueError(
                f"{self._WHAT} model rejected: need 1..{self._MAX} symbols, total_freq in "
                f"{self._TOTALS}, cum[0] == 0, cum[i+1] == cum[i] + c[i], sum(c) == total_freq")

    @classmethod
    def from_counts(cls, counts, target_total=65536, ctx=None):
        """A histogram scaled to target_total with every symbol kept encodable
        (rc_quantize_counts_wide with RC_Q_ALL_SYMBOLS)."""
        from .model_build import quantize_counts_wide
        c, cum, total = quantize_counts_wide(counts, target_total, all_symbols=True)
        return cls(c, cum, total, ctx=ctx)

    @classmethod
    def from_pmodel(cls, pmodel, n_symbols=None, ctx=None):
        """Snapshot any PModel via c_freq/cum_freq/total_freq (pmodel.rs:6-10)."""
        n = pmodel.alphabet_count() if n_symbols is None else int(n_symbols)
        c = [pmodel.c_freq(i) for i in range(n)]
        cum = [pmodel.cum_freq(i) for i in range(n)]
        return cls(c, cum, pmodel.total_freq(), ctx=ctx)

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    @property
    def handle(self):
        if self._handle is None:
            h = ctypes.c_void_p()
            N.check(getattr(self.ctx._lib, self._CREATE)(
                self.ctx.handle, self.n_symbols, ctypes.c_void_p(self.c.ctypes.data),
                ctypes.c_void_p(self.cum.ctypes.data), ctypes.c_uint32(self.total),
                ctypes.byref(h)), self._CREATE)
            self._handle = h
        return self._handle

    def max_bits_per_symbol(self):
        nz = self.c[self.c > 0]
        return math.log2(self.total / float(nz.min()))

    close = StaticModelSet.close
    __del__ = StaticModel.__del__


class Wide16StaticModel(WideStaticModel):
    """rc_model_create_static_wide16: one static table over an alphabet of up to 65536 16-bit
    symbols, its tables in device memory, for the wide16 batch calls, which code uint16 symbols
    exactly as encode(&table, sym[i]) / decode(&table).  For a table a WideStaticModel accepts
    too, both give the same bytes; the two kinds do not mix: every call but the wide16 ones
    refuses this model (RC_E_ARG from the library), and the wide16 calls refuse every other.

    The table is validated on the host at construction (ValueError); the device tables are made
    on first use, so a model can be built and inspected without a device."""
    _CHECK = "rc_model_wide16_check_"
    _CREATE = "rc_model_create_static_wide16"
    _MAX = N.MAX_WIDE16_SYMBOLS
    _WHAT = "wide16"

    @classmethod
    def from_counts(cls, counts, target_total=65536, ctx=None):
        """A histogram scaled to target_total with every symbol kept encodable
        (rc_quantize_counts_wide16 with RC_Q_ALL_SYMBOLS; more symbols than target_total is a
        ValueError)."""
        from .model_build import quantize_counts_wide16
        c, cum, total = quantize_counts_wide16(counts, target_total, all_symbols=True)
        return cls(c, cum, total, ctx=ctx)

    def plan(self):
        """rc_model_wide16_plan_: what the launchers use for this table, as a dict."""
        out = (ctypes.c_uint32 * 8)()
        N.check(N.load().rc_model_wide16_plan_(self.n_symbols, self.total, out),
                "rc_model_wide16_plan_")
        keys = ("enc_lanes", "enc_lds", "enc_layout", "enc_table_bytes", "dec_lanes", "dec_lds",
                "dec_symof_bits", "dec_shift")
        d = dict(zip(keys, (int(v) for v in out)))
        d["dec_symof_bytes"] = 2 << d["dec_symof_bits"]
        d["dec_row_bytes"] = 4 * (self.n_symbols + 2)
        return d


class Wide16FineModel(Wide16StaticModel):
    """rc_model_create_static_wide16_fine: a wide16 static model whose total lies above 65536, up
    to 2^24, so that a table over thousands of rare symbols, or over all 65536 with every one
    encodable, still tells them apart.  The wide16 batch calls and chunk helpers take it as they
    take a Wide16StaticModel, with the same contract; a table whose total is at most 65536 is a
    Wide16StaticModel's and is refused here (ValueError), so each table has one class.

    The table is validated on the host at construction (ValueError); the device tables are made
    on first use, so a model can be built and inspected without a device."""
    _CHECK = "rc_model_wide16_fine_check_"
    _CREATE = "rc_model_create_static_wide16_fine"
    _WHAT = "wide16 fine"
    _TOTALS = "65537..16777216"

    @classmethod
    def from_counts(cls, counts, target_total=1 << 20, ctx=None):
        """A histogram scaled to target_total (65537..2^24) with every symbol kept encodable
        (rc_quantize_counts_wide16_fine with RC_Q_ALL_SYMBOLS)."""
        from .model_build import quantize_counts_wide16_fine
        c, cum, total = quantize_counts_wide16_fine(counts, target_total, all_symbols=True)
        return cls(c, cum, total, ctx=ctx)

    def plan(self):
        """rc_model_wide16_fine_plan_: what the launchers use for this table, as a dict."""
        out = (ctypes.c_uint32 * 8)()
        N.check(N.load().rc_model_wide16_fine_plan_(self.n_symbols, self.total, out),
                "rc_model_wide16_fine_plan_")
        keys = ("enc_lanes", "enc_lds", "enc_layout", "enc_table_bytes", "dec_lanes", "dec_lds",
                "dec_bucket_bits", "dec_shift")
        d = dict(zip(keys, (int(v) for v in out)))
        d["dec_bucket_bytes"] = (2 << d["dec_bucket_bits"]) + 4  # (with the sentinel)
        n_occ = int(np.count_nonzero(self.c))
        d["dec_occ_bytes"] = 2 * (n_occ + (n_occ & 1))
        d["dec_rcum_bytes"] = 4 * (n_occ + 2)
        return d

    def max_bits_per_symbol(self):
        """The bits to plan a slot with (slot_capacity): the costliest symbol's ideal
        log2(total / c_min), up to 24, and 1/8 bit for what the coder loses at these totals: the
        rounding of range / total (under 2^-23 bit) and range_reduction_expansion (1.44 bits on
        average on fewer than one symbol in 256: under 0.006 bit).  It is no hard bound: one
        symbol can settle 11 bytes (include/range_coder.h), and a slot that is too small is
        RC_F_CAPACITY with the exact length, which encode_chunks_wide16 encodes again."""
        return WideStaticModel.max_bits_per_symbol(self) + 0.125


# ----------------------------------------------------------------------------- batch API
def slot_capacity(n_symbols, bits_per_symbol, slack=1.02):
    """A per-chunk output slot size (16-B multiple) for n symbols at a given worst bit cost."""
    return int(math.ceil((n_symbols * bits_per_symbol / 8.0) * slack + 64)) + 15 & ~15


def _sym16(t, name):
    """A uint16 symbol tensor (int16 tensors are viewed as uint16: the bits are the symbols)."""
    torch = _torch()
    u16 = getattr(torch, "uint16", None)  # (absent from older torch: int16 tensors still work)
    _check_dev(t, name, (torch.int16,) if u16 is None else (u16, torch.int16))
    return t


def _check_syms(t, name, wide):
    if wide:
        _sym16(t, name)
    else:
        _check_dev(t, name, (_torch().uint8,))


def _encode_batch(native, model, syms, idx, sym_off, out, out_off, out_len, flags, wide=False):
    """The four encode_batch* calls: the checks, the result tensors, the stream and the native
    call `native` (idx: None, or the index stream that follows syms in its arguments)."""
    torch = _torch()
    _check_syms(syms, "syms", wide)
    if idx is not None:
        _check_dev(idx, "idx", (torch.uint8,))
    _check_dev(out, "out", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    _check_dev(out_off, "out_off", (torch.int64, torch.uint64))
    # (idx is indexed exactly like syms, so a tensor as long as syms covers every read)
    if idx is not None and idx.numel() < syms.numel():
        raise ValueError("idx must hold one index per symbol: at least syms.numel() entries")
    n = sym_off.numel() - 1
    if out_off.numel() != n + 1:
        raise ValueError("out_off must have n_chunks + 1 entries")
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int64, device=syms.device)
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=syms.device)
    ctx = model.ctx
    ctx.bind_stream()
    side = () if idx is None else (_ptr(idx),)
    N.check(getattr(ctx._lib, native)(ctx.handle, model.handle, _ptr(syms), *side, _ptr(sym_off),
                                      n, _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(flags)),
            native)
    return out_len[:n], flags[:n]


def _decode_batch(native, model, code, code_off, code_len, idx, syms_out, sym_off, flags,
                  wide=False):
    """The four decode_batch* calls (idx: None, or the index stream that follows code_len)."""
    torch = _torch()
    _check_dev(code, "code", (torch.uint8,))
    if idx is not None:
        _check_dev(idx, "idx", (torch.uint8,))
    _check_syms(syms_out, "syms_out", wide)
    for name, t in (("code_off", code_off), ("code_len", code_len), ("sym_off", sym_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
    # (idx is indexed exactly like syms_out, so a tensor as long as syms_out covers every read)
    if idx is not None and idx.numel() < syms_out.numel():
        raise ValueError("idx must hold one index per symbol: at least syms_out.numel() entries")
    n = sym_off.numel() - 1
    if code_off.numel() < n or code_len.numel() < n:
        raise ValueError("code_off/code_len need n_chunks entries")
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=code.device)
    ctx = model.ctx
    ctx.bind_stream()
    side = () if idx is None else (_ptr(idx),)
    N.check(getattr(ctx._lib, native)(ctx.handle, model.handle, _ptr(code), _ptr(code_off),
                                      _ptr(code_len), *side, _ptr(syms_out), _ptr(sym_off), n,
                                      _ptr(flags)), native)
    return flags[:n]


def _u8_chunk(c):
    return (np.frombuffer(bytes(c), dtype=np.uint8) if not isinstance(c, np.ndarray)
            else np.ascontiguousarray(c, dtype=np.uint8))


def _u16_chunk(c):
    a = np.asarray(c)
    if a.size and (a.min() < 0 or a.max() > 0xFFFF):
        raise BadSymbolError("symbol outside 0..65535")
    return np.ascontiguousarray(a, dtype=np.uint16).reshape(-1)


def _offsets(lens, hint):
    """int64 [0, cumsum(lens)] of a batch's chunk lengths (ChunkTooLongError past the limit)."""
    if int(lens.max()) > N.MAX_CHUNK_SYMBOLS:
        raise ChunkTooLongError(f"chunk of {int(lens.max())} symbols: the batch API takes at "
                                f"most {N.MAX_CHUNK_SYMBOLS} per chunk{hint}")
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _to_dev(arrs, total, dev):
    """The chunks' arrays back to back on the device (uint16 travels as int16, bit for bit)."""
    cat = np.concatenate(arrs) if total else np.zeros(1, arrs[0].dtype)
    return _torch().from_numpy(cat.view(np.int16) if cat.dtype == np.uint16 else cat).to(dev)


def _raise_flagged(fl):
    for k in np.flatnonzero(fl):
        _raise_for_flag(int(fl[k]), f"chunk {k}")


def _encode_chunks(batch, model, arrs, idxs, raise_on_error, hint=""):
    """The four encode_chunks*: upload, encode with `batch`, encode once more with exact slots if
    a chunk overflowed its first one, download.  arrs: one symbol array per chunk (uint8 or
    uint16); idxs: None, or one index array per chunk for batch's idx argument."""
    torch = _torch()
    dev = torch.device("cuda", model.ctx.device)
    n = len(arrs)
    if n == 0:
        return []
    sym_off = _offsets(np.array([len(a) for a in arrs], dtype=np.int64), hint)
    bits = model.max_bits_per_symbol()
    caps = np.array([slot_capacity(int(L), bits) for L in np.diff(sym_off)], dtype=np.int64)
    ins = (_to_dev(arrs, sym_off[-1], dev),)
    if idxs is not None:
        ins += (_to_dev(idxs, sym_off[-1], dev),)
    soff_d = torch.from_numpy(sym_off).to(dev)
    for attempt in range(2):
        out_off = np.zeros(n + 1, dtype=np.int64)
        out_off[1:] = np.cumsum(caps)
        out_d = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
        out_len, flags = batch(model, *ins, soff_d, out_d, torch.from_numpy(out_off).to(dev))
        fl = flags.cpu().numpy()
        ol = out_len.cpu().numpy()
        if attempt == 0 and np.any(fl == N.F_CAPACITY):
            caps = np.where(fl == N.F_CAPACITY, (ol + 15) // 16 * 16, caps)
            continue
        break
    host = out_d.cpu().numpy()
    if raise_on_error:
        _raise_flagged(fl)
    return [bytes(host[out_off[k]: out_off[k] + min(ol[k], caps[k])]) for k in range(n)]


def _decode_chunks(batch, model, codes, counts, idxs, raise_on_error, wide=False, hint=""):
    """The four decode_chunks*: counts[k] symbols from codes[k], decoded with `batch` (idxs: None,
    or one index array per chunk for its idx argument).  Returns uint8 (wide: uint16) arrays."""
    torch = _torch()
    dev = torch.device("cuda", model.ctx.device)
    n = len(codes)
    if n == 0:
        return []
    codes = [bytes(c) for c in codes]
    clen = np.array([len(c) for c in codes], dtype=np.int64)
    coff = np.zeros(n, dtype=np.int64)
    coff[1:] = np.cumsum(clen)[:-1]
    sym_off = _offsets(np.asarray(counts, dtype=np.int64), hint)
    blob = np.frombuffer(b"".join(codes) + b"\0" * 16, dtype=np.uint8)
    code_d = torch.from_numpy(blob.copy()).to(dev)
    side = () if idxs is None else (_to_dev(idxs, sym_off[-1], dev),)
    syms_d = torch.empty(max(int(sym_off[-1]), 1), dtype=torch.int16 if wide else torch.uint8,
                         device=dev)
    flags = batch(model, code_d, torch.from_numpy(coff).to(dev), torch.from_numpy(clen).to(dev),
                  *side, syms_d, torch.from_numpy(sym_off).to(dev))
    fl = flags.cpu().numpy()
    host = syms_d.cpu().numpy()
    if wide:
        host = host.view(np.uint16)
    if raise_on_error:
        _raise_flagged(fl)
    return [host[sym_off[k]: sym_off[k + 1]].copy() for k in range(n)]


def encode_batch(model, syms, sym_off, out, out_off, out_len=None, flags=None):
    """rc_encode_batch on torch tensors (async on torch's current stream).

    syms uint8[...]; sym_off int64/uint64[n+1]; out uint8[...]; out_off int64/uint64[n+1].
    Returns (out_len int64[n], flags int32[n]) device tensors."""
    return _encode_batch("rc_encode_batch", model, syms, None, sym_off, out, out_off, out_len,
                         flags)


def decode_batch(model, code, code_off, code_len, syms_out, sym_off, flags=None):
    """rc_decode_batch on torch tensors (async on torch's current stream).  Returns flags."""
    return _decode_batch("rc_decode_batch", model, code, code_off, code_len, None, syms_out,
                         sym_off, flags)


def encode_chunks(model, chunks, raise_on_error=True):
    """Encode a list of symbol sequences (bytes / uint8 arrays), one chunk each.

    Host-resident convenience: uploads, encodes on the GPU, re-encodes chunks that overflowed
    their first slot with their exact length, downloads.  Returns a list of bytes."""
    return _encode_chunks(encode_batch, model, [_u8_chunk(c) for c in chunks], None,
                          raise_on_error, " (use Encoder for longer streams)")


def decode_chunks(model, codes, counts, raise_on_error=True):
    """Decode a list of code streams; counts[k] symbols each (the count is out-of-band,
    as in the reference: sample_impl.rs:113-120).  Returns a list of uint8 numpy arrays."""
    return _decode_chunks(decode_batch, model, codes, counts, None, raise_on_error,
                          hint=" (use Decoder for longer streams)")


# ------------------------------------------------------------- batch API, a model per symbol
def encode_batch_indexed(model_set, syms, idx, sym_off, out, out_off, out_len=None, flags=None):
    """rc_encode_batch_indexed on torch tensors (async on torch's current stream): encode_batch
    with idx uint8[...], one row of model_set per symbol, indexed like syms.
    Returns (out_len int64[n], flags int32[n]) device tensors."""
    return _encode_batch("rc_encode_batch_indexed", model_set, syms, idx, sym_off, out, out_off,
                         out_len, flags)


def decode_batch_indexed(model_set, code, code_off, code_len, idx, syms_out, sym_off, flags=None):
    """rc_decode_batch_indexed on torch tensors (async on torch's current stream): decode_batch
    with idx uint8[...], one row of model_set per symbol, indexed like syms_out.  Returns flags."""
    return _decode_batch("rc_decode_batch_indexed", model_set, code, code_off, code_len, idx,
                         syms_out, sym_off, flags)


def encode_chunks_indexed(model_set, chunks, raise_on_error=True):
    """encode_chunks over a list of (symbols, indexes) pairs (bytes / uint8 arrays of equal
    length), one chunk each: symbol i is coded with row indexes[i].  Returns a list of bytes."""
    pairs = [(_u8_chunk(s), _u8_chunk(x)) for s, x in chunks]
    for k, (s, x) in enumerate(pairs):
        if len(s) != len(x):
            raise ValueError(f"chunk {k}: {len(s)} symbols, {len(x)} indexes")
    return _encode_chunks(encode_batch_indexed, model_set, [s for s, _ in pairs],
                          [x for _, x in pairs], raise_on_error)


def decode_chunks_indexed(model_set, chunks, raise_on_error=True):
    """decode_chunks over a list of (code, indexes) pairs: chunk k decodes len(indexes) symbols,
    symbol i with row indexes[i].  Returns a list of uint8 numpy arrays."""
    idxs = [_u8_chunk(x) for _, x in chunks]
    return _decode_chunks(decode_batch_indexed, model_set, [c for c, _ in chunks],
                          [len(x) for x in idxs], idxs, raise_on_error)


# ------------------------------------------------------------- batch API, a model per chunk
def encode_batch_chunk_set(chunk_set, class_of, syms, sym_off, out, out_off, out_len=None,
                           flags=None):
    """rc_encode_batch_chunk_set on torch tensors (async on torch's current stream): encode_batch
    with class_of uint8[n], the row of chunk_set (a ChunkModelSet) that codes chunk k.
    Returns (out_len int64[n], flags int32[n]) device tensors."""
    torch = _torch()
    _check_syms(syms, "syms", False)
    _check_dev(class_of, "class_of", (torch.uint8,))
    _check_dev(out, "out", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    _check_dev(out_off, "out_off", (torch.int64, torch.uint64))
    n = sym_off.numel() - 1
    if out_off.numel() != n + 1:
        raise ValueError("out_off must have n_chunks + 1 entries")
    if class_of.numel() < n:
        raise ValueError("class_of must hold one class per chunk")
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int64, device=syms.device)
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=syms.device)
    ctx = chunk_set.ctx
    ctx.bind_stream()
    N.check(ctx._lib.rc_encode_batch_chunk_set(
        ctx.handle, chunk_set.handle, _ptr(class_of), _ptr(syms), _ptr(sym_off), n, _ptr(out),
        _ptr(out_off), _ptr(out_len), _ptr(flags)), "rc_encode_batch_chunk_set")
    return out_len[:n], flags[:n]


def decode_batch_chunk_set(chunk_set, class_of, code, code_off, code_len, syms_out, sym_off,
                           flags=None):
    """rc_decode_batch_chunk_set on torch tensors (async on torch's current stream): decode_batch
    with class_of uint8[n], the row of chunk_set that codes chunk k.  Returns flags."""
    torch = _torch()
    _check_dev(code, "code", (torch.uint8,))
    _check_dev(class_of, "class_of", (torch.uint8,))
    _check_syms(syms_out, "syms_out", False)
    for name, t in (("code_off", code_off), ("code_len", code_len), ("sym_off", sym_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
    n = sym_off.numel() - 1
    if code_off.numel() < n or code_len.numel() < n:
        raise ValueError("code_off/code_len need n_chunks entries")
    if class_of.numel() < n:
        raise ValueError("class_of must hold one class per chunk")
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=code.device)
    ctx = chunk_set.ctx
    ctx.bind_stream()
    N.check(ctx._lib.rc_decode_batch_chunk_set(
        ctx.handle, chunk_set.handle, _ptr(class_of), _ptr(code), _ptr(code_off), _ptr(code_len),
        _ptr(syms_out), _ptr(sym_off), n, _ptr(flags)), "rc_decode_batch_chunk_set")
    return flags[:n]


def _class_tensor(chunk_set, class_of, n):
    cls = np.ascontiguousarray(class_of, dtype=np.uint8).reshape(-1)
    if len(cls) != n:
        raise ValueError(f"{n} chunks, {len(cls)} classes")
    torch = _torch()
    return torch.from_numpy(cls if n else np.zeros(1, np.uint8)).to(
        torch.device("cuda", chunk_set.ctx.device))


def encode_chunks_chunk_set(chunk_set, class_of, chunks, raise_on_error=True):
    """encode_chunks over a list of symbol chunks (bytes / uint8 arrays), chunk k against row
    class_of[k] of a ChunkModelSet.  Returns a list of bytes."""
    arrs = [_u8_chunk(c) for c in chunks]
    cls_d = _class_tensor(chunk_set, class_of, len(arrs))
    return _encode_chunks(lambda m, *a: encode_batch_chunk_set(m, cls_d, *a), chunk_set, arrs, None,
                          raise_on_error)


def decode_chunks_chunk_set(chunk_set, class_of, codes, counts, raise_on_error=True):
    """decode_chunks against a ChunkModelSet: counts[k] symbols from codes[k] with row
    class_of[k].  Returns a list of uint8 numpy arrays."""
    cls_d = _class_tensor(chunk_set, class_of, len(codes))
    return _decode_chunks(lambda m, *a: decode_batch_chunk_set(m, cls_d, *a), chunk_set, codes,
                          counts, None, raise_on_error)


# ------------------------------------------------- batch API, the previous symbol picks the model
def encode_batch_order1(o1_set, syms, sym_off, out, out_off, out_len=None, flags=None):
    """rc_encode_batch_order1 on torch tensors (async on torch's current stream): encode_batch
    against an Order1ModelSet, the row of each symbol chosen by the chunk's previous symbol.
    Returns (out_len int64[n], flags int32[n]) device tensors."""
    return _encode_batch("rc_encode_batch_order1", o1_set, syms, None, sym_off, out, out_off,
                         out_len, flags)


def decode_batch_order1(o1_set, code, code_off, code_len, syms_out, sym_off, flags=None):
    """rc_decode_batch_order1 on torch tensors (async on torch's current stream): decode_batch
    against an Order1ModelSet, the row of each symbol chosen by the previous decoded symbol.
    Returns flags."""
    return _decode_batch("rc_decode_batch_order1", o1_set, code, code_off, code_len, None,
                         syms_out, sym_off, flags)


def encode_chunks_order1(o1_set, chunks, raise_on_error=True):
    """encode_chunks over a list of symbol chunks (bytes / uint8 arrays) against an
    Order1ModelSet.  Returns a list of bytes."""
    return _encode_chunks(encode_batch_order1, o1_set, [_u8_chunk(c) for c in chunks], None,
                          raise_on_error)


def decode_chunks_order1(o1_set, codes, counts, raise_on_error=True):
    """decode_chunks against an Order1ModelSet: counts[k] symbols from codes[k] (the count is
    out-of-band, as in the reference).  Returns a list of uint8 numpy arrays."""
    return _decode_chunks(decode_batch_order1, o1_set, codes, counts, None, raise_on_error)


# --------------------------------------------------------------- batch API, 16-bit symbols
def encode_batch_wide(model, syms, sym_off, out, out_off, out_len=None, flags=None):
    """rc_encode_batch_wide on torch tensors (async on torch's current stream): encode_batch with
    syms uint16[...] (int16 is taken as uint16) against a WideStaticModel; sym_off counts symbols.
    Returns (out_len int64[n], flags int32[n]) device tensors."""
    return _encode_batch("rc_encode_batch_wide", model, syms, None, sym_off, out, out_off,
                         out_len, flags, wide=True)


def decode_batch_wide(model, code, code_off, code_len, syms_out, sym_off, flags=None):
    """rc_decode_batch_wide on torch tensors (async on torch's current stream): decode_batch into
    syms_out uint16[...] (or int16, written as uint16).  Returns flags."""
    return _decode_batch("rc_decode_batch_wide", model, code, code_off, code_len, None, syms_out,
                         sym_off, flags, wide=True)


def encode_batch_wide16(model, syms, sym_off, out, out_off, out_len=None, flags=None):
    """rc_encode_batch_wide16 on torch tensors (async on torch's current stream):
    encode_batch_wide against a Wide16StaticModel or a Wide16FineModel (up to 65536 symbols).
    Returns (out_len, flags)."""
    return _encode_batch("rc_encode_batch_wide16", model, syms, None, sym_off, out, out_off,
                         out_len, flags, wide=True)


def decode_batch_wide16(model, code, code_off, code_len, syms_out, sym_off, flags=None):
    """rc_decode_batch_wide16 on torch tensors (async on torch's current stream):
    decode_batch_wide against a Wide16StaticModel or a Wide16FineModel.  Returns flags."""
    return _decode_batch("rc_decode_batch_wide16", model, code, code_off, code_len, None,
                         syms_out, sym_off, flags, wide=True)


def encode_chunks_wide16(model, chunks, raise_on_error=True):
    """encode_chunks_wide against a Wide16StaticModel or a Wide16FineModel.  Returns a list of
    bytes."""
    return _encode_chunks(encode_batch_wide16, model, [_u16_chunk(c) for c in chunks], None,
                          raise_on_error)


def decode_chunks_wide16(model, codes, counts, raise_on_error=True):
    """decode_chunks_wide against a Wide16StaticModel or a Wide16FineModel.  Returns a list of
    uint16 arrays."""
    return _decode_chunks(decode_batch_wide16, model, codes, counts, None, raise_on_error,
                          wide=True)


def encode_chunks_wide(model, chunks, raise_on_error=True):
    """encode_chunks over a list of 16-bit symbol sequences (uint16 arrays or lists of ints), one
    chunk each, against a WideStaticModel.  Returns a list of bytes."""
    return _encode_chunks(encode_batch_wide, model, [_u16_chunk(c) for c in chunks], None,
                          raise_on_error)


def decode_chunks_wide(model, codes, counts, raise_on_error=True):
    """decode_chunks against a WideStaticModel; counts[k] symbols each.  Returns a list of uint16
    numpy arrays."""
    return _decode_chunks(decode_batch_wide, model, codes, counts, None, raise_on_error, wide=True)


# ----------------------------------------------------------------------------- stream API


class RangeCoder:
    """RangeCoder (src/range_coder.rs:7-146): the public accessors of one coder state.

    A snapshot: a stream's state lives with its GPU call between calls (rc_stream_state), so
    Encoder.range_coder and Decoder.range_coder() return a copy.  param_update / left_shift are
    pub(crate) in the reference and run only inside the kernels."""

    TOP8 = 1 << (64 - 8)  # range_coder.rs:23
    TOP16 = 1 << (64 - 16)  # range_coder.rs:24

    def __init__(self, lower_bound=0, range_=M64):  # Default (:13-20)
        self._low, self._range = int(lower_bound), int(range_)

    @classmethod
    def new(cls):  # :26-28
        return cls()

    def lower_bound(self):  # :30-32
        return self._low

    def range(self):  # :33-35
        return self._range

    def range_par_total(self, total_freq):  # :38-40
        if int(total_freq) == 0:
            raise BadModelError("range_par_total: attempt to divide by zero")
        return self._range // int(total_freq)

    def upper_bound(self):  # :138-146
        s = self._low + self._range
        if s > M64:
            raise RangeCoderError(f"UpperBoundOverflow {{ lower_bound: {self._low}, "
                                  f"range: {self._range} }}")
        return s

    def __eq__(self, other):
        return (isinstance(other, RangeCoder) and
                (self._low, self._range) == (other._low, other._range))

    def __repr__(self):
        return f"RangeCoder(lower_bound={self._low:#x}, range={self._range:#x})"


class ByteCount:
    """The value Encoder.encode returns: the number of bytes that symbol settled
    (encoder.rs:34-36).  Symbols are staged and coded on the GPU in batches, so the count is
    known once the symbol is flushed: int(), comparisons and arithmetic flush on demand (one
    launch for everything staged); code that ignores the value, as sample_impl.rs:96 does,
    never waits for it."""

    __slots__ = ("_enc", "_i")

    def __init__(self, enc, i):
        self._enc, self._i = enc, i

    def __int__(self):
        return self._enc._count(self._i)

    __index__ = __int__

    def __eq__(self, other):
        return int(self) == other

    def __ne__(self, other):
        return int(self) != other

    def __lt__(self, other):
        return int(self) < other

    def __le__(self, other):
        return int(self) <= other

    def __gt__(self, other):
        return int(self) > other

    def __ge__(self, other):
        return int(self) >= other

    def __hash__(self):
        return hash(int(self))

    def __bool__(self):
        return int(self) != 0

    def __float__(self):
        return float(int(self))

    def __add__(self, other):
        return int(self) + other

    __radd__ = __add__

    def __sub__(self, other):
        return int(self) - other

    def __rsub__(self, other):
        return other - int(self)

    def __mul__(self, other):
        return int(self) * other

    __rmul__ = __mul__

    def __floordiv__(self, other):
        return int(self) // other

    def __repr__(self):
        return repr(int(self))


def _u32(v, what):
    v = int(v)
    if not 0 <= v <= 0xFFFFFFFF:
        raise RangeCoderError(f"{what} = {v} is not a u32")
    return v


def _canonical_find_index(pmodel):
    """True when decoding may use FreqTable::find_index's binary search (sample_impl.rs:27-45):
    the model does not override find_index (pmodel.rs:12), or says its override has those
    semantics (canonical_find_index = True in the class that defines the override)."""
    t = type(pmodel)
    # (cached per class and per the find_index / canonical_find_index the class resolves to
    # now: the MRO scan is ~1 us of every decode call, and a class patched after its first
    # decode gets a new key)
    key = (t, getattr(t, "find_index", None), getattr(t, "canonical_find_index", None))
    hit = _CANONICAL.get(key)
    if hit is None:
        owner = next((k for k in t.__mro__ if "find_index" in vars(k)), None)
        hit = (owner is None or owner is PModel or owner is FreqTable or
               bool(vars(owner).get("canonical_find_index", False)))
        if len(_CANONICAL) > 4096:
            _CANONICAL.clear()
        _CANONICAL[key] = hit
    return hit


_CANONICAL = {}  # (class, find_index, flag) -> whether find_index keeps FreqTable's semantics


def _find_index_rfreq(st, total):
    """rfreq of FreqTable::find_index (sample_impl.rs:29): (data - lower_bound) / range_par_total.
    Only for error reports (the decode itself ran on the GPU)."""
    return ((st.data - st.lower_bound) & M64) // (st.range // total)


def _decode_error(st, sig, flags, where):
    """Raise the reference's error for a decode that stopped at state st under table sig."""
    if flags & N.F_BAD_MODEL:
        c, cum, total = sig
        if total == 0 or not c:
            raise BadModelError(f"{where}: range_par_total: attempt to divide by zero")
        rf = _find_index_rfreq(st, total)
        left, right = 0, len(c) - 1  # the binary search of sample_impl.rs:31-44
        while left < right:
            mid = (left + right) // 2
            if cum[mid + 1] <= rf:
                left = mid + 1
            else:
                right = mid
        _raise_bad_model(st.lower_bound, st.range, c[left], cum[left], total, where)
    _raise_for_flag(flags, where)


_U32_PACK = {}  # alphabet size -> struct.Struct of that many little-endian u32


def _table_of(pmodel):
    """(c, cum, total) of a PModel, read through c_freq / cum_freq / total_freq over its
    alphabet, as the reference's decode reads them (decoder.rs:38-50, sample_impl.rs:27-45)."""
    fast = getattr(pmodel, "_rc_table", None)
    if fast is not None:
        return fast()
    n = pmodel.alphabet_count()
    return (tuple(int(pmodel.c_freq(i)) for i in range(n)),
            tuple(int(pmodel.cum_freq(i)) for i in range(n)), int(pmodel.total_freq()))


class Encoder:
    """Encoder (src/encoder.rs:7-55) for ONE stream, with the reference's per-call semantics.

    encode(pmodel, index) reads (c_freq(index), cum_freq(index), total_freq()) at that call, as
    encoder.rs:24-31 does, so a model the caller changes between calls (an adaptive PModel) is
    coded exactly as the reference codes it.  The triples are staged and coded on the GPU by the
    resumable stream kernel (rc_stream_encode_host) when a result is needed: peek_code(),
    range_coder, finish(), the int value of encode()'s ByteCount, or every 2^20 symbols.  A
    stream has no length limit.  Errors the reference panics on surface as RangeCoderError
    subclasses at the call that flushes them; the encoder is then unusable, as after a panic."""

    FLUSH_AT = 1 << 20
    SMALL = 64  # flushes of up to this many symbols use reused ctypes buffers

    def __init__(self, ctx=None):
        self._ctx = ctx
        self._bufs = None          # (triples, output, counts) ctypes buffers of the small flushes
        self._state = N.StreamState.fresh()
        self._code = bytearray()
        self._trip = []            # staged (c, cum, total), flat
        self._counts = bytearray()  # encode() return values of the flushed symbols
        self._staged0 = 0          # index of the first staged symbol
        self._finished = False
        self._exc = None           # the error of the failing symbol, raised again after it

    @classmethod
    def new(cls):  # encoder.rs:14-16
        return cls()

    def encode(self, pmodel, index):  # encoder.rs:24-37
        if self._finished:
            raise FinishedError("encode after finish")
        c = _u32(pmodel.c_freq(index), "c_freq")
        cum = _u32(pmodel.cum_freq(index), "cum_freq")
        total = _u32(pmodel.total_freq(), "total_freq")
        if c == 0:  # range_coder.rs:83-85 would never terminate
            raise ZeroFrequencyError(f"encode({index}): c_freq == 0")
        if total == 0:  # range_coder.rs:38-40 divides by zero
            raise BadModelError(f"encode({index}): total_freq == 0")
        self._trip += (c, cum, total)
        i = self._staged0 + len(self._trip) // 3 - 1
        if len(self._trip) >= 3 * self.FLUSH_AT:
            self._flush()
        return ByteCount(self, i)

    def peek_code(self):  # encoder.rs:18-20: the bytes emitted so far
        self._flush()
        return bytes(self._code)

    @property
    def range_coder(self):  # the pub field of encoder.rs:8 (a snapshot)
        self._flush()
        return RangeCoder(self._state.lower_bound, self._state.range)

    def finish(self):  # encoder.rs:40-46
        if self._finished:
            raise FinishedError("finish twice")
        self._flush(finish=True)
        self._finished = True
        return bytes(self._code)

    def _count(self, i):
        if i >= self._staged0:
            self._flush()
        if i >= len(self._counts):
            raise RangeCoderError(f"symbol {i} was not coded (an earlier symbol failed)")
        return self._counts[i]

    def _flush(self, finish=False):
        if self._state.flags:  # the reference panicked at an earlier call
            if self._exc is not None:
                raise self._exc
            _raise_for_flag(self._state.flags, "encode")
        n = len(self._trip) // 3
        if n == 0 and not finish:
            return
        ctx = self._ctx or default_context()
        cap = N.stream_max_bytes(n, finish)
        small = n <= self.SMALL
        if small:  # (numpy arrays and their .ctypes cost ~1 us each per call)
            if self._bufs is None:
                self._bufs = ((ctypes.c_uint32 * (3 * self.SMALL))(),
                              ctypes.create_string_buffer(N.stream_max_bytes(self.SMALL, True)),
                              ctypes.create_string_buffer(self.SMALL))
            tb, out, nb = self._bufs
            tb[: 3 * n] = self._trip
            args = (tb, out, nb)
        else:
            out = np.empty(max(cap, 1), np.uint8)
            nb = np.empty(max(n, 1), np.uint8)
            trip = np.array(self._trip, dtype=np.uint32)  # (held: _np_ptr keeps no reference)
            args = (_np_ptr(trip), _np_ptr(out), _np_ptr(nb))
        out_len = ctypes.c_uint64()
        fl = ctypes.c_uint32()
        n0 = self._state.n
        rc = ctx._lib.rc_stream_encode_host(ctx.handle, ctypes.byref(self._state), args[0], n,
                                            args[1], cap, ctypes.byref(out_len), args[2],
                                            1 if finish else 0, ctypes.byref(fl))
        if rc not in (N.RC_OK, N.RC_E_CHUNK):
            N.check(rc, "rc_stream_encode_host")
        done = self._state.n - n0
        if small:
            self._code += out.raw[: out_len.value]
            self._counts += nb.raw[:done]
        else:
            self._code += out[: out_len.value].tobytes()
            self._counts += nb[:done].tobytes()
        failed = self._trip[3 * done: 3 * done + 3]
        self._staged0 += n
        self._trip = []
        if fl.value:
            where = f"encode (symbol {self._state.n})"
            try:
                if fl.value & N.F_BAD_MODEL and len(failed) == 3:
                    _raise_bad_model(self._state.lower_bound, self._state.range, *failed, where)
                _raise_for_flag(fl.value, where)
            except RangeCoderError as e:
                self._exc = e
                raise


class Decoder:
    """Decoder (src/decoder.rs:6-55) for ONE stream, with the reference's per-call semantics.

    Decoder(code) runs Decoder::new (the first 8 bytes; a shorter code raises as the reference
    panics).  decode(pmodel) reads the model's table at that call (c_freq / cum_freq /
    total_freq over alphabet_count()) and decodes with FreqTable::find_index's binary search
    and param_update (sample_impl.rs:27-45, decoder.rs:38-54), evaluated on the GPU by the
    resumable stream kernel.  Symbols are decoded ahead in blocks that double while the table
    stays the same; when the caller's table changes (an adaptive PModel), the state at that
    symbol is re-derived and decoding continues under the new table, so every symbol is decoded
    with the table the caller held at its call.

    A PModel that overrides find_index (pmodel.rs:12) gets it called, as decoder.rs:40 does:
    once per symbol, with this decoder (range_coder(), data() give the exact state), and the
    index it returns is what param_update uses (one GPU step per symbol, with the table cut to
    that index's (c_freq, cum_freq)).  That path is launch-latency-bound; a subclass whose
    override keeps FreqTable's binary-search semantics can set canonical_find_index = True to
    stay on the decode-ahead path.  n_symbols (optional, out-of-band as in
    sample_impl.rs:113-120) only bounds the decode-ahead."""

    MAX_BLOCK = 1 << 20
    SMALL = 64  # calls of up to this many symbols decode into a reused buffer

    def __init__(self, code, n_symbols=None, ctx=None):
        self._ctx = ctx or default_context()
        self._code = np.frombuffer(bytes(code), dtype=np.uint8)
        self._code_ptr = _np_ptr(self._code)  # (the array lives as long as the decoder)
        self._small = ctypes.create_string_buffer(self.SMALL)  # output of the short calls
        self._fl = ctypes.c_uint32()
        self._limit = None if n_symbols is None else int(n_symbols)
        self._arrays = (None, None)  # table signature -> (c, cum) uint32 arrays
        st = N.StreamState.fresh()
        if len(self._code) < 8:  # Decoder::new panics (decoder.rs:21, :33)
            raise TruncatedStreamError("code shorter than 8 bytes")
        self._run(st, ((1,), (0,), 1), 0)  # Decoder::new: prime the data window
        self._start = st            # state at the first symbol of the current block
        self._end = st              # state after the block (before a failing symbol)
        self._buf = np.zeros(0, np.uint8)
        self._bpos = 0
        self._sig = None
        self._err = 0               # flag of the symbol after the block, if it failed
        self._block = 1
        self._taken = 0             # symbols returned

    @classmethod
    def new(cls, code):  # decoder.rs:14-23
        return cls(code)

    def _run(self, st, sig, n):
        """Decode n symbols from state st (updated) under table sig; returns (symbols, flags)."""
        na = len(sig[0])
        if not 1 <= na <= 256 or len(sig[1]) != na:
            raise RangeCoderError(f"alphabet of {na} symbols (the GPU decoders take 1..256)")
        if self._arrays[0] != sig:  # the table as packed u32 (struct: ~2 us, numpy ~10-28 us)
            pk = _U32_PACK.get(na) or _U32_PACK.setdefault(na, struct.Struct(f"<{na}I"))
            try:
                self._arrays = (sig, (pk.pack(*sig[0]), pk.pack(*sig[1])))
            except struct.error as e:
                raise RangeCoderError(f"table entry outside u32: {e}") from None
        c, cum = self._arrays[1]
        small = n <= self.SMALL
        out = self._small if small else np.empty(n, np.uint8)
        fl = self._fl
        n0 = st.n
        ctx = self._ctx
        rc = ctx._lib.rc_stream_decode_host(ctx.handle, c, cum, na,
                                            _u32(sig[2], "total_freq"), ctypes.byref(st),
                                            self._code_ptr, len(self._code),
                                            out if small else _np_ptr(out), n, ctypes.byref(fl))
        if rc not in (N.RC_OK, N.RC_E_CHUNK):
            N.check(rc, "rc_stream_decode_host")
        got = st.n - n0
        return (out.raw[:got] if small else out[:got]), fl.value

    @staticmethod
    def _copy(st):
        return N.StreamState.from_buffer_copy(st)

    def _here(self):
        """The state at the current symbol (re-derived inside a block; the block then starts
        here, so the next call needs no re-derivation)."""
        if self._bpos == 0:
            return self._start
        if self._bpos == len(self._buf):
            st = self._copy(self._end)
            st.flags = 0
            return st
        st = self._copy(self._start)
        self._run(st, self._sig, self._bpos)
        self._start, self._buf, self._bpos = st, self._buf[self._bpos:], 0
        return st

    def decode(self, pmodel):  # decoder.rs:38-54
        if not _canonical_find_index(pmodel):
            return self._decode_by_find_index(pmodel)
        sig = _table_of(pmodel)
        same = sig == self._sig
        used = self._bpos == len(self._buf)
        if same and not used:
            s = self._buf[self._bpos]
            self._bpos += 1
            self._taken += 1
            return int(s)
        if same and self._err:  # the reference panics / hangs at this symbol
            _decode_error(self._end, sig, self._err, f"decode (symbol {self._taken})")
        self._block = min(2 * self._block, self.MAX_BLOCK) if same and used else 1
        if used and self._bpos:  # (the block used up: its end state, as _here gives it, once)
            st = self._copy(self._end)
            st.flags = 0
        else:
            st = self._copy(self._here())
        n = self._block
        if self._limit is not None:
            n = max(1, min(n, self._limit - self._taken))
        start = self._copy(st)
        syms, fl = self._run(st, sig, n)
        self._start, self._end, self._buf, self._bpos = start, st, syms, 0
        self._sig, self._err = sig, fl
        if len(syms) == 0:
            _decode_error(st, sig, fl, f"decode (symbol {self._taken})")
        self._bpos = 1
        self._taken += 1
        return int(syms[0])

    def _decode_by_find_index(self, pmodel):
        """decoder.rs:38-54 with the caller's find_index: the index it returns at this state,
        then param_update and shift_left_buffer on the GPU (a one-entry table (c, cum) of that
        index, so the kernel's search has nothing to choose)."""
        st = self._copy(self._here())
        self._start, self._end, self._bpos = st, st, 0
        self._buf, self._sig, self._err = np.zeros(0, np.uint8), None, 0
        idx = int(pmodel.find_index(self))  # reads range_coder() / data(): the state st
        where = f"decode (symbol {self._taken})"
        sig = ((_u32(pmodel.c_freq(idx), "c_freq"),), (_u32(pmodel.cum_freq(idx), "cum_freq"),),
               _u32(pmodel.total_freq(), "total_freq"))
        nxt = self._copy(st)
        syms, fl = self._run(nxt, sig, 1)
        if len(syms) == 0:
            if fl & N.F_BAD_MODEL:
                _raise_bad_model(st.lower_bound, st.range, sig[0][0], sig[1][0], sig[2], where)
            _raise_for_flag(fl, where)
        self._start = self._end = nxt
        self._taken += 1
        return idx

    def range_coder(self):  # decoder.rs:24-26 (a snapshot)
        st = self._here()
        return RangeCoder(st.lower_bound, st.range)

    def data(self):  # decoder.rs:27-29
        return int(self._here().data)


def stream_states(n, device=None):
    """n fresh rc_stream_state on the device (RC_STREAM_STATE_INIT), as an int64 tensor of shape
    (n, 6): lower_bound, range, data, pos, n, flags | stage << 32."""
    torch = _torch()
    st = torch.zeros((n, 6), dtype=torch.int64, device=device or "cuda")
    st[:, 1] = -1  # range = u64::MAX
    return st


def stream_encode_batch(ctx, states, triples, sym_off, out, out_off, out_len=None, nbytes=None,
                        finish=False, flags=None):
    """rc_stream_encode on torch tensors (async on torch's current stream): n = states.shape[0]
    streams, triples uint32/int32 (3 per symbol), sym_off int64[n+1] indexing the triples, out
    uint8 with slots out_off int64[n+1].  Returns (out_len, flags)."""
    torch = _torch()
    n = states.shape[0]
    _check_dev(states, "states", (torch.int64,))
    _check_dev(triples, "triples", (torch.int32, torch.uint32))
    _check_dev(out, "out", (torch.uint8,))
    for name, t in (("sym_off", sym_off), ("out_off", out_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
        if t.numel() != n + 1:
            raise ValueError(f"{name} must have n_streams + 1 entries")
    if nbytes is not None:
        _check_dev(nbytes, "nbytes", (torch.uint8,))
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int64, device=states.device)
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=states.device)
    ctx.bind_stream()
    N.check(ctx._lib.rc_stream_encode(ctx.handle, _ptr(states), _ptr(triples), _ptr(sym_off), n,
                                      _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(nbytes),
                                      1 if finish else 0, _ptr(flags)), "rc_stream_encode")
    return out_len[:n], flags[:n]


def stream_decode_batch(ctx, c, cum, total, states, code, code_off, code_len, syms, sym_off,
                        flags=None):
    """rc_stream_decode on torch tensors: one (c, cum, total) table (uint32/int32 device
    tensors) for every stream's next sym_off[k+1] - sym_off[k] symbols.  Returns flags."""
    torch = _torch()
    n = states.shape[0]
    _check_dev(states, "states", (torch.int64,))
    for name, t in (("c", c), ("cum", cum)):
        _check_dev(t, name, (torch.int32, torch.uint32))
    _check_dev(code, "code", (torch.uint8,))
    _check_dev(syms, "syms", (torch.uint8,))
    for name, t in (("code_off", code_off), ("code_len", code_len), ("sym_off", sym_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=states.device)
    ctx.bind_stream()
    rc = ctx._lib.rc_stream_decode(ctx.handle, _ptr(c), _ptr(cum), c.numel(),
                                   ctypes.c_uint32(int(total) & 0xFFFFFFFF), _ptr(states),
                                   _ptr(code), _ptr(code_off), _ptr(code_len), _ptr(syms),
                                   _ptr(sym_off), n, _ptr(flags))
    N.check(rc, "rc_stream_decode")
    return flags[:n]


def _check_rows(c, cum, total, row_of):
    """The tensor checks of a row table and its per-symbol row indexes; returns (n_rows,
    n_symbols)."""
    torch = _torch()
    for name, t in (("c", c), ("cum", cum), ("total", total), ("row_of", row_of)):
        _check_dev(t, name, (torch.int32, torch.uint32))
    if c.dim() != 2 or cum.shape != c.shape:
        raise ValueError("c and cum must be 2-D (n_rows, n_symbols) tensors of one shape")
    if total.numel() != c.shape[0]:
        raise ValueError("total must have one entry per row")
    return int(c.shape[0]), int(c.shape[1])


def stream_decode_rows_batch(ctx, c, cum, total, row_of, states, code, code_off, code_len, syms,
                             sym_off, flags=None):
    """rc_stream_decode_rows on torch tensors: c, cum (n_rows, n_symbols) and total (n_rows)
    uint32/int32 device tensors, row_of one uint32/int32 row index per symbol, indexed like syms;
    the rest as stream_decode_batch.  Returns flags.

    The library picks one of two kernels with the same results, by the stream count against the
    device's CU count: one wave per stream (fewer than 16 streams per CU: a symbol's whole row
    read coalesced), or one lane per stream (only the row entries the search visits)."""
    torch = _torch()
    n = states.shape[0]
    n_rows, n_symbols = _check_rows(c, cum, total, row_of)
    _check_dev(states, "states", (torch.int64,))
    _check_dev(code, "code", (torch.uint8,))
    _check_dev(syms, "syms", (torch.uint8,))
    for name, t in (("code_off", code_off), ("code_len", code_len), ("sym_off", sym_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=states.device)
    ctx.bind_stream()
    rc = ctx._lib.rc_stream_decode_rows(ctx.handle, _ptr(c), _ptr(cum), _ptr(total), n_rows,
                                        n_symbols, _ptr(row_of), _ptr(states), _ptr(code),
                                        _ptr(code_off), _ptr(code_len), _ptr(syms), _ptr(sym_off),
                                        n, _ptr(flags))
    N.check(rc, "rc_stream_decode_rows")
    return flags[:n]


def stream_encode_rows_batch(ctx, c, cum, total, row_of, syms, states, sym_off, out, out_off,
                             out_len=None, nbytes=None, finish=False, flags=None):
    """rc_stream_encode_rows on torch tensors: the row table and row_of as in
    stream_decode_rows_batch, syms uint8 (one per symbol, indexed by sym_off); the rest as
    stream_encode_batch.  Returns (out_len, flags)."""
    torch = _torch()
    n = states.shape[0]
    n_rows, n_symbols = _check_rows(c, cum, total, row_of)
    _check_dev(states, "states", (torch.int64,))
    _check_dev(syms, "syms", (torch.uint8,))
    _check_dev(out, "out", (torch.uint8,))
    for name, t in (("sym_off", sym_off), ("out_off", out_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
        if t.numel() != n + 1:
            raise ValueError(f"{name} must have n_streams + 1 entries")
    if nbytes is not None:
        _check_dev(nbytes, "nbytes", (torch.uint8,))
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int64, device=states.device)
    if flags is None:
        flags = torch.empty(max(n, 1), dtype=torch.int32, device=states.device)
    ctx.bind_stream()
    rc = ctx._lib.rc_stream_encode_rows(ctx.handle, _ptr(c), _ptr(cum), _ptr(total), n_rows,
                                        n_symbols, _ptr(row_of), _ptr(syms), _ptr(states),
                                        _ptr(sym_off), n, _ptr(out), _ptr(out_off), _ptr(out_len),
                                        _ptr(nbytes), 1 if finish else 0, _ptr(flags))
    N.check(rc, "rc_stream_encode_rows")
    return out_len[:n], flags[:n]


def _u32_rows(a, name, dim):
    """a (tensor or array of non-negative integers below 2^32) as a contiguous uint32 numpy array"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != dim:
        raise ValueError(f"{name} must be {dim}-D")
    if a.dtype == np.int32:
        a = a.view(np.uint32)
    elif a.dtype != np.uint32:
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise BadModelError(f"{name}: entry outside 0..2^32 - 1")
        a = a.astype(np.uint32)
    return np.ascontiguousarray(a)


class RowTable:
    """n_rows tables of n_symbols (1..256) entries each, held in device memory, for the calls
    that code every symbol against a row of its own (rc_stream_decode_rows /
    rc_stream_encode_rows).  c, cum: (n_rows, n_symbols); total: (n_rows).  The tables are used
    as given (no consistency requirement, as with Decoder.decode's PModel)."""

    def __init__(self, c, cum, total, ctx=None):
        torch = _torch()
        self.ctx = ctx or default_context()
        c, cum, total = _u32_rows(c, "c", 2), _u32_rows(cum, "cum", 2), _u32_rows(total, "total", 1)
        if cum.shape != c.shape or total.shape[0] != c.shape[0]:
            raise ValueError("c and cum must have one shape, total one entry per row")
        if c.shape[0] < 1 or not 1 <= c.shape[1] <= 256:
            raise BadModelError("a row table has at least one row of 1..256 symbols")
        self.n_rows, self.n_symbols = int(c.shape[0]), int(c.shape[1])
        dev = torch.device("cuda", self.ctx.device)
        self.c, self.cum, self.total = (torch.from_numpy(a.view(np.int32)).to(dev)
                                        for a in (c, cum, total))

    @classmethod
    def from_counts(cls, counts, ctx=None):
        """Rows from symbol counts: cum by FreqTable.calc_cum's rule (sample_impl.rs:61-69), total
        the row's sum, which must fit 32 bits."""
        return cls(*cls.tables_from_counts(counts), ctx=ctx)

    @staticmethod
    def tables_from_counts(counts):
        """from_counts' (c, cum, total) as uint32 numpy arrays (host only)."""
        c = np.asarray(counts)
        if c.ndim != 2:
            raise ValueError("counts must be 2-D (n_rows, n_symbols)")
        if c.size and (c.min() < 0 or c.max() > 0xFFFFFFFF):
            raise BadModelError("counts: entry outside 0..2^32 - 1")
        c = c.astype(np.uint64)
        run = np.cumsum(c, axis=1, dtype=np.uint64)
        total = run[:, -1] if c.shape[1] else np.zeros(c.shape[0], np.uint64)
        if total.size and total.max() > 0xFFFFFFFF:
            raise BadModelError("counts: a row's total exceeds 2^32 - 1")
        cum = np.zeros_like(run)
        cum[:, 1:] = run[:, :-1]
        return c.astype(np.uint32), cum.astype(np.uint32), total.astype(np.uint32)


def _row_arrays(rows, lens):
    rows = [np.ascontiguousarray(_u32_rows(r, "rows", 1)) for r in rows]
    if [len(r) for r in rows] != list(lens):
        raise ValueError("rows must give one row index per symbol of every chunk")
    return rows


def encode_chunks_rows(table, chunks, rows, raise_on_error=True):
    """Encode a list of symbol sequences (bytes / uint8 arrays), symbol i of chunk k against row
    rows[k][i] of `table` (a RowTable): fresh streams, finished.  Returns a list of bytes."""
    torch = _torch()
    arrs = [_u8_chunk(c) for c in chunks]
    n = len(arrs)
    if n == 0:
        return []
    dev = torch.device("cuda", table.ctx.device)
    lens = np.array([len(a) for a in arrs], dtype=np.int64)
    rows = _row_arrays(rows, lens)
    sym_off = np.zeros(n + 1, dtype=np.int64)
    sym_off[1:] = np.cumsum(lens)
    out_off = np.zeros(n + 1, dtype=np.int64)
    out_off[1:] = np.cumsum([N.stream_max_bytes(L, True) for L in lens])
    out_d = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
    row_d = _to_dev([r.view(np.int32) for r in rows], sym_off[-1], dev)
    states = stream_states(n, dev)
    out_len, flags = stream_encode_rows_batch(
        table.ctx, table.c, table.cum, table.total, row_d, _to_dev(arrs, sym_off[-1], dev),
        states, torch.from_numpy(sym_off).to(dev), out_d, torch.from_numpy(out_off).to(dev),
        finish=True)
    fl, ol, host = flags.cpu().numpy(), out_len.cpu().numpy(), out_d.cpu().numpy()
    if raise_on_error:
        _raise_flagged(fl)
    return [bytes(host[out_off[k]: out_off[k] + ol[k]]) for k in range(n)]


def decode_chunks_rows(table, codes, rows, raise_on_error=True):
    """Decode a list of code streams, len(rows[k]) symbols each, symbol i of stream k against row
    rows[k][i] of `table`.  Returns a list of uint8 numpy arrays (a flagged stream's symbols
    before its error, when raise_on_error is false).  One launch: a wave per stream for a short
    list, a lane per stream from 16 streams per CU on (stream_decode_rows_batch)."""
    torch = _torch()
    n = len(codes)
    if n == 0:
        return []
    dev = torch.device("cuda", table.ctx.device)
    codes = [bytes(c) for c in codes]
    rows = _row_arrays(rows, [len(r) for r in rows])
    clen = np.array([len(c) for c in codes], dtype=np.int64)
    coff = np.zeros(n, dtype=np.int64)
    coff[1:] = np.cumsum(clen)[:-1]
    sym_off = np.zeros(n + 1, dtype=np.int64)
    sym_off[1:] = np.cumsum([len(r) for r in rows])
    code_d = torch.from_numpy(np.frombuffer(b"".join(codes) + b"\0", dtype=np.uint8).copy()).to(dev)
    syms_d = torch.zeros(max(int(sym_off[-1]), 1), dtype=torch.uint8, device=dev)
    states = stream_states(n, dev)
    flags = stream_decode_rows_batch(
        table.ctx, table.c, table.cum, table.total,
        _to_dev([r.view(np.int32) for r in rows], sym_off[-1], dev), states, code_d,
        torch.from_numpy(coff).to(dev), torch.from_numpy(clen).to(dev), syms_d,
        torch.from_numpy(sym_off).to(dev))
    fl, host = flags.cpu().numpy(), syms_d.cpu().numpy()
    got = states.cpu().numpy().view(np.uint64)[:, 4]
    if raise_on_error:
        _raise_flagged(fl)
    return [host[sym_off[k]: sym_off[k] + int(got[k])].copy() for k in range(n)]


# ----------------------------------------------------------------------------- host streaming
def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else ctypes.c_void_p(0)


def encode_host(model, syms, sym_off, out_off, out=None):
    """rc_encode_host: host-resident numpy arrays through the pipelined H2D / encode / D2H
    stream (rc_stream.hip).  Returns (out uint8[out_off[-1]], out_len uint64[n], flags
    uint32[n]); flags are returned, not raised.  out: optional caller buffer (e.g. a view of
    pinned memory, which skips the per-call page locking)."""
    syms = np.ascontiguousarray(syms, dtype=np.uint8)
    sym_off = np.ascontiguousarray(sym_off, dtype=np.uint64)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    n = len(sym_off) - 1
    if out is None:
        out = np.empty(int(out_off[-1]), np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < int(out_off[-1]):
        raise ValueError("out must be a contiguous uint8 array of out_off[-1] bytes")
    out_len = np.zeros(max(n, 1), np.uint64)
    flags = np.zeros(max(n, 1), np.uint32)
    ctx = model.ctx
    rc = ctx._lib.rc_encode_host(ctx.handle, model.handle, _np_ptr(syms), _np_ptr(sym_off), n,
                                 _np_ptr(out), _np_ptr(out_off), _np_ptr(out_len), _np_ptr(flags))
    if rc not in (N.RC_OK, N.RC_E_CHUNK):
        N.check(rc, "rc_encode_host")
    return out, out_len[:n], flags[:n]


def decode_host(model, code, code_off, code_len, sym_off, out=None):
    """rc_decode_host: the pipelined host path of decode_batch.  Returns (syms, flags).
    out: optional caller buffer for the symbols."""
    code = np.ascontiguousarray(code, dtype=np.uint8)
    code_off = np.ascontiguousarray(code_off, dtype=np.uint64)
    code_len = np.ascontiguousarray(code_len, dtype=np.uint64)
    sym_off = np.ascontiguousarray(sym_off, dtype=np.uint64)
    n = len(sym_off) - 1
    if out is None:
        syms = np.empty(int(sym_off[-1]), np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < int(sym_off[-1]):
        raise ValueError("out must be a contiguous uint8 array of sym_off[-1] bytes")
    else:
        syms = out
    flags = np.zeros(max(n, 1), np.uint32)
    ctx = model.ctx
    rc = ctx._lib.rc_decode_host(ctx.handle, model.handle, _np_ptr(code), _np_ptr(code_off),
                                 _np_ptr(code_len), _np_ptr(syms), _np_ptr(sym_off), n,
                                 _np_ptr(flags))
    if rc not in (N.RC_OK, N.RC_E_CHUNK):
        N.check(rc, "rc_decode_host")
    return syms, flags[:n]


# ----------------------------------------------------------------------------- several devices
def _handles(models):
    ctxs = (ctypes.c_void_p * len(models))(*[m.ctx.handle.value for m in models])
    hs = (ctypes.c_void_p * len(models))(*[m.handle.value for m in models])
    return ctxs, hs


def encode_host_multi(models, syms, sym_off, out_off, out=None):
    """rc_encode_host_multi: encode_host over several devices at once.  models: one model per
    device (context), e.g. [StaticModel(c, cum, total, ctx=Context(d)) for d in devices]; the
    chunks are split into contiguous ranges of about equal bytes, one per model.  Returns
    (out, out_len, flags) like encode_host."""
    if not models:
        raise ValueError("need at least one model")
    syms = np.ascontiguousarray(syms, dtype=np.uint8)
    sym_off = np.ascontiguousarray(sym_off, dtype=np.uint64)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    n = len(sym_off) - 1
    if out is None:
        out = np.empty(int(out_off[-1]), np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    flags = np.zeros(max(n, 1), np.uint32)
    ctxs, hs = _handles(models)
    rc = models[0].ctx._lib.rc_encode_host_multi(ctxs, hs, len(models), _np_ptr(syms),
                                                 _np_ptr(sym_off), n, _np_ptr(out),
                                                 _np_ptr(out_off), _np_ptr(out_len),
                                                 _np_ptr(flags))
    if rc not in (N.RC_OK, N.RC_E_CHUNK):
        N.check(rc, "rc_encode_host_multi")
    return out, out_len[:n], flags[:n]


def decode_host_multi(models, code, code_off, code_len, sym_off, out=None):
    """rc_decode_host_multi: decode_host over several devices at once.  Returns (syms, flags)."""
    if not models:
        raise ValueError("need at least one model")
    code = np.ascontiguousarray(code, dtype=np.uint8)
    code_off = np.ascontiguousarray(code_off, dtype=np.uint64)
    code_len = np.ascontiguousarray(code_len, dtype=np.uint64)
    sym_off = np.ascontiguousarray(sym_off, dtype=np.uint64)
    n = len(sym_off) - 1
    syms = np.empty(int(sym_off[-1]), np.uint8) if out is None else out
    flags = np.zeros(max(n, 1), np.uint32)
    ctxs, hs = _handles(models)
    rc = models[0].ctx._lib.rc_decode_host_multi(ctxs, hs, len(models), _np_ptr(code),
                                                 _np_ptr(code_off), _np_ptr(code_len),
                                                 _np_ptr(syms), _np_ptr(sym_off), n,
                                                 _np_ptr(flags))
    if rc not in (N.RC_OK, N.RC_E_CHUNK):
        N.check(rc, "rc_decode_host_multi")
    return syms, flags[:n]
