"""The chunked container "RCB1" (layout in include/range_coder.h).

The reference's stream holds neither its symbol count (examples/sample_impl.rs:113-120) nor
its model (decoder.rs:38); the container frames a batch of chunk streams with both, so

    blob = compress(data)          # data: uint8 HIP tensor -> container (uint8 HIP tensor)
    data == decompress(blob)

is a complete codec.  compress = GPU histogram + table (model_build) -> encode_batch ->
rc_container_pack; decompress = rc_container_info_parse -> model from the table ->
rc_container_offsets -> decode_batch, reading the payload in place.

"RCB2" is a second format beside it (same header file): it also frames an order-1 set or a wide
static model and may carry one 32-bit checksum of the decoded symbols per chunk.  compress
writes it when asked for something RCB1 cannot hold (order=1, 16-bit data, an Order1ModelSet or
WideStaticModel, checksum=True); decompress, info, model_of, offsets and pack look at the magic
or the model and take either.  RCB2 decompress = rc_container2_info_parse ->
rc_container2_model -> rc_container2_offsets -> the kind's decode call -> rc_container2_verify.
"""
import ctypes
import math

import numpy as np

from . import _native as N
from .api import (AdaptiveModel, Order1ModelSet, RangeCoderError, StaticModel, WideStaticModel,
                  _check_dev, _ptr, _raise_for_flag, _sym16, _torch, decode_batch,
                  decode_batch_order1, decode_batch_wide, default_context, encode_batch,
                  encode_batch_order1, encode_batch_wide, slot_capacity)
from .model_build import build_model, build_wide_model, fit_order1_set


class ContainerError(RangeCoderError):
    """A malformed or inconsistent container (RC_E_BAD_CONTAINER)."""


class ChecksumError(RangeCoderError):
    """The symbols decoded from an RCB2 container miss a chunk's stored checksum
    (RC_E_CHECKSUM).  `chunk` is the lowest such chunk."""

    def __init__(self, chunk):
        super().__init__(f"chunk {chunk}: decoded symbols do not match the stored checksum")
        self.chunk = chunk


def checksum_batch(data, sym_off, ctx=None):
    """rc_checksum_batch on torch tensors (async, torch's current stream): RCB2's checksum of
    every chunk [sym_off[k], sym_off[k+1]) of data (uint8, or uint16 / int16 symbols taken as
    two bytes each; offsets in symbols).  Returns an int32 tensor holding the n u32 sums' bits."""
    torch = _torch()
    wide = data.dtype != torch.uint8
    if wide:
        _sym16(data, "data")
    else:
        _check_dev(data, "data", (torch.uint8,))
    _check_dev(sym_off, "sym_off", (torch.int64, torch.uint64))
    ctx = ctx or default_context(data.device.index)
    n = sym_off.numel() - 1
    sums = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
    ctx.bind_stream()
    N.check(ctx._lib.rc_checksum_batch(ctx.handle, _ptr(data), _ptr(sym_off), n,
                                       2 if wide else 1, _ptr(sums)), "rc_checksum_batch")
    return sums[:n]


def _pack2(model, slots, slot_off, code_len, sym_off, sums):
    """rc_container2_pack: encoder slots (and checksums, or None) -> a new RCB2 container."""
    torch = _torch()
    n = sym_off.numel() - 1
    if sums is not None:
        _check_dev(sums, "sums", (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32")
                                                   else ()))
        if sums.numel() < n:
            raise ValueError("sums needs one checksum per chunk")
    ctx = model.ctx
    ctx.bind_stream()
    size = ctypes.c_uint64()
    # (a non-null sums pointer asks for the checksum section, also for a container of no chunks)
    psums = None if sums is None else ctypes.c_void_p(sums.data_ptr() or slots.data_ptr())
    args = (ctx.handle, model.handle, _ptr(slots), _ptr(slot_off), _ptr(code_len), _ptr(sym_off),
            n, psums)
    rc = ctx._lib.rc_container2_pack(*args, None, 0, ctypes.byref(size))
    if rc != N.RC_E_CAPACITY:
        N.check(rc, "rc_container2_pack (size)")
    dst = torch.empty(size.value, dtype=torch.uint8, device=slots.device)
    N.check(ctx._lib.rc_container2_pack(*args, _ptr(dst), dst.numel(), ctypes.byref(size)),
            "rc_container2_pack")
    return dst


def _refuse_period(model):
    """RCB2 frames one context map: a container of a periodic Order1ModelSet would silently drop
    the period (rc_container2_pack returns RC_E_ARG for one), so it is refused before any work."""
    if isinstance(model, Order1ModelSet) and model.period > 1:
        raise ValueError(f"a container cannot frame an Order1ModelSet with period "
                         f"{model.period}: keep the set beside the code, or use period 1")
    # (RCB2 has no field for a lag either: rc_container2_pack returns RC_E_ARG for lag > 1)
    if isinstance(model, Order1ModelSet) and model.lag > 1:
        raise ValueError(f"a container cannot frame an Order1ModelSet with lag {model.lag}: "
                         f"keep the set beside the code, or use lag 1")


def pack(model, slots, slot_off, code_len, sym_off, sums=None, rcb2=False):
    """rc_container_pack: encoder slots -> a new container tensor (uint8, same device).  With
    checksums (sums, from checksum_batch), an Order1ModelSet or WideStaticModel, or rcb2=True,
    the container is RCB2 (rc_container2_pack), else RCB1.  An Order1ModelSet with period > 1 is
    a ValueError."""
    _refuse_period(model)
    torch = _torch()
    _check_dev(slots, "slots", (torch.uint8,))
    for name, t in (("slot_off", slot_off), ("code_len", code_len), ("sym_off", sym_off)):
        _check_dev(t, name, (torch.int64, torch.uint64))
    if rcb2 or sums is not None or isinstance(model, (Order1ModelSet, WideStaticModel)):
        return _pack2(model, slots, slot_off, code_len, sym_off, sums)
    n = sym_off.numel() - 1
    ctx = model.ctx
    ctx.bind_stream()
    size = ctypes.c_uint64()
    rc = ctx._lib.rc_container_pack(ctx.handle, model.handle, _ptr(slots), _ptr(slot_off),
                                    _ptr(code_len), _ptr(sym_off), n, None, 0, ctypes.byref(size))
    if rc != N.RC_E_CAPACITY:
        N.check(rc, "rc_container_pack (size)")
    dst = torch.empty(size.value, dtype=torch.uint8, device=slots.device)
    N.check(ctx._lib.rc_container_pack(ctx.handle, model.handle, _ptr(slots), _ptr(slot_off),
                                       _ptr(code_len), _ptr(sym_off), n, _ptr(dst), dst.numel(),
                                       ctypes.byref(size)), "rc_container_pack")
    return dst


def info(container):
    """rc_container_info_parse of a container (tensor or bytes): a ContainerInfo; for an RCB2
    container rc_container2_info_parse and a Container2Info."""
    if isinstance(container, (bytes, bytearray, memoryview)):
        head = bytes(container[:N.CONTAINER_HEADER_BYTES])
    else:
        head = bytes(container[:N.CONTAINER_HEADER_BYTES].cpu().numpy())
    if head[:4] == b"RCB2":
        inf = N.Container2Info()
        rc = N.load().rc_container2_info_parse(ctypes.c_char_p(head), len(head),
                                               ctypes.byref(inf))
        if rc == N.RC_E_BAD_CONTAINER:
            raise ContainerError("malformed RCB2 container header")
        N.check(rc, "rc_container2_info_parse")
        return inf
    inf = N.ContainerInfo()
    rc = N.load().rc_container_info_parse(ctypes.c_char_p(head), len(head), ctypes.byref(inf))
    if rc == N.RC_E_BAD_CONTAINER:
        raise ContainerError("not an RCB1 container header")
    N.check(rc, "rc_container_info_parse")
    return inf


def _model_of2(container, inf, ctx):
    """rc_container2_model, its handle adopted by the Python model class of the kind (whose host
    arrays are filled from the table section the library has just validated)."""
    torch = _torch()
    _check_dev(container, "container", (torch.uint8,))
    if container.numel() < inf.index_off:
        raise ContainerError(f"container truncated: {container.numel()} bytes end inside the "
                             "table section")
    ctx.bind_stream()
    h = ctypes.c_void_p()
    rc = ctx._lib.rc_container2_model(ctx.handle, _ptr(container), ctypes.byref(inf),
                                      ctypes.byref(h))
    if rc == N.RC_E_BAD_CONTAINER:
        raise ContainerError("the container's model table is rejected (rows must sum to "
                             "total_freq, map entries must name rows)")
    N.check(rc, "rc_container2_model")
    n, k = inf.n_symbols, inf.n_models
    if inf.kind == 1:
        m = AdaptiveModel.__new__(AdaptiveModel)
        m.ctx, m.handle = ctx, h
        m.n_symbols, m.increment, m.limit, m.period = n, inf.increment, inf.limit, inf.period
        return m
    tab = container[inf.table_off:inf.index_off].cpu().numpy()
    rows = max(k, 1)
    c = tab[:4 * rows * n].view(np.uint32).reshape(rows, n).copy()
    cum = np.zeros_like(c)
    cum[:, 1:] = np.cumsum(c.astype(np.uint64), axis=1)[:, :-1].astype(np.uint32)
    if inf.kind == 2:
        m = Order1ModelSet.__new__(Order1ModelSet)
        m.c, m.cum, m.n_models = c, cum, k
        m.ctx_map = tab[4 * k * n:4 * k * n + n].copy()
        m.first_row, m.period, m.lag = inf.first_row, 1, 1
    else:
        cls = StaticModel if inf.kind == 0 else WideStaticModel
        m = cls.__new__(cls)
        m.c, m.cum = c[0], cum[0]
    m.total, m.n_symbols = inf.total_freq, n
    if inf.kind == 0:
        m.ctx, m.handle = ctx, h
    else:
        m._ctx, m._handle = ctx, h
    return m


def model_of(container, inf=None, ctx=None):
    """The container's model: a StaticModel from its c_freq table (cum by calc_cum) or an
    AdaptiveModel from its parameters; from an RCB2 container also an Order1ModelSet or a
    WideStaticModel (rc_container2_model)."""
    inf = inf or info(container)
    ctx = ctx or default_context(container.device.index)
    if isinstance(inf, N.Container2Info):
        return _model_of2(container, inf, ctx)
    if inf.kind == 1:
        return AdaptiveModel(inf.n_symbols, inf.increment, inf.limit, inf.period, ctx=ctx)
    tab = container[inf.table_off: inf.table_off + 4 * inf.n_symbols].cpu().numpy()
    c = tab.view(np.uint32).copy()
    if int(c.sum(dtype=np.uint64)) != inf.total_freq:
        raise ContainerError("table does not sum to the header's total_freq")
    try:
        return StaticModel(c, None, inf.total_freq, ctx=ctx)
    except ValueError as e:
        raise ContainerError(str(e)) from None


def offsets(container, inf=None, ctx=None):
    """rc_container_offsets: (code_off, code_len, sym_off) device tensors for decode_batch."""
    torch = _torch()
    _check_dev(container, "container", (torch.uint8,))
    inf = inf or info(container)
    if container.numel() < inf.container_bytes:
        raise ContainerError(f"container truncated: {container.numel()} of "
                             f"{inf.container_bytes} bytes")
    ctx = ctx or default_context(container.device.index)
    n = inf.n_chunks
    dev = container.device
    code_off = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    code_len = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    sym_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ctx.bind_stream()
    native = ("rc_container2_offsets" if isinstance(inf, N.Container2Info)
              else "rc_container_offsets")
    rc = getattr(ctx._lib, native)(ctx.handle, _ptr(container), ctypes.byref(inf),
                                   _ptr(code_off), _ptr(code_len), _ptr(sym_off))
    if rc == N.RC_E_BAD_CONTAINER:
        raise ContainerError("container index inconsistent with its header")
    N.check(rc, native)
    return code_off[:n], code_len[:n], sym_off


def compress(data, chunk_size=65536, model=None, target_total=1 << 16, ctx=None, order=0,
             n_models=8, checksum=False, n_symbols=None):
    """HIP tensor of symbols -> container (uint8 HIP tensor).

    With order=0, checksum=False, uint8 data and a model that is None (built on the GPU from the
    data's histogram, scaled to target_total with every symbol encodable), a StaticModel or an
    AdaptiveModel, the container is RCB1, byte for byte what this function always wrote.
    Anything else is written as RCB2:
      order=1, model None   an Order1ModelSet fitted to the data (fit_order1_set with at most
                            n_models context classes) and encode_batch_order1.  n_models
                            defaults to 8, not to the 64 a set may hold: more classes price the
                            data lower, but the order-1 decoder keeps one table per class on
                            chip and measured 287 Gsym/s at K = 8 against 37 at K = 64
                            (DESIGN.md §9.7); ask for more where size matters more than
                            decode speed.  Empty data has nothing to fit and is written with
                            the order-0 table (kind 0), as the order-0 path writes it.
      model                 an Order1ModelSet or a WideStaticModel is used as given (an
                            Order1ModelSet with period > 1 is a ValueError: the container has
                            no field for a period).
      uint16 / int16 data   16-bit symbols: model None builds a WideStaticModel over n_symbols
                            symbols (default: the data's largest symbol + 1; at most 4096).
      checksum=True         one checksum per chunk of the input (checksum_batch), which
                            decompress compares with the decoded symbols."""
    _refuse_period(model)
    torch = _torch()
    wide = data.dtype != torch.uint8 or isinstance(model, WideStaticModel)
    if wide:
        _sym16(data, "data")
    else:
        _check_dev(data, "data", (torch.uint8,))
    if order not in (0, 1):
        raise ValueError("order must be 0 or 1")
    o1 = isinstance(model, Order1ModelSet)
    if order == 1 and (wide or (model is not None and not o1)):
        raise ValueError("order=1 codes uint8 data with a fitted or given Order1ModelSet")
    if wide and model is not None and not isinstance(model, WideStaticModel):
        raise ValueError("16-bit data needs a WideStaticModel")
    ctx = ctx or default_context(data.device.index)
    n_sym = data.numel()
    n = (n_sym + chunk_size - 1) // chunk_size
    dev = data.device
    sym_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * chunk_size
    sym_off[-1] = n_sym
    if model is None and wide:
        if n_symbols is None:  # (int16 holds the symbols' bits: compare them as unsigned)
            n_symbols = (int(data.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).max())
                         if n_sym else 0) + 1
        model = build_wide_model(data, sym_off, n_symbols, target_total=target_total,
                                 all_symbols=True, ctx=ctx)
    elif model is None and order == 1 and n_sym:
        model = fit_order1_set(data, sym_off, n_models=n_models, target_total=target_total,
                               ctx=ctx)
        o1 = True
    elif model is None:
        model = build_model(data, sym_off, target_total=target_total, all_symbols=True, ctx=ctx)
    encode = encode_batch_wide if wide else encode_batch_order1 if o1 else encode_batch
    cap = slot_capacity(chunk_size, model.max_bits_per_symbol())
    slot_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
    slots = torch.empty(max(n * cap, 16), dtype=torch.uint8, device=dev)
    out_len, flags = encode(model, data, sym_off, slots, slot_off)
    if n:
        bad = flags[flags != 0]
        if bad.numel():
            _raise_for_flag(int(bad[0].item()), "compress")
    if order == 0 and not checksum and not wide and not o1:
        return pack(model, slots, slot_off, out_len, sym_off)
    sums = checksum_batch(data, sym_off, ctx=ctx) if checksum else None
    return _pack2(model, slots, slot_off, out_len, sym_off, sums)


def verify(container, inf, syms, sym_off, ctx=None):
    """rc_container2_verify: compare decoded symbols with an RCB2 container's checksums (no
    checksum section: nothing to compare).  Raises ChecksumError naming the lowest bad chunk."""
    ctx = ctx or default_context(container.device.index)
    ctx.bind_stream()
    bad = ctypes.c_uint64()
    rc = ctx._lib.rc_container2_verify(ctx.handle, _ptr(container), ctypes.byref(inf),
                                       _ptr(syms), _ptr(sym_off), ctypes.byref(bad))
    if rc == N.RC_E_CHECKSUM:
        raise ChecksumError(int(bad.value))
    N.check(rc, "rc_container2_verify")


def decompress(container, ctx=None):
    """Container (uint8 HIP tensor; RCB1 or RCB2 by its magic) -> the original tensor: uint8, or
    uint16 for an RCB2 container of a wide model.  An RCB2 container with checksums is verified:
    ChecksumError when the decoded symbols of a chunk miss its checksum."""
    torch = _torch()
    _check_dev(container, "container", (torch.uint8,))
    ctx = ctx or default_context(container.device.index)
    inf = info(container)
    model = model_of(container, inf, ctx)
    code_off, code_len, sym_off = offsets(container, inf, ctx)
    rcb2 = isinstance(inf, N.Container2Info)
    decode, dtype = decode_batch, torch.uint8
    if rcb2 and inf.kind == 2:
        decode = decode_batch_order1
    elif rcb2 and inf.kind == 3:
        decode, dtype = decode_batch_wide, getattr(torch, "uint16", torch.int16)
    out = torch.empty(max(inf.n_syms, 1), dtype=dtype, device=container.device)
    flags = decode(model, container, code_off, code_len, out, sym_off)
    if inf.n_chunks:
        bad = flags[flags != 0]
        if bad.numel():
            _raise_for_flag(int(bad[0].item()), "decompress")
    if rcb2:
        verify(container, inf, out, sym_off, ctx)
    return out[:inf.n_syms]
