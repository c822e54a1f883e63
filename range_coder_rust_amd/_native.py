"""ctypes binding of librc_amd.so (the C ABI declared in include/range_coder.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950).
There is no CPU fallback: if the library is missing this module raises on first use.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RC_LIB_PATH") or os.path.join(_HERE, "librc_amd.so")

RC_OK = 0
RC_E_ARG = -1
RC_E_BAD_MODEL = -2
RC_E_DEVICE = -3
RC_E_NO_DEVICE = -4
RC_E_CHUNK = -5

F_ZERO_FREQ = 1
F_BAD_SYMBOL = 2
F_CAPACITY = 4
F_TRUNCATED = 8
F_CORRUPT = 16
F_TOO_LONG = 32
F_BAD_MODEL = 64
F_FINISHED = 128
MAX_CHUNK_SYMBOLS = 1 << 25  # RC_MAX_CHUNK_SYMBOLS

# every symbol include/range_coder.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "rc_ctx_create", "rc_ctx_destroy", "rc_ctx_set_stream", "rc_ctx_reset_stream",
    "rc_ctx_synchronize",
    "rc_status_string", "rc_last_error", "rc_device_info", "rc_model_create_static",
    "rc_model_create_adaptive", "rc_model_destroy", "rc_encode_batch", "rc_decode_batch", "rc_encode_host",
    "rc_decode_host", "rc_synth_fill", "rc_histogram", "rc_quantize_counts", "rc_ideal_bits",
    "rc_container_pack", "rc_container_info_parse", "rc_container_offsets",
    "rc_stream_encode", "rc_stream_decode", "rc_stream_encode_host", "rc_stream_decode_host",
    "rc_stream_decode_rows", "rc_stream_encode_rows",
    "rc_encode_host_multi", "rc_decode_host_multi",
    "rc_model_create_static_set", "rc_encode_batch_indexed", "rc_decode_batch_indexed",
    "rc_model_create_static_wide", "rc_encode_batch_wide", "rc_decode_batch_wide",
    "rc_quantize_counts_wide",
    "rc_model_create_order1_set", "rc_encode_batch_order1", "rc_decode_batch_order1",
    "rc_histogram_order1",
    "rc_histogram_wide", "rc_ideal_bits_wide",
    "rc_histogram_pairs", "rc_cluster_contexts", "rc_ideal_bits_order1",
    "rc_model_create_order1_set_periodic", "rc_histogram_pairs_periodic",
    "rc_checksum_batch", "rc_container2_info_parse", "rc_container2_pack",
    "rc_container2_offsets", "rc_container2_model", "rc_container2_verify",
    "rc_cluster_contexts_dev",
    "rc_model_create_static_wide16", "rc_encode_batch_wide16", "rc_decode_batch_wide16",
    "rc_quantize_counts_wide16",
    "rc_model_create_static_wide16_fine", "rc_quantize_counts_wide16_fine",
    "rc_model_create_order1_set_lagged", "rc_histogram_pairs_lagged",
    "rc_model_create_chunk_set", "rc_encode_batch_chunk_set", "rc_decode_batch_chunk_set",
    "rc_cost_table", "rc_chunk_set_costs", "rc_histogram_by_class",
)
MAX_SET_MODELS = 64  # RC_MAX_SET_MODELS
MAX_WIDE_SYMBOLS = 4096  # RC_MAX_WIDE_SYMBOLS
MAX_WIDE16_SYMBOLS = 65536  # RC_MAX_WIDE16_SYMBOLS
MAX_WIDE16_FINE_TOTAL = 1 << 24  # RC_MAX_WIDE16_FINE_TOTAL
RC_E_BAD_CONTAINER = -6
RC_E_CAPACITY = -7
RC_E_BAD_SYMBOL = -8
CONTAINER_HEADER_BYTES = 64


class ContainerInfo(ctypes.Structure):
    """rc_container_info (include/range_coder.h)."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("version", "kind", "n_symbols", "total_freq",
                                              "increment", "limit", "period", "reserved")] + \
               [(n, ctypes.c_uint64) for n in ("n_chunks", "n_syms", "payload_bytes", "table_off",
                                              "index_off", "payload_off", "container_bytes")]
Q_ALL_SYMBOLS = 1
RC_E_CHECKSUM = -9
CONTAINER2_F_CHECKSUMS = 1  # RC_CONTAINER2_F_CHECKSUMS


class Container2Info(ctypes.Structure):
    """rc_container2_info (include/range_coder.h): rc_container_info's fields, then RCB2's."""
    _fields_ = ContainerInfo._fields_ + \
               [(n, ctypes.c_uint32) for n in ("n_models", "first_row", "flags", "sym_bytes")] + \
               [("sum_off", ctypes.c_uint64)]


class StreamState(ctypes.Structure):
    """rc_stream_state (include/range_coder.h): one reference Encoder / Decoder between calls."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("lower_bound", "range", "data", "pos", "n")] + \
               [("flags", ctypes.c_uint32), ("stage", ctypes.c_uint32)]

    @classmethod
    def fresh(cls):  # RC_STREAM_STATE_INIT
        return cls(0, (1 << 64) - 1, 0, 0, 0, 0, 0)


def stream_max_bytes(n, finish):  # RC_STREAM_MAX_BYTES
    return 12 * int(n) + (8 if finish else 0)

_P = ctypes.c_void_p
_U32 = ctypes.c_uint32
_U64 = ctypes.c_uint64
_I = ctypes.c_int

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def load():
    """Load librc_amd.so (import torch first so the HIP runtime is shared with PyTorch)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:  # share libamdhip64.so.7 with torch when torch is present
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.rc_ctx_create.argtypes = [_I, ctypes.POINTER(_P)]
    L.rc_ctx_destroy.argtypes = [_P]
    L.rc_ctx_set_stream.argtypes = [_P, _P]
    L.rc_ctx_reset_stream.argtypes = [_P]
    L.rc_ctx_synchronize.argtypes = [_P]
    L.rc_status_string.argtypes = [_I]
    L.rc_status_string.restype = ctypes.c_char_p
    L.rc_last_error.argtypes = []
    L.rc_last_error.restype = ctypes.c_char_p
    L.rc_device_info.argtypes = [_I, ctypes.c_char_p, ctypes.c_size_t]
    L.rc_model_create_static.argtypes = [_P, _U32, _P, _P, _U32, ctypes.POINTER(_P)]
    L.rc_model_create_adaptive.argtypes = [_P, _U32, _U32, _U32, _U32, ctypes.POINTER(_P)]
    L.rc_model_destroy.argtypes = [_P]
    L.rc_encode_batch.argtypes = [_P, _P, _P, _P, _U32, _P, _P, _P, _P]
    L.rc_decode_batch.argtypes = [_P, _P, _P, _P, _P, _P, _P, _U32, _P]
    L.rc_encode_host.argtypes = [_P, _P, _P, _P, _U32, _P, _P, _P, _P]
    L.rc_decode_host.argtypes = [_P, _P, _P, _P, _P, _P, _P, _U32, _P]
    L.rc_synth_fill.argtypes = [_P, _U64, _P, _P, _U64, _U32]
    L.rc_histogram.argtypes = [_P, _P, _P, _U32, _P, _P]
    L.rc_quantize_counts.argtypes = [_P, _U32, _U64, _U32, _P, _P, _P]
    L.rc_ideal_bits.argtypes = [_P, _P, _U32, _U32, _P, _U32, _P]
    L.rc_container_pack.argtypes = [_P, _P, _P, _P, _P, _P, _U32, _P, _U64, ctypes.POINTER(_U64)]
    L.rc_container_info_parse.argtypes = [_P, _U64, ctypes.POINTER(ContainerInfo)]
    L.rc_container_offsets.argtypes = [_P, _P, ctypes.POINTER(ContainerInfo), _P, _P, _P]
    SP = ctypes.POINTER(StreamState)
    L.rc_stream_encode.argtypes = [_P, _P, _P, _P, _U32, _P, _P, _P, _P, _U32, _P]
    L.rc_stream_decode.argtypes = [_P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _U32, _P]
    L.rc_stream_decode_rows.argtypes = [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P,
                                        _U32, _P]
    L.rc_stream_encode_rows.argtypes = [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _P, _P,
                                        _P, _P, _U32, _P]
    L.rc_stream_encode_host.argtypes = [_P, SP, _P, _U64, _P, _U64, ctypes.POINTER(_U64), _P,
                                        _U32, ctypes.POINTER(_U32)]
    L.rc_stream_decode_host.argtypes = [_P, _P, _P, _U32, _U32, SP, _P, _U64, _P, _U64,
                                        ctypes.POINTER(_U32)]
    L.rc_encode_host_multi.argtypes = [_P, _P, _U32, _P, _P, _U32, _P, _P, _P, _P]
    L.rc_decode_host_multi.argtypes = [_P, _P, _U32, _P, _P, _P, _P, _P, _U32, _P]
    L.rc_model_create_static_set.argtypes = [_P, _U32, _U32, _P, _P, _U32, ctypes.POINTER(_P)]
    L.rc_encode_batch_indexed.argtypes = [_P, _P, _P, _P, _P, _U32, _P, _P, _P, _P]
    L.rc_decode_batch_indexed.argtypes = [_P, _P, _P, _P, _P, _P, _P, _P, _U32, _P]
    # host-only hooks of the model sets (not in the header; tests/test_model_set.py)
    L.rc_model_set_check_.argtypes = [_U32, _U32, _P, _P, _U32]
    L.rc_model_set_check_.restype = _I
    L.rc_model_set_plan_.argtypes = [_U32, _U32, _P]
    L.rc_model_set_plan_.restype = _I
    # host-only hook: the direct-table decoder's q-to-symbol table (tests/test_direct_table.py;
    # a library of an earlier revision, tools/build_rev.sh, has none)
    if hasattr(L, "rc_symof_table_"):
        L.rc_symof_table_.argtypes = [_U32, _P, _P, _U32, _P, _U32, ctypes.POINTER(_U32)]
        L.rc_symof_table_.restype = _I
    # host-only hooks of the single-table static models: the class of a table (9 words) and the
    # wide bucket decoder's table (tests/test_static_cases.py; an earlier revision has neither)
    if hasattr(L, "rc_model_static_plan_"):
        L.rc_model_static_plan_.argtypes = [_U32, _P, _P, _U32, _P]
        L.rc_model_static_plan_.restype = _I
        L.rc_bucket_table_.argtypes = [_U32, _P, _P, _U32, _P, _U32, ctypes.POINTER(_U32)]
        L.rc_bucket_table_.restype = _I
    # host-only hooks of rc_stream_decode_rows: the rule that picks its kernel, and a context's
    # choice (0 the rule, 1 wave per stream, 2 lane per stream; tests/test_rows_plan.py,
    # tools/kbench_rows.py; an earlier revision has neither)
    if hasattr(L, "rc_rows_decode_plan_"):
        L.rc_rows_decode_plan_.argtypes = [_U32, _U32, _U32]
        L.rc_rows_decode_plan_.restype = _I
        L.rc_rows_decoder_.argtypes = [_P, _U32]
        L.rc_rows_decoder_.restype = _I
    L.rc_model_create_static_wide.argtypes = [_P, _U32, _P, _P, _U32, ctypes.POINTER(_P)]
    L.rc_encode_batch_wide.argtypes = [_P, _P, _P, _P, _U32, _P, _P, _P, _P]
    L.rc_decode_batch_wide.argtypes = [_P, _P, _P, _P, _P, _P, _P, _U32, _P]
    L.rc_quantize_counts_wide.argtypes = [_P, _U32, _U64, _U32, _P, _P, _P]
    # host-only hooks of the wide models (not in the header; tests/test_wide_model.py)
    L.rc_model_wide_check_.argtypes = [_U32, _P, _P, _U32]
    L.rc_model_wide_check_.restype = _I
    L.rc_model_wide_plan_.argtypes = [_U32, _U32, _P]
    L.rc_model_wide_plan_.restype = _I
    L.rc_model_create_order1_set.argtypes = [_P, _U32, _U32, _P, _P, _U32, _P, _U32,
                                             ctypes.POINTER(_P)]
    L.rc_encode_batch_order1.argtypes = [_P, _P, _P, _P, _U32, _P, _P, _P, _P]
    L.rc_decode_batch_order1.argtypes = [_P, _P, _P, _P, _P, _P, _P, _U32, _P]
    L.rc_histogram_order1.argtypes = [_P, _U32, _P, _U32, _P, _P, _U32, _P]
    # host-only hooks of the order-1 sets (not in the header; tests/test_order1_model.py)
    L.rc_model_order1_check_.argtypes = [_U32, _U32, _P, _P, _U32, _P, _U32]
    L.rc_model_order1_check_.restype = _I
    L.rc_model_order1_plan_.argtypes = [_U32, _U32, _P]
    L.rc_model_order1_plan_.restype = _I
    # periodic order-1 sets (a library of an earlier revision has none of these)
    per = ("rc_model_create_order1_set_periodic", "rc_histogram_pairs_periodic")
    old3 = not hasattr(L, per[0])
    if not old3:
        L.rc_model_create_order1_set_periodic.argtypes = [_P, _U32, _U32, _P, _P, _U32, _U32, _P,
                                                          _U32, ctypes.POINTER(_P)]
        L.rc_histogram_pairs_periodic.argtypes = [_P, _U32, _P, _P, _U32, _P, _P]
        L.rc_model_order1_check_periodic_.argtypes = [_U32, _U32, _P, _P, _U32, _U32, _P, _U32]
        L.rc_model_order1_check_periodic_.restype = _I
        L.rc_model_order1_plan_periodic_.argtypes = [_U32, _U32, _U32, _P]
        L.rc_model_order1_plan_periodic_.restype = _I
    L.rc_histogram_wide.argtypes = [_P, _P, _P, _U32, _U32, _P, _P, _P]
    L.rc_ideal_bits_wide.argtypes = [_P, _P, _P, _P, _U32, _P]
    # fitting an order-1 set (a library of an earlier revision, tools/build_rev.sh, has none of
    # the three; using one of them with such a library raises AttributeError)
    fit = ("rc_histogram_pairs", "rc_cluster_contexts", "rc_ideal_bits_order1")
    old = not hasattr(L, fit[0])
    if not old:
        L.rc_histogram_pairs.argtypes = [_P, _P, _P, _U32, _P, _P]
        L.rc_cluster_contexts.argtypes = [_P, _P, _U32, _U32, _P, ctypes.POINTER(_U32),
                                          ctypes.POINTER(_U32), ctypes.POINTER(ctypes.c_double)]
        L.rc_ideal_bits_order1.argtypes = [_P, _P, _P, _P, _U32, _P]
    # RCB2 (a library of an earlier revision has none of these either)
    c2 = ("rc_checksum_batch", "rc_container2_info_parse", "rc_container2_pack",
          "rc_container2_offsets", "rc_container2_model", "rc_container2_verify")
    old2 = not hasattr(L, c2[0])
    if not old2:
        C2P = ctypes.POINTER(Container2Info)
        L.rc_checksum_batch.argtypes = [_P, _P, _P, _U32, _U32, _P]
        L.rc_container2_info_parse.argtypes = [_P, _U64, C2P]
        L.rc_container2_pack.argtypes = [_P, _P, _P, _P, _P, _P, _U32, _P, _P, _U64,
                                         ctypes.POINTER(_U64)]
        L.rc_container2_offsets.argtypes = [_P, _P, C2P, _P, _P, _P]
        L.rc_container2_model.argtypes = [_P, _P, C2P, ctypes.POINTER(_P)]
        L.rc_container2_verify.argtypes = [_P, _P, C2P, _P, _P, ctypes.POINTER(_U64)]
        # host-only hook: rc_checksum_batch with a given grid (tests/test_gpu_container2.py)
        L.rc_checksum_batch_grid_.argtypes = [_P, _P, _P, _U32, _U32, _P, _U32]
        L.rc_checksum_batch_grid_.restype = _I
    # host-only hook of the wide histogram (not in the header; tests/test_gpu_wide_build.py)
    L.rc_histogram_wide_copies_.argtypes = [_U32]
    L.rc_histogram_wide_copies_.restype = _U32
    # the joint device clustering (a library of an earlier revision has none)
    cj = ("rc_cluster_contexts_dev",)
    old4 = not hasattr(L, cj[0])
    if not old4:
        L.rc_cluster_contexts_dev.argtypes = [_P, _U32, _P, _P, _U32, _U32, _P,
                                              ctypes.POINTER(_U32), ctypes.POINTER(_U32),
                                              ctypes.POINTER(ctypes.c_double)]
    # lagged order-1 sets (a library of an earlier revision has none of these)
    lag = ("rc_model_create_order1_set_lagged", "rc_histogram_pairs_lagged")
    old5 = not hasattr(L, lag[0])
    if not old5:
        L.rc_model_create_order1_set_lagged.argtypes = [_P, _U32, _U32, _P, _P, _U32, _U32, _U32,
                                                        _P, _U32, ctypes.POINTER(_P)]
        L.rc_histogram_pairs_lagged.argtypes = [_P, _U32, _U32, _P, _P, _U32, _P, _P]
        L.rc_model_order1_check_lagged_.argtypes = [_U32, _U32, _P, _P, _U32, _U32, _U32, _P, _U32]
        L.rc_model_order1_check_lagged_.restype = _I
        L.rc_model_order1_plan_lagged_.argtypes = [_U32, _U32, _U32, _U32, _P]
        L.rc_model_order1_plan_lagged_.restype = _I
    # static chunk sets (a library of an earlier revision has none of these)
    cset = ("rc_model_create_chunk_set", "rc_encode_batch_chunk_set", "rc_decode_batch_chunk_set",
            "rc_cost_table", "rc_chunk_set_costs", "rc_histogram_by_class")
    old6 = not hasattr(L, cset[0])
    if not old6:
        L.rc_model_create_chunk_set.argtypes = [_P, _U32, _U32, _P, _P, _U32, ctypes.POINTER(_P)]
        L.rc_encode_batch_chunk_set.argtypes = [_P, _P, _P, _P, _P, _U32, _P, _P, _P, _P]
        L.rc_decode_batch_chunk_set.argtypes = [_P, _P, _P, _P, _P, _P, _P, _P, _U32, _P]
        L.rc_cost_table.argtypes = [_P, _U32, _U32, _P]
        L.rc_chunk_set_costs.argtypes = [_P, _P, _U32, _P, _U32, _P, _P, _P]
        L.rc_histogram_by_class.argtypes = [_P, _P, _P, _U32, _U32, _P]
        # host-only hooks (not in the header; tests/test_chunk_set.py): the constructor's
        # validation, its plan (10 words), the grouping rule, and the device grouping itself
        L.rc_chunk_set_check_.argtypes = [_U32, _U32, _P, _P, _U32]
        L.rc_chunk_set_check_.restype = _I
        L.rc_chunk_set_plan_.argtypes = [_U32, _U32, _P, _P, _U32, _P]
        L.rc_chunk_set_plan_.restype = _I
        L.rc_chunk_group_plan_.argtypes = [_P, _U32, _U32, _U32, _P, _P]
        L.rc_chunk_group_plan_.restype = _I
        L.rc_chunk_group_.argtypes = [_P, _P, _U32, _U32, _U32, _P, _P, _P]
        L.rc_chunk_group_.restype = _I
        L.rc_chunk_last_.argtypes = [_P, _P]
        L.rc_chunk_last_.restype = _I
    # wide16 static models (a library of an earlier revision has none of these)
    w16 = ("rc_model_create_static_wide16", "rc_encode_batch_wide16", "rc_decode_batch_wide16",
           "rc_quantize_counts_wide16")
    old7 = not hasattr(L, w16[0])
    if not old7:
        L.rc_model_create_static_wide16.argtypes = [_P, _U32, _P, _P, _U32, ctypes.POINTER(_P)]
        L.rc_encode_batch_wide16.argtypes = [_P, _P, _P, _P, _U32, _P, _P, _P, _P]
        L.rc_decode_batch_wide16.argtypes = [_P, _P, _P, _P, _P, _P, _P, _U32, _P]
        L.rc_quantize_counts_wide16.argtypes = [_P, _U32, _U64, _U32, _P, _P, _P]
        # host-only hooks (not in the header; tests/test_wide16_model.py, test_gpu_wide16.py):
        # the constructor's validation, the plan (8 words) and the lanes per workgroup of the
        # process's last wide16 encode and decode launch
        L.rc_model_wide16_check_.argtypes = [_U32, _P, _P, _U32]
        L.rc_model_wide16_check_.restype = _I
        L.rc_model_wide16_plan_.argtypes = [_U32, _U32, _P]
        L.rc_model_wide16_plan_.restype = _I
        L.rc_wide16_last_lanes_.argtypes = [_P]
        L.rc_wide16_last_lanes_.restype = None
    # wide16 fine models (a library of an earlier revision has none of these)
    w16f = ("rc_model_create_static_wide16_fine", "rc_quantize_counts_wide16_fine")
    old8 = not hasattr(L, w16f[0])
    if not old8:
        L.rc_model_create_static_wide16_fine.argtypes = [_P, _U32, _P, _P, _U32,
                                                         ctypes.POINTER(_P)]
        L.rc_quantize_counts_wide16_fine.argtypes = [_P, _U32, _U64, _U32, _P, _P, _P]
        # host-only hooks (not in the header; tests/test_wide16_fine_model.py,
        # test_gpu_wide16_fine.py): as the wide16 ones
        L.rc_model_wide16_fine_check_.argtypes = [_U32, _P, _P, _U32]
        L.rc_model_wide16_fine_check_.restype = _I
        L.rc_model_wide16_fine_plan_.argtypes = [_U32, _U32, _P]
        L.rc_model_wide16_fine_plan_.restype = _I
        L.rc_wide16_fine_last_lanes_.argtypes = [_P]
        L.rc_wide16_fine_last_lanes_.restype = None
    for name in EXPORTS:
        if name not in ("rc_status_string", "rc_last_error") and not (old and name in fit) \
                and not (old6 and name in cset) and not (old7 and name in w16) \
                and not (old8 and name in w16f) \
                and not (old2 and name in c2) and not (old3 and name in per) \
                and not (old4 and name in cj) and not (old5 and name in lag):
            getattr(L, name).restype = _I
    _lib = L
    return L


def status_string(code):
    return load().rc_status_string(code).decode()


class RCError(RuntimeError):
    def __init__(self, code, what):
        detail = load().rc_last_error().decode() if code == RC_E_DEVICE else ""
        super().__init__(f"{what}: {status_string(code)} ({code}) {detail}".rstrip())
        self.code = code


def check(code, what):
    if code != RC_OK:
        raise RCError(code, what)
    return code
