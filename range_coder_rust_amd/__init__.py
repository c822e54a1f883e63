"""range_coder_rust_amd — MI355X-native batched range coder (drop-in for the encode/decode path
of diegodox/range_coder_rust).  See DESIGN.md and include/range_coder.h."""
from .api import (  # noqa: F401
    ADAPTIVE_DEFAULTS, AdaptiveModel, BadSymbolError, CapacityError, ChunkTooLongError, Context, CorruptStreamError, Decoder, Encoder, FreqTable,
    PModel, RangeCoderError, StaticModel, TruncatedStreamError, ZeroFrequencyError,
    decode_batch, decode_chunks, default_context, encode_batch, encode_chunks, flag_names,
    slot_capacity, encode_host, decode_host, BadModelError, ByteCount, FinishedError, RangeCoder,
    LowerBoundOverflow, UpperBoundOverflow,
    stream_states, stream_encode_batch, stream_decode_batch, encode_host_multi, decode_host_multi,
    StaticModelSet, encode_batch_indexed, decode_batch_indexed, encode_chunks_indexed,
    decode_chunks_indexed,
    WideStaticModel, encode_batch_wide, decode_batch_wide, encode_chunks_wide,
    decode_chunks_wide,
    Wide16StaticModel, Wide16FineModel, encode_batch_wide16, decode_batch_wide16, encode_chunks_wide16,
    decode_chunks_wide16,
    Order1ModelSet, encode_batch_order1, decode_batch_order1, encode_chunks_order1,
    decode_chunks_order1,
    RowTable, stream_decode_rows_batch, stream_encode_rows_batch, encode_chunks_rows,
    decode_chunks_rows,
    ChunkModelSet, encode_batch_chunk_set, decode_batch_chunk_set, encode_chunks_chunk_set,
    decode_chunks_chunk_set,
)
from . import synth  # noqa: F401
from .model_build import build_model, histogram, ideal_bits, quantize_counts, quantize_counts_wide  # noqa: F401
from .model_build import build_order1_set, histogram_order1  # noqa: F401
from .model_build import build_wide_model, histogram_wide, ideal_bits_wide  # noqa: F401
from .model_build import build_wide16_model, histogram16, quantize_counts_wide16  # noqa: F401
from .model_build import quantize_counts_wide16_fine  # noqa: F401
from .model_build import (cluster_contexts, cluster_contexts_joint, fit_order1_set,  # noqa: F401
                          histogram_pairs, histogram_pairs_periodic, ideal_bits_order1)
from .model_build import (chunk_set_costs, cost_table, fit_chunk_set,  # noqa: F401
                          histogram_by_class)
from . import container  # noqa: F401
from .container import (ChecksumError, ContainerError, checksum_batch, compress,  # noqa: F401
                        decompress)

__version__ = "0.1.0"
