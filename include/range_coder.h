/*
 * range_coder.h — C ABI of the MI355X-native batched range coder (librc_amd.so).
 *
 * Drop-in boundary for the encode/decode hot path of diegodox/range_coder_rust.  The reference
 * exposes a per-stream, per-symbol Rust API (src/lib.rs:1-13):
 *     Encoder::new / encode<T: PModel>(&T, usize) -> u32 / finish() -> VecDeque<u8>
 *         (src/encoder.rs:14-46)
 *     Decoder::new(code) / decode<T: PModel>(&T) -> usize      (src/decoder.rs:14-54)
 *     trait PModel { c_freq, cum_freq, total_freq, find_index } (src/pmodel.rs:4-12)
 * Each of these entry points replaces the reference's per-symbol loops over many independent
 * streams ("chunks", one fresh Encoder/Decoder each) with one kernel launch.  The emitted bytes
 * of every chunk are bit-identical to Encoder::encode* + Encoder::finish on the same symbols.
 *
 * Conventions
 *  - Plain pointers and sizes only.  "dev" pointers are HIP device (or managed) memory; "host"
 *    pointers are ordinary host memory.  No exceptions or panics cross this boundary.
 *  - Every function returns an rc_status (RC_OK == 0).  Data-dependent problems of a single
 *    chunk are reported per chunk in a uint32 flags array (RC_F_*), never by aborting.
 *  - Batch calls are asynchronous and stream-ordered on the context's stream.
 *  - Offsets: chunk k's symbols are sym[sym_off[k] .. sym_off[k+1]) (n_chunks+1 entries,
 *    non-decreasing, any alignment).  Encoder output slot k is out[out_off[k] .. out_off[k+1]).
 *    Offsets are full 64-bit element indices (symbols, rows, triples or bytes, as the call
 *    says); arenas beyond 4 GiB, with byte offsets and element indices past 2^32, are covered
 *    by the suite for every batch call (tests/test_gpu_high_offsets.py).
 */
#ifndef RANGE_CODER_AMD_H
#define RANGE_CODER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (function results) ---- */
typedef int rc_status;
#define RC_OK 0
#define RC_E_ARG (-1)       /* null handle/pointer, n_chunks too large, bad parameter */
#define RC_E_BAD_MODEL (-2) /* frequency table rejected (see rc_model_create_static) */
#define RC_E_DEVICE (-3)    /* HIP runtime error (launch, allocation, copy) */
#define RC_E_NO_DEVICE (-4) /* no gfx950 device visible / device index out of range */
#define RC_E_CHUNK (-5)     /* synchronous helpers only: at least one chunk has a flag set */
#define RC_E_BAD_CONTAINER (-6) /* container header / index malformed or inconsistent */
#define RC_E_CAPACITY (-7)  /* destination buffer too small (the needed size is reported) */
#define RC_E_BAD_SYMBOL (-8) /* counts name a symbol outside the alphabet (rc_cluster_contexts) */
#define RC_E_CHECKSUM (-9)  /* decoded symbols miss a chunk's checksum (rc_container2_verify) */

/* ---- per-chunk flags (bitwise; the first error of a chunk wins) ----
 * Where the reference panics or never terminates, the kernels flag the chunk instead.      */
#define RC_F_ZERO_FREQ 1u  /* encode of a symbol with c_freq == 0: the reference loops forever
                              in no_carry_expansion (range_coder.rs:83-85, 110-116)          */
#define RC_F_BAD_SYMBOL 2u /* symbol index >= n_symbols: the reference panics
                              (examples/sample_impl.rs:19, Vec::get().unwrap())              */
#define RC_F_CAPACITY 4u   /* encoded chunk longer than its output slot; out_len[k] still holds
                              the exact length so the caller can retry with a larger slot   */
#define RC_F_TRUNCATED 8u  /* decoder needed a byte past code_len: the reference panics
                              (decoder.rs:33, pop_front().unwrap())                         */
#define RC_F_CORRUPT 16u   /* decoder selected a c_freq == 0 symbol (only possible on corrupt
                              input): the reference loops forever                            */
#define RC_F_BAD_MODEL 64u /* stream API: a (c, cum, total) on which the reference panics — total
                              0 (u64 division by zero, range_coder.rs:38-40), LowerBoundOverflow
                              (:68-81) or UpperBoundOverflow (upper_bound().unwrap(), :138-146);
                              indexed batch calls (rc_*_batch_indexed): a model index >= the
                              set's n_models (the caller's models[idx] would panic)          */
#define RC_F_FINISHED 128u /* stream API: encode after Encoder::finish, which consumes the
                              encoder (encoder.rs:40)                                        */
#define RC_F_TOO_LONG 32u  /* chunk of more than RC_MAX_CHUNK_SYMBOLS symbols: the batch kernels
                              keep 32-bit in-chunk stream positions, so such a chunk is neither
                              read nor written (out_len 0).  The reference has no limit
                              (VecDeque, encoder.rs:7-11): code a longer stream with the
                              resumable stream entry points (rc_stream_*), which have none    */

/* Longest chunk of the batch entry points.  A symbol settles at most 12 code bytes (5 in
 * no_carry_expansion, range_coder.rs:110-116, and 7 in range_reduction_expansion, :126-135;
 * DESIGN.md §3), so 2^25 symbols stay below 2^29 code bytes = 2^32 bits. */
#define RC_MAX_CHUNK_SYMBOLS (1ull << 25)

/* Maximum chunks per batch call (grid limit) */
#define RC_MAX_CHUNKS (1u << 28)

typedef struct rc_ctx rc_ctx;     /* one device + one stream; use one per host thread */

/* Environment.  rc_ctx_create reads these switches once and the context keeps them; nothing
 * reads the environment per launch or per call (changing a variable affects contexts created
 * after the change only).  Unset is the default.
 *   RC_PRIO=off             wave priorities off (every launch oldest-first)
 *   RC_DEC_PAIR=512|1024    decode 2^15 < total <= 2^16 static models with the pair-bucket
 *                           decoder in workgroups of that size (measurements; slower)
 *   RC_DEC_PAIR=6           decode every 2048 < total <= 2^16 static model through the direct
 *                           q-to-symbol table (1,024-lane workgroups) at every launch size
 *   RC_DEC_PAIR=4           decode them through the bucket table at every launch size (unset:
 *                           chosen per launch from its chunk count and the device's CU count)
 *   RC_STREAM_SERVICE=0     per-call stream entry points launch a kernel per call instead of
 *                           using the stream-service wave
 *   RC_STREAM_DMA=1         host pipeline (rc_*_host): every transfer by DMA engine copies
 *   RC_STREAM_DIRECT=0      host pipeline: stage outputs in HBM instead of writing them into
 *                           mapped host memory from the kernel
 *   RC_STREAM_BATCH_BYTES=n host pipeline batch size in input bytes (default 2 GiB)
 *   RC_HIST_HOT=0           rc_histogram without its ballot-counted most frequent symbol */
typedef struct rc_model rc_model; /* device-resident snapshot of a PModel */

/* ---- context ---- */
rc_status rc_ctx_create(int device, rc_ctx** out);
rc_status rc_ctx_destroy(rc_ctx* ctx);
/* Launch on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL is the HIP null (legacy default) stream.  rc_ctx_reset_stream returns to the
 * context's own non-blocking stream. */
rc_status rc_ctx_set_stream(rc_ctx* ctx, void* hip_stream);
rc_status rc_ctx_reset_stream(rc_ctx* ctx);
rc_status rc_ctx_synchronize(rc_ctx* ctx);
const char* rc_status_string(rc_status s);
/* Text of the last HIP runtime error seen by this thread ("" if none) */
const char* rc_last_error(void);
/* Library / device info: writes a short NUL-terminated description (arch, CUs) */
rc_status rc_device_info(int device, char* buf, size_t buf_len);

/* ---- models (the PModel plug-in point, pmodel.rs:4-12) ----
 * Static model: a snapshot of PModel::c_freq(i), cum_freq(i) (i < n_symbols) and total_freq().
 * Accepted when 1 <= n_symbols <= 256, total_freq >= 1, cum_freq[0] == 0,
 * cum_freq[i+1] == cum_freq[i] + c_freq[i] and cum_freq[n-1] + c_freq[n-1] == total_freq
 * (the tables FreqTable::calc_cum builds, sample_impl.rs:61-69).  The decoder then uses the
 * canonical inverse cum[s] <= rfreq < cum[s+1] — exactly FreqTable::find_index
 * (sample_impl.rs:27-45), including its choice of n_symbols-1 when rfreq >= total.
 * Zero-frequency symbols are allowed in the table (they are just never encodable).       */
rc_status rc_model_create_static(rc_ctx* ctx, uint32_t n_symbols, const uint32_t* c_freq_host,
                                 const uint32_t* cum_freq_host, uint32_t total_freq,
                                 rc_model** out);
/* Adaptive order-0 model (build-defined; the reference ships none).
 * Per chunk, c[i] = 1 for i < n_symbols.  After coding the i-th symbol s (0-based):
 * c[s] += increment, and if (i + 1) % period == 0 and the total exceeds limit, every
 * c[i] = (c[i] + 1) >> 1.  The coder sees (c[s], cum[s], total) before the update.
 * Accepted when 1 <= n_symbols <= 256, increment >= 1, period is a power of two <= 65536 and
 * n_symbols + increment*period <= limit <= 65535 - increment*period (so the total, and every
 * count, stays below 2^16 for all inputs).  Default (config C4): increment 32, limit 57343,
 * period 256.                                                                               */
rc_status rc_model_create_adaptive(rc_ctx* ctx, uint32_t n_symbols, uint32_t increment,
                                   uint32_t limit, uint32_t period, rc_model** out);
rc_status rc_model_destroy(rc_model* m);

/* ---- batch encode (replaces n_chunks x {Encoder::new; encode...; finish}) ----
 * syms_dev      symbol bytes (index < n_symbols), chunk k = [sym_off[k], sym_off[k+1])
 * sym_off_dev   n_chunks+1 offsets into syms_dev
 * out_dev       output arena; chunk k's stream is written at out_off[k], capacity
 *               out_off[k+1]-out_off[k] bytes (any alignment; 16-B aligned is fastest)
 * out_len_dev   n_chunks: exact stream length (== 8 + sum of encode() return values);
 *               slot bytes past out_len are unspecified, nothing outside the slot is written
 * flags_dev     n_chunks: RC_F_* (0 == success)                                         */
rc_status rc_encode_batch(rc_ctx* ctx, const rc_model* m, const uint8_t* syms_dev,
                          const uint64_t* sym_off_dev, uint32_t n_chunks, uint8_t* out_dev,
                          const uint64_t* out_off_dev, uint64_t* out_len_dev,
                          uint32_t* flags_dev);

/* ---- batch decode (replaces n_chunks x {Decoder::new(code); n x decode}) ----
 * code_dev      code arena; chunk k's stream = code[code_off[k] .. code_off[k]+code_len[k])
 * code_off_dev, code_len_dev   n_chunks entries each
 * syms_out_dev  decoded symbols; chunk k gets sym_off[k+1]-sym_off[k] symbols (the count is
 *               out-of-band, as in the reference: sample_impl.rs:113-120)
 * flags_dev     n_chunks: RC_F_* (0 == success)                                         */
rc_status rc_decode_batch(rc_ctx* ctx, const rc_model* m, const uint8_t* code_dev,
                          const uint64_t* code_off_dev, const uint64_t* code_len_dev,
                          uint8_t* syms_out_dev, const uint64_t* sym_off_dev, uint32_t n_chunks,
                          uint32_t* flags_dev);

/* ---- static model sets: a model chosen per symbol (encoder.rs:24-37, decoder.rs:38-54) ----
 * The reference takes the model on EVERY call, so a caller may code each symbol against another
 * table (context modelling; side information that picks one of a few quantised CDFs).  A static
 * model set holds n_models static tables over one alphabet and one total_freq, and the indexed
 * batch calls take one model index per symbol: symbol i of chunk k is coded exactly as
 * encoder.encode(&models[idx[i]], sym[i]) and decoded exactly as decoder.decode(&models[idx[i]])
 * with FreqTable::find_index over that row (including its choice of n_symbols-1 when rfreq >=
 * total).  Bytes, lengths and flags are bit-identical to the reference arithmetic.
 *
 * Accepted when 1 <= n_models <= RC_MAX_SET_MODELS, 1 <= n_symbols <= 256, 256 <= total_freq <=
 * 65536 (a power of two or not) and every row (c_freq_host / cum_freq_host: n_models x n_symbols,
 * row-major) passes rc_model_create_static's checks against the shared total_freq; anything else
 * is RC_E_BAD_MODEL.  Zero-frequency symbols are allowed in a row.  The total is shared and
 * bounded because that is the small-model regime of the coders: range / total is
 * then computed once per symbol whatever the row, the decoder's carried hint scale does not
 * depend on the row, and at most 3 bytes settle per symbol, so the margins of both kernels'
 * rings hold unchanged.  (Rows with different totals: rescale them, rc_quantize_counts.)
 *
 * A set is its own kind of rc_model: the indexed calls take nothing else (RC_E_ARG for a static
 * or adaptive model), and every other entry point that takes a model returns RC_E_ARG for a set.
 * Destroy it with rc_model_destroy.                                                          */
#define RC_MAX_SET_MODELS 64u
rc_status rc_model_create_static_set(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                     const uint32_t* c_freq_host,   /* n_models x n_symbols */
                                     const uint32_t* cum_freq_host, /* likewise */
                                     uint32_t total_freq, rc_model** out);
/* rc_encode_batch with a model index per symbol.
 * idx_dev       one byte per symbol, indexed exactly like the symbols: idx[sym_off[k] + i] is
 *               the row of symbol i of chunk k.  Any alignment works; fastest when idx_dev is
 *               congruent to syms_dev modulo 16.
 * flags_dev     as rc_encode_batch (RC_F_ZERO_FREQ and RC_F_BAD_SYMBOL against the symbol's own
 *               row, RC_F_CAPACITY with the exact length, RC_F_TOO_LONG), and RC_F_BAD_MODEL for
 *               an index >= n_models; the first error of a chunk wins (at one symbol the index
 *               is looked at first).  After a flag the chunk's remaining output is unspecified;
 *               a flagged chunk never reads or writes outside its slots.
 * Asynchronous and stream-ordered on the context's stream, like rc_encode_batch.           */
rc_status rc_encode_batch_indexed(rc_ctx* ctx, const rc_model* set, const uint8_t* syms_dev,
                                  const uint8_t* idx_dev, const uint64_t* sym_off_dev,
                                  uint32_t n_chunks, uint8_t* out_dev, const uint64_t* out_off_dev,
                                  uint64_t* out_len_dev, uint32_t* flags_dev);
/* rc_decode_batch with a model index per symbol (side information, known before decoding).
 * idx_dev       as above, indexed like syms_out_dev; fastest when congruent to it modulo 16
 * flags_dev     as rc_decode_batch (RC_F_TRUNCATED, RC_F_CORRUPT, RC_F_TOO_LONG), and
 *               RC_F_BAD_MODEL for an index >= n_models; the first error of a chunk wins.
 * Over-read: the code of a chunk is fetched in whole 64-B aligned segments of the address space,
 * so up to 63 bytes before code_off[k] and after code_off[k] + code_len[k] may be READ (never
 * beyond the aligned segment that holds the stream's first or last byte, hence never from an
 * unmapped page); bytes past the end are consumed only by a decode that is flagged
 * RC_F_TRUNCATED.  rc_decode_batch reads the same way.  Indexes and symbols are touched inside
 * [sym_off[k], sym_off[k+1]) only.                                                          */
rc_status rc_decode_batch_indexed(rc_ctx* ctx, const rc_model* set, const uint8_t* code_dev,
                                  const uint64_t* code_off_dev, const uint64_t* code_len_dev,
                                  const uint8_t* idx_dev, uint8_t* syms_out_dev,
                                  const uint64_t* sym_off_dev, uint32_t n_chunks,
                                  uint32_t* flags_dev);

/* ---- static chunk sets: a model chosen per chunk ----
 * A batch is often a mixture (weights beside indices, text beside binary), which one pooled
 * table prices badly.  A chunk set holds n_models static tables over one alphabet and one
 * total_freq, and the chunk-set batch calls take one class per CHUNK: chunk k is coded exactly as
 * rc_encode_batch / rc_decode_batch code it with rc_model_create_static(row class_of[k]) --
 * bytes, out_len, flags, the capacity rule and RC_F_TOO_LONG, and for the decoder garbage and
 * truncated streams judged against that row.  The launch is sorted by class on the device, every
 * workgroup stages one row and runs the single-table symbol step, so
 * the cost over the single-table calls is the sort and at most n_models partly filled workgroups.
 *
 * Accepted inputs are exactly rc_model_create_static_set's (1 <= n_models <= RC_MAX_SET_MODELS,
 * 1 <= n_symbols <= 256, 256 <= total_freq <= 65536 shared by the rows, every row passing
 * rc_model_create_static's checks); anything else is RC_E_BAD_MODEL.  A chunk set is its own kind
 * of rc_model: the chunk-set calls take nothing else (RC_E_ARG), and every other entry point that
 * takes a model returns RC_E_ARG for a chunk set.  Destroy it with rc_model_destroy.  A set and
 * its class_of travel beside the code: the containers do not carry them.                      */
rc_status rc_model_create_chunk_set(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                    const uint32_t* c_freq_host,   /* n_models x n_symbols */
                                    const uint32_t* cum_freq_host, /* likewise */
                                    uint32_t total_freq, rc_model** out);
/* rc_encode_batch with a row per chunk.
 * class_of_dev  one byte per chunk: the row of chunk k.  class_of[k] >= n_models gives that chunk
 *               RC_F_BAD_MODEL and out_len 0; its slot is not written and its symbols are not
 *               read, and every other chunk is unaffected.
 * Everything else as rc_encode_batch with that row's static model.  Asynchronous and
 * stream-ordered on the context's stream; nothing synchronises with the host.  The context keeps
 * the launch's grouping in a scratch buffer of its own, which grows in stream order; a call on
 * another stream than the context's last chunk-set call waits on the device for that call's
 * coder before it regroups, so a context may change streams between calls (rc_ctx_set_stream).
 * As with every entry point, one context is used by one host thread at a time.               */
rc_status rc_encode_batch_chunk_set(rc_ctx* ctx, const rc_model* set,
                                    const uint8_t* class_of_dev, const uint8_t* syms_dev,
                                    const uint64_t* sym_off_dev, uint32_t n_chunks,
                                    uint8_t* out_dev, const uint64_t* out_off_dev,
                                    uint64_t* out_len_dev, uint32_t* flags_dev);
/* rc_decode_batch with a row per chunk (side information, known before decoding).
 * class_of_dev  as above; class_of[k] >= n_models gives that chunk RC_F_BAD_MODEL, and its
 *               symbols are not written.
 * Everything else, the over-read of the code included, as rc_decode_batch with that row's static
 * model.                                                                                     */
rc_status rc_decode_batch_chunk_set(rc_ctx* ctx, const rc_model* set,
                                    const uint8_t* class_of_dev, const uint8_t* code_dev,
                                    const uint64_t* code_off_dev, const uint64_t* code_len_dev,
                                    uint8_t* syms_out_dev, const uint64_t* sym_off_dev,
                                    uint32_t n_chunks, uint32_t* flags_dev);
/* Fitting the classes of a chunk set.  Costs are integers in units of 2^-16 bit, so every result
 * is exact.
 * rc_cost_table (host only): cost_out_host[s] = round(65536 * log2(total_freq / c_freq[s])), and
 * RC_COST_NONE where c_freq[s] == 0 (the row cannot code s).  RC_E_ARG: a null pointer,
 * n_symbols outside 1..256, total_freq == 0, a c_freq above total_freq.                      */
#define RC_COST_NONE 0xFFFFFFFFu
rc_status rc_cost_table(const uint32_t* c_freq_host, uint32_t n_symbols, uint32_t total_freq,
                        uint32_t* cost_out_host /* n_symbols */);
/* The cost of every chunk under every row, and the cheapest row.
 * chunk_hist_dev  n_chunks x 256 counts, rc_histogram's rows (16-byte aligned)
 * cost_host       n_models x 256 entries, taken as given (rc_cost_table's; entries past a row's
 *                 alphabet: RC_COST_NONE)
 * best_row_dev    n_chunks bytes: the row of the least cost, ties to the lowest row
 * best_cost_dev   n_chunks x u64: that cost
 * costs_dev       NULL, or n_chunks x n_models u64: every cost
 * The cost of chunk k under row r is the sum over s of hist[k][s] * cost[r][s] in 64 bits, and
 * UINT64_MAX if the chunk counts a symbol whose entry is RC_COST_NONE.  Stream-ordered; returns
 * after the table's upload (it waits for the context's stream).  RC_E_ARG: a null pointer (costs_dev
 * aside), n_models outside 1..RC_MAX_SET_MODELS, n_chunks > RC_MAX_CHUNKS.                   */
rc_status rc_chunk_set_costs(rc_ctx* ctx, const uint32_t* chunk_hist_dev, uint32_t n_chunks,
                             const uint32_t* cost_host, uint32_t n_models, uint8_t* best_row_dev,
                             uint64_t* best_cost_dev, uint64_t* costs_dev);
/* The member chunks' rows summed per class: class_hist_dev[c][s] += the sum of hist[k][s] over the
 * chunks with class_of[k] == c (n_models x 256 u64, ADDED into; a class id >= n_models is
 * skipped).  Asynchronous and stream-ordered.  RC_E_ARG as above.                            */
rc_status rc_histogram_by_class(rc_ctx* ctx, const uint32_t* chunk_hist_dev,
                                const uint8_t* class_of_dev, uint32_t n_chunks, uint32_t n_models,
                                uint64_t* class_hist_dev);

/* ---- order-1 sets: the previous symbol picks the model (encoder.rs:24-37, decoder.rs:38-54) ----
 * The commonest context model: the table of symbol i is chosen by symbol i - 1.  The indexed calls
 * above can write such a stream (idx[i] = f(sym[i-1])) but not read it back, because the decoder
 * has no index stream before it has the symbols.  An order-1 set is the K rows of a static model
 * set (exactly rc_model_create_static_set's rules for n_models, n_symbols, total_freq and the
 * rows) plus a context map:
 *   the row of symbol 0 of every chunk is first_row;
 *   the row of symbol i > 0 is ctx_map[sym[i-1]].
 * Symbol i of chunk k is coded exactly as encoder.encode(&models[row_i], sym[i]) and decoded
 * exactly as decoder.decode(&models[row_i]) with FreqTable::find_index over that row (including
 * its choice of n_symbols-1 when rfreq >= total).  Bytes, lengths and flags are bit-identical to
 * the reference arithmetic, so the encoder's output is that of rc_encode_batch_indexed fed the
 * derived index stream; the decoder is what the indexed calls cannot do.
 *
 * ctx_map_host: n_symbols bytes, every entry < n_models; first_row < n_models; anything else is
 * RC_E_BAD_MODEL.  The map is validated here, on the host, so the kernels never meet a bad row
 * and RC_F_BAD_MODEL cannot occur in the order-1 calls.  n_models <= RC_MAX_SET_MODELS = 64
 * classes of previous symbol is what fits a CU's local memory beside the chunks' rings; a full
 * order-1 model of 256 rows does not fit (256 cum rows alone are 257 KiB of the 160 KiB), so
 * previous symbols are grouped into at most 64 classes by the map.
 *
 * An order-1 set is its own kind of rc_model: the order-1 calls take nothing else (RC_E_ARG for a
 * static, adaptive, set or wide model), and every other entry point that takes a model returns
 * RC_E_ARG for an order-1 set.  Destroy it with rc_model_destroy.                            */
rc_status rc_model_create_order1_set(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                     const uint32_t* c_freq_host,   /* n_models x n_symbols */
                                     const uint32_t* cum_freq_host, /* likewise */
                                     uint32_t total_freq, const uint8_t* ctx_map_host,
                                     uint32_t first_row, rc_model** out);
/* An order-1 set with a period: the position in a record joins the context.  Tensors are mostly
 * records of 2, 4 or 8 bytes (fp32, bf16, int32 fields, RGBA), and which byte of its record a
 * symbol is often says more about it than the byte before.  With period P in {1, 2, 4, 8}:
 *   the row of symbol 0 of every chunk is first_row;
 *   the row of symbol i > 0 is ctx_map[(i mod P) * n_symbols + sym[i-1]], i counted from the
 *   chunk's first symbol.
 * Everything else is rc_model_create_order1_set's: the same rules for the tables, the same
 * coding of symbol i as encoder.encode(&models[row_i], sym[i]) / decoder.decode(&models[row_i]),
 * bit-exactly.  A map whose slices do not depend on the previous symbol is a purely positional
 * model; a map of P identical slices codes what the unphased set codes.
 * ctx_map_host: period x n_symbols bytes, slice ph (the map of the symbols with i mod P = ph)
 * at ctx_map_host + ph * n_symbols.  A period outside {1, 2, 4, 8} is RC_E_ARG (periods that do
 * not divide 16 are not supported: the kernels' 16-symbol blocks rely on 16 = 0 mod P); a map
 * entry or first_row >= n_models is RC_E_BAD_MODEL.
 * The result is an order-1 set: rc_encode_batch_order1, rc_decode_batch_order1 and
 * rc_ideal_bits_order1 take it as they are and dispatch on its period.  With period 1 it is the
 * set rc_model_create_order1_set makes (same kernels, same bytes).  A set with period > 1 is
 * refused (RC_E_ARG) by every other entry point that takes a model, rc_container2_pack included:
 * RCB2 frames one map, so a container of it would silently drop the period.                  */
rc_status rc_model_create_order1_set_periodic(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                              const uint32_t* c_freq_host,
                                              const uint32_t* cum_freq_host, uint32_t total_freq,
                                              uint32_t period, const uint8_t* ctx_map_host,
                                              uint32_t first_row, rc_model** out);
/* An order-1 set with a lag: the context is the symbol `lag` positions back.  In a tensor of 2-,
 * 4- or 8-byte records the byte before a symbol is another field of the same number; the byte
 * that tells most about it is the same byte of the record before, sym[i-P].  With lag D and
 * period P, each in {1, 2, 4, 8} and independent of each other:
 *   the row of symbol i < D of every chunk is first_row;
 *   the row of symbol i >= D is ctx_map[(i mod P) * n_symbols + sym[i-D]], i counted from the
 *   chunk's first symbol.
 * Everything else is rc_model_create_order1_set_periodic's: the same rules for the tables and
 * the map (period x n_symbols bytes, entries from n_symbols on name row 0 when staged), the same
 * coding of symbol i as encoder.encode(&models[row_i], sym[i]) / decoder.decode(&models[row_i]),
 * bit-exactly, the same flags, slots and over-read rule, and the first error of a chunk wins.
 * A lag or a period outside {1, 2, 4, 8} is RC_E_ARG; a map entry or first_row >= n_models is
 * RC_E_BAD_MODEL.
 * The result is an order-1 set: rc_encode_batch_order1, rc_decode_batch_order1 and
 * rc_ideal_bits_order1 take it as they are and dispatch on its lag.  With lag 1 the call is
 * rc_model_create_order1_set_periodic itself (same kernels, same bytes).  A lagged set needs no
 * more local memory than the periodic set of its (n_models, total_freq, period).  A set with
 * lag > 1 is refused (RC_E_ARG) by every other entry point that takes a model, rc_container2_pack
 * included: RCB2 has no field for a lag.                                                     */
rc_status rc_model_create_order1_set_lagged(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                            const uint32_t* c_freq_host,
                                            const uint32_t* cum_freq_host, uint32_t total_freq,
                                            uint32_t period, uint32_t lag,
                                            const uint8_t* ctx_map_host, uint32_t first_row,
                                            rc_model** out);
/* rc_encode_batch with the row chosen by the chunk's previous symbol.
 * flags_dev     RC_F_BAD_SYMBOL for a symbol >= n_symbols, RC_F_ZERO_FREQ against the row the
 *               context chose, RC_F_CAPACITY with the exact length in out_len, RC_F_TOO_LONG; the
 *               first error of a chunk wins.  After a flag the chunk's remaining output is
 *               unspecified (the symbol after a bad symbol is coded with row 0); a flagged chunk
 *               never reads or writes outside its slots.
 * Asynchronous and stream-ordered on the context's stream, like rc_encode_batch.           */
rc_status rc_encode_batch_order1(rc_ctx* ctx, const rc_model* o1, const uint8_t* syms_dev,
                                 const uint64_t* sym_off_dev, uint32_t n_chunks, uint8_t* out_dev,
                                 const uint64_t* out_off_dev, uint64_t* out_len_dev,
                                 uint32_t* flags_dev);
/* rc_decode_batch with the row chosen by the previous DECODED symbol of the chunk.
 * flags_dev     as rc_decode_batch_indexed without RC_F_BAD_MODEL: RC_F_TRUNCATED (also for
 *               code_len < 8, empty chunks included), RC_F_CORRUPT, RC_F_TOO_LONG; the first
 *               error of a chunk wins.
 * Over-read: that of rc_decode_batch_indexed (whole 64-B aligned segments of the code: up to 63
 * bytes before code_off[k] and after code_off[k] + code_len[k] may be READ, never beyond the
 * aligned segment that holds the stream's first or last byte).  Symbols are touched inside
 * [sym_off[k], sym_off[k+1]) only.                                                          */
rc_status rc_decode_batch_order1(rc_ctx* ctx, const rc_model* o1, const uint8_t* code_dev,
                                 const uint64_t* code_off_dev, const uint64_t* code_len_dev,
                                 uint8_t* syms_out_dev, const uint64_t* sym_off_dev,
                                 uint32_t n_chunks, uint32_t* flags_dev);

/* ---- wide static models: alphabets of 16-bit symbols (pmodel.rs:6-12 indexes with usize) ----
 * The reference's PModel is indexed with usize and FreqTable::new(alphabet_count) takes any
 * size; the calls above code one-byte symbols.  A wide static model is one static table over up
 * to RC_MAX_WIDE_SYMBOLS symbols, and the wide batch calls code 16-bit symbols against it: symbol
 * i of chunk k is coded exactly as encoder.encode(&table, sym[i]) and decoded exactly as
 * decoder.decode(&table) with FreqTable::find_index over the table (including its choice of
 * n_symbols-1 when rfreq >= total and its choice among equal cum values).  Bytes, lengths and
 * flags are bit-identical to the reference arithmetic.
 *
 * Accepted when 1 <= n_symbols <= RC_MAX_WIDE_SYMBOLS, 256 <= total_freq <= 65536 (a power of two
 * or not) and the table passes rc_model_create_static's checks; anything else is
 * RC_E_BAD_MODEL.  Zero-frequency symbols are allowed, so n_symbols > total_freq is legal.  The
 * total is bounded for the same reason as for sets: at most 3 bytes settle per symbol, so the
 * margins of both kernels' rings and RC_MAX_CHUNK_SYMBOLS hold unchanged.  The cap of 4096 is
 * where the table still sits in a CU's local memory beside at least 768 chunks' rings in both
 * directions; larger alphabets, up to all 2^16 symbols, are coded by the
 * wide16 models below, whose tables stay in device memory.
 *
 * Symbol buffers hold 16-bit unsigned symbols in host byte order and sym_off counts symbols,
 * not bytes.  They are declared void pointers; a symbol pointer that is not 2-byte aligned is
 * RC_E_ARG.
 *
 * A wide model is its own kind of rc_model: the wide calls take nothing else (RC_E_ARG for a
 * static, adaptive or set model), and every other entry point that takes a model returns RC_E_ARG
 * for a wide model.  Destroy it with rc_model_destroy.                                       */
#define RC_MAX_WIDE_SYMBOLS 4096u
rc_status rc_model_create_static_wide(rc_ctx* ctx, uint32_t n_symbols,
                                      const uint32_t* c_freq_host, const uint32_t* cum_freq_host,
                                      uint32_t total_freq, rc_model** out);
/* rc_encode_batch over 16-bit symbols.
 * syms16_dev    uint16 symbols (index < n_symbols), chunk k = [sym_off[k], sym_off[k+1])
 * flags_dev     as rc_encode_batch: RC_F_BAD_SYMBOL for any 16-bit value >= n_symbols (65535
 *               included), RC_F_ZERO_FREQ, RC_F_CAPACITY with the exact length in out_len,
 *               RC_F_TOO_LONG; the first error of a chunk wins.  After a flag the chunk's
 *               remaining output is unspecified; a flagged chunk never reads or writes outside
 *               its slots.
 * Asynchronous and stream-ordered on the context's stream, like rc_encode_batch.           */
rc_status rc_encode_batch_wide(rc_ctx* ctx, const rc_model* wide, const void* syms16_dev,
                               const uint64_t* sym_off_dev, uint32_t n_chunks, uint8_t* out_dev,
                               const uint64_t* out_off_dev, uint64_t* out_len_dev,
                               uint32_t* flags_dev);
/* rc_decode_batch into 16-bit symbols.
 * syms16_out_dev  uint16 symbols; chunk k gets sym_off[k+1]-sym_off[k] of them
 * flags_dev     as rc_decode_batch (RC_F_TRUNCATED, also for code_len < 8; RC_F_CORRUPT;
 *               RC_F_TOO_LONG); the first error of a chunk wins.
 * Over-read: as rc_decode_batch_indexed (whole 64-B aligned segments of the code).  Symbols are
 * touched inside [sym_off[k], sym_off[k+1]) only.                                           */
rc_status rc_decode_batch_wide(rc_ctx* ctx, const rc_model* wide, const uint8_t* code_dev,
                               const uint64_t* code_off_dev, const uint64_t* code_len_dev,
                               void* syms16_out_dev, const uint64_t* sym_off_dev,
                               uint32_t n_chunks, uint32_t* flags_dev);

/* ---- wide16 static models: the full 16-bit alphabet, tables in device memory ----
 * A wide16 static model is one static table over up to RC_MAX_WIDE16_SYMBOLS (2^16) symbols, so
 * bf16 / fp16 bit patterns, int16 samples and 16-bit indices are coded as they are.  The wide16
 * batch calls have the wide calls' signatures and contract: symbol i of chunk k is coded exactly
 * as encoder.encode(&table, sym[i]) and decoded exactly as decoder.decode(&table) with
 * FreqTable::find_index over the table (its choice of n_symbols-1 when rfreq >= total and its
 * choice among equal cum values included); bytes, lengths and flags are bit-identical to the
 * reference arithmetic, and for n_symbols <= RC_MAX_WIDE_SYMBOLS to the wide calls'.
 *
 * Accepted when 1 <= n_symbols <= RC_MAX_WIDE16_SYMBOLS, 256 <= total_freq <= 65536 (a power of
 * two or not) and the table passes rc_model_create_static's checks; anything else is
 * RC_E_BAD_MODEL.  Zero-frequency symbols are allowed (an alphabet of 2^16 symbols with a total
 * below 2^16 needs them).  The total stays in the small-model regime for the wide models'
 * reason; a table whose total lies above 2^16 belongs to a wide16 fine model
 * (rc_model_create_static_wide16_fine, below), which the same batch calls code.  The tables (at most 512 KiB of encoder entries,
 * 128 KiB of q-to-symbol halfwords and a cum row) are built by the constructor in device memory
 * and read through the L2; the decoder's workgroups stage the halfwords in a CU's local memory
 * beside their rings.
 *
 * Symbol buffers, sym_off, the alignment rule, the flags (RC_F_BAD_SYMBOL for a value >=
 * n_symbols; at n_symbols = 65536 no 16-bit value is one), the RC_F_CAPACITY length rule,
 * RC_F_TOO_LONG, first-error-wins and the over-read and touch rules are the wide calls'.
 *
 * A wide16 model is its own kind of rc_model: the wide16 calls take nothing else (RC_E_ARG), and
 * every other entry point that takes a model returns RC_E_ARG for a wide16 model (containers,
 * sets, order-1 and host-memory helpers over wide16 models are not provided).  Destroy it with
 * rc_model_destroy.                                                                           */
#define RC_MAX_WIDE16_SYMBOLS 65536u
rc_status rc_model_create_static_wide16(rc_ctx* ctx, uint32_t n_symbols,
                                        const uint32_t* c_freq_host,
                                        const uint32_t* cum_freq_host, uint32_t total_freq,
                                        rc_model** out);
rc_status rc_encode_batch_wide16(rc_ctx* ctx, const rc_model* wide16, const void* syms16_dev,
                                 const uint64_t* sym_off_dev, uint32_t n_chunks,
                                 uint8_t* out_dev, const uint64_t* out_off_dev,
                                 uint64_t* out_len_dev, uint32_t* flags_dev);
rc_status rc_decode_batch_wide16(rc_ctx* ctx, const rc_model* wide16, const uint8_t* code_dev,
                                 const uint64_t* code_off_dev, const uint64_t* code_len_dev,
                                 void* syms16_out_dev, const uint64_t* sym_off_dev,
                                 uint32_t n_chunks, uint32_t* flags_dev);

/* ---- wide16 fine models: totals up to 2^24 for the full 16-bit alphabet ----
 * A wide16 fine model is a wide16 static model whose total lies above 2^16: one frequency in 2^16
 * is too coarse once thousands of symbols are rare, and a table over all 2^16 symbols with every
 * symbol encodable is all ones at a total of 2^16.
 *
 * Accepted when 1 <= n_symbols <= RC_MAX_WIDE16_SYMBOLS, 65536 < total_freq <=
 * RC_MAX_WIDE16_FINE_TOTAL (a power of two or not) and the table passes rc_model_create_static's
 * checks; anything else is RC_E_BAD_MODEL, a total of at most 65536 included: such a table is
 * rc_model_create_static_wide16's, so every table has exactly one constructor.  Zero-frequency
 * symbols are allowed.
 *
 * Coding goes through rc_encode_batch_wide16 / rc_decode_batch_wide16, which take a wide16 model
 * of either constructor, and the contract is theirs word for word: symbol i of chunk k is coded
 * exactly as encoder.encode(&table, sym[i]) and decoded exactly as decoder.decode(&table) with
 * FreqTable::find_index over the table (among equal cum values the last is chosen, and the result
 * is n_symbols-1 when rfreq >= total); bytes, lengths and flags are bit-identical to the
 * reference arithmetic.  RC_F_BAD_SYMBOL, RC_F_ZERO_FREQ, the RC_F_CAPACITY length rule,
 * RC_F_TOO_LONG, RC_F_TRUNCATED, RC_F_CORRUPT, first-error-wins and the over-read and touch rules
 * are unchanged.  Every other entry point that takes a model returns RC_E_ARG for a fine model,
 * as for a wide16 model.
 *
 * Bytes per symbol.  A symbol starts with range >= 2^48, so range / total >= 2^24 and the
 * symbol's range r * c is at least 2^24; no_carry_expansion settles k bytes only while that range
 * is below 2^(64 - 8k), so at most 4 (3 at totals up to 2^16), and range_reduction_expansion at
 * most 7 more: one symbol settles at most 11 bytes, and 8 + 11 n bytes hold every chunk of n
 * symbols (RC_STREAM_MAX_BYTES' 12 n + 8 covers it).  That bound is met only where
 * range_reduction_expansion cuts the range down to the part below a byte boundary it straddles,
 * which costs log2(range / part) bits: 1.44 bits on average, on fewer than one symbol in 256.
 * The size to plan an output slot with is therefore the ideal one, log2(total / c) bits per
 * symbol (up to 24), plus the flush's 8 bytes and a little slack; a slot that turns out too
 * small is RC_F_CAPACITY with the exact length, as ever.  A slot sized that
 * way carries no guarantee: only 8 + 11 n bytes are certain to hold a chunk of n symbols, and a
 * caller who sizes by the ideal cost must check the flags and encode a flagged chunk again.
 *
 * The tables (at most 512 KiB of encoder entries; for the decoder the occupied symbols, their
 * cum row and a bucket table over the top bits of the scaled code value, at most 512 KiB together)
 * are built by the constructor in device memory; the decoder's workgroups stage the bucket table
 * in a CU's local memory beside their rings.  Destroy the model with rc_model_destroy.          */
#define RC_MAX_WIDE16_FINE_TOTAL (1u << 24)
rc_status rc_model_create_static_wide16_fine(rc_ctx* ctx, uint32_t n_symbols,
                                             const uint32_t* c_freq_host,
                                             const uint32_t* cum_freq_host, uint32_t total_freq,
                                             rc_model** out);

/* ---- synchronous host-memory helpers (stage through device memory, wait for completion;
 *      returns RC_E_CHUNK when any chunk is flagged — flags are still filled in).  Their
 *      staging buffers (4 x ~2 batches of ~1 GiB, on the context's device) stay allocated
 *      with the context between calls and are freed by rc_ctx_destroy. ---- */
rc_status rc_encode_host(rc_ctx* ctx, const rc_model* m, const uint8_t* syms,
                         const uint64_t* sym_off, uint32_t n_chunks, uint8_t* out,
                         const uint64_t* out_off, uint64_t* out_len, uint32_t* flags);
rc_status rc_decode_host(rc_ctx* ctx, const rc_model* m, const uint8_t* code,
                         const uint64_t* code_off, const uint64_t* code_len, uint8_t* syms_out,
                         const uint64_t* sym_off, uint32_t n_chunks, uint32_t* flags);

/* ---- several devices of one node from one host thread (the rc_*_multi entry points) ----
 * rc_encode_host / rc_decode_host over a list of contexts (one per device; two contexts on one
 * device also work): the chunks are cut into n_ctx contiguous ranges of about equal input
 * bytes, coded concurrently (one host thread per context).  Chunks are independent streams
 * (a fresh Encoder each, encoder.rs:48-55), so there is no data-path exchange between devices:
 * every device reads its range of the caller's buffers and writes its chunks' results in place.
 * models[i] is the model as created on ctxs[i]'s device (identical tables).  Returns the first
 * failing status, RC_E_CHUNK when a chunk is flagged, else RC_OK.                             */
rc_status rc_encode_host_multi(rc_ctx* const* ctxs, const rc_model* const* models, uint32_t n_ctx,
                               const uint8_t* syms, const uint64_t* sym_off, uint32_t n_chunks,
                               uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                               uint32_t* flags);
rc_status rc_decode_host_multi(rc_ctx* const* ctxs, const rc_model* const* models, uint32_t n_ctx,
                               const uint8_t* code, const uint64_t* code_off,
                               const uint64_t* code_len, uint8_t* syms_out,
                               const uint64_t* sym_off, uint32_t n_chunks, uint32_t* flags);

/* ---- resumable streams: the reference's per-call Encoder / Decoder (any PModel) ----
 * The batch entry points code whole chunks against one table.  The reference instead reads the
 * model on EVERY call — Encoder::encode takes (c_freq(i), cum_freq(i), total_freq()) of the
 * caller's PModel at that moment (encoder.rs:24-31), Decoder::decode runs find_index and reads
 * the table again (decoder.rs:38-50) — so a caller may change its model between calls
 * (adaptive models).  These entry points keep a stream's state between calls instead:
 *   encode: the caller passes the (c, cum, total) triple it read for each symbol;
 *   decode: the caller passes the table to use for the next n symbols (FreqTable::find_index's
 *           binary search over cum, sample_impl.rs:27-45, and param_update over (c, cum, total),
 *           evaluated as given: no consistency requirement on the table).
 * State positions are 64-bit: a stream has no length limit.  Per-symbol arithmetic follows
 * range_coder.rs:53-135 exactly; where the reference panics or never terminates the stream is
 * flagged (sticky) and stops before that symbol. */
typedef struct rc_stream_state {
  uint64_t lower_bound, range; /* RangeCoder (range_coder.rs:7-12): Encoder::range_coder, or
                                  Decoder::range_coder() (decoder.rs:24-26)                   */
  uint64_t data;               /* decoder: Decoder::data() (decoder.rs:27-29)                */
  uint64_t pos;                /* encoder: code bytes emitted (peek_code().len(), encoder.rs:18);
                                  decoder: code bytes consumed, incl. the 8 of Decoder::new   */
  uint64_t n;                  /* symbols coded so far                                       */
  uint32_t flags;              /* sticky RC_F_* (ZERO_FREQ, BAD_MODEL, TRUNCATED, CORRUPT,
                                  FINISHED)                                                  */
  uint32_t stage;              /* 0 fresh (a decoder runs Decoder::new on its first call),
                                  1 running, 2 finished (encoder)                            */
} rc_stream_state;
/* RangeCoder::default / Encoder::new / a decoder before Decoder::new */
#define RC_STREAM_STATE_INIT {0u, ~(uint64_t)0, 0u, 0u, 0u, 0u, 0u}
/* bytes one call may emit: a symbol settles at most 12 bytes, finish 8 */
#define RC_STREAM_MAX_BYTES(n, finish) (12ull * (uint64_t)(n) + ((finish) ? 8ull : 0ull))

/* Encoder::encode x n (+ Encoder::finish if `finish`) for n_streams independent streams.
 * states_dev     n_streams rc_stream_state, updated in place
 * triples_dev    per symbol {c_freq, cum_freq, total_freq} (3 x uint32); stream k's symbols are
 *                triples [sym_off[k], sym_off[k+1])
 * out_dev        this call's NEW bytes of stream k go to out[out_off[k] ..); the slot must hold
 *                RC_STREAM_MAX_BYTES(symbols, finish) or the stream is flagged RC_F_CAPACITY
 *                (not sticky) and left unchanged
 * out_len_dev    n_streams: new bytes written
 * nbytes_dev     NULL or one uint8 per symbol (same indexing as the triples): encode()'s return
 *                value, the bytes that symbol settled (encoder.rs:34-36)
 * flags_dev      n_streams: RC_F_* of this call (the sticky ones are also in the state)      */
rc_status rc_stream_encode(rc_ctx* ctx, rc_stream_state* states_dev, const uint32_t* triples_dev,
                           const uint64_t* sym_off_dev, uint32_t n_streams, uint8_t* out_dev,
                           const uint64_t* out_off_dev, uint64_t* out_len_dev,
                           uint8_t* nbytes_dev, uint32_t finish, uint32_t* flags_dev);
/* Decoder::decode x (sym_off[k+1] - sym_off[k]) for n_streams streams against one table
 * (c_dev, cum_dev: n_symbols uint32 each; total_freq).  Stream k's whole code is
 * code[code_off[k] .. + code_len[k]) and the state's pos indexes it.  Symbols go to
 * syms_dev[sym_off[k] ..).  A stream stops before its first failing symbol; state.n counts the
 * symbols decoded.                                                                           */
rc_status rc_stream_decode(rc_ctx* ctx, const uint32_t* c_dev, const uint32_t* cum_dev,
                           uint32_t n_symbols, uint32_t total_freq, rc_stream_state* states_dev,
                           const uint8_t* code_dev, const uint64_t* code_off_dev,
                           const uint64_t* code_len_dev, uint8_t* syms_dev,
                           const uint64_t* sym_off_dev, uint32_t n_streams, uint32_t* flags_dev);
/* The same pair against a table per symbol, out of rows held in device memory: tables that both
 * sides know beforehand and that change from symbol to symbol (chosen by side information, by
 * position, by a model evaluated earlier), any number of rows, in one launch.
 * A row table: n_rows tables of n_symbols (1..256) entries each, row-major in device memory:
 * c_dev, cum_dev  n_rows * n_symbols uint32;  total_dev  n_rows uint32.
 * Evaluated as given, like rc_stream_decode's table: no consistency requirement.
 * row_of_dev: one uint32 per symbol, indexed like syms (stream k's symbols are
 * [sym_off[k], sym_off[k+1])): the row that symbol is coded against.
 * Symbol i of stream k, g = sym_off[k] + i, r = row_of[g], is coded exactly as rc_stream_decode
 * would with the table (c + r n_symbols, cum + r n_symbols, n_symbols, total[r]), or
 * rc_stream_encode with the triple (c[r][s], cum[r][s], total[r]), s = syms[g]: the same state
 * (Decoder::new on a fresh one), finish, nbytes and capacity rule, sticky flags, and stop before
 * the first failing symbol.  Two checks come first, per symbol: row_of[g] >= n_rows is
 * RC_F_BAD_MODEL; encode only, syms[g] >= n_symbols is RC_F_BAD_SYMBOL (sticky, too).
 * RC_E_BAD_MODEL: n_symbols outside 1..256; RC_E_ARG: a null pointer (nbytes_dev may be NULL), or
 * n_rows == 0 with n_streams > 0.
 * The decoder is one of two kernels with the same results, picked per launch by the stream count
 * against the device's CU count: one wave per stream (fewer than 16 streams per CU, and always
 * for 64 streams or fewer), which reads a symbol's whole row coalesced and code bytes in aligned
 * dwords; or one lane per stream, which reads only the row entries its search visits and code
 * bytes in aligned 8-byte words.  Neither reads a code byte outside the 64-B segments that hold a
 * byte of the stream, or a table entry outside the rows.                                        */
rc_status rc_stream_decode_rows(rc_ctx* ctx, const uint32_t* c_dev, const uint32_t* cum_dev,
                                const uint32_t* total_dev, uint32_t n_rows, uint32_t n_symbols,
                                const uint32_t* row_of_dev, rc_stream_state* states_dev,
                                const uint8_t* code_dev, const uint64_t* code_off_dev,
                                const uint64_t* code_len_dev, uint8_t* syms_dev,
                                const uint64_t* sym_off_dev, uint32_t n_streams,
                                uint32_t* flags_dev);
rc_status rc_stream_encode_rows(rc_ctx* ctx, const uint32_t* c_dev, const uint32_t* cum_dev,
                                const uint32_t* total_dev, uint32_t n_rows, uint32_t n_symbols,
                                const uint32_t* row_of_dev, const uint8_t* syms_dev,
                                rc_stream_state* states_dev, const uint64_t* sym_off_dev,
                                uint32_t n_streams, uint8_t* out_dev, const uint64_t* out_off_dev,
                                uint64_t* out_len_dev, uint8_t* nbytes_dev, uint32_t finish,
                                uint32_t* flags_dev);
/* One stream in host memory, synchronous (the host mirrors' Encoder / Decoder).  Only the bytes a
 * call can touch cross PCIe: the encoder's new bytes, the decoder's window
 * [pos, pos + RC_STREAM_MAX_BYTES(n, 0) + 8).  Return RC_E_CHUNK when a flag is set (in
 * *flags_out, and sticky ones in the state).
 * Small calls (request and result within 64 KiB) go to the context's stream-service wave: one
 * workgroup of one wave, launched by the first such call on a stream of its own, holding 64.4 KiB
 * of one CU's LDS, which polls a mailbox in pinned host memory and leaves 0.25 ms after its last
 * request, 1 ms after its launch at most, or as soon as a batch entry point of the library
 * launches a kernel (the next call launches another wave).  While it runs it occupies that CU
 * slot and its hardware queue like any resident kernel: a kernel of another library on a
 * stream that shares that queue can wait up to 1 ms behind it.  A call waits for the
 * wave WITHOUT a time limit while the wave has not started (a wave waiting for a CU behind
 * long-running kernels is waited for, exactly as a launch would be); once the wave runs, a
 * call that sees no answer within 10 s returns RC_E_DEVICE and the context's service is off
 * from then on (later calls take the launch path).  RC_STREAM_SERVICE=0 (below) sends every
 * call down the launch path.                                                                 */
rc_status rc_stream_encode_host(rc_ctx* ctx, rc_stream_state* state, const uint32_t* triples,
                                uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                uint8_t* nbytes, uint32_t finish, uint32_t* flags_out);
rc_status rc_stream_decode_host(rc_ctx* ctx, const uint32_t* c, const uint32_t* cum,
                                uint32_t n_symbols, uint32_t total_freq, rc_stream_state* state,
                                const uint8_t* code, uint64_t code_len, uint8_t* syms,
                                uint64_t n, uint32_t* flags_out);

/* ---- synthetic workload generator (bench/test inputs, generated in HBM) ----
 * Fills n_chunks chunks of chunk_len symbols at syms_dev (chunk k at k*chunk_len).  Symbol i of
 * chunk k = inv_cdf[u16] where u16 = bits [16(i%4), 16(i%4)+16) of
 * mix64(seed + 0x9E3779B97F4A7C15 * ((k << 32) + i/4 + 1)) (splitmix64 finaliser).
 * inv_cdf_host: 65536 symbol bytes (an inverse CDF quantised to 2^16).                      */
rc_status rc_synth_fill(rc_ctx* ctx, uint64_t seed, const uint8_t* inv_cdf_host,
                        uint8_t* syms_dev, uint64_t chunk_len, uint32_t n_chunks);

/* ---- model construction: the step before encode ----
 * The reference builds a FreqTable by counting symbols (FreqTable::new + add_alphabet_freq per
 * symbol, examples/sample_impl.rs:49-60) and then scanning (calc_cum, :61-69).              */

/* Symbol histogram of n_chunks chunks (device pointers; stream-ordered).
 * chunk_hist_dev  NULL or n_chunks*256 uint32: row k = counts of chunk k (overwritten)
 * hist_dev        NULL or 256 uint64: batch counts ADDED into it (zero it first)          */
rc_status rc_histogram(rc_ctx* ctx, const uint8_t* syms_dev, const uint64_t* sym_off_dev,
                       uint32_t n_chunks, uint32_t* chunk_hist_dev, uint64_t* hist_dev);

/* Histogram of 16-bit symbols (device pointers; stream-ordered on the context's stream).
 * syms16_dev      uint16 symbols, host byte order, 2-byte aligned (else RC_E_ARG);
 *                 chunk k = [sym_off[k], sym_off[k+1]), offsets in symbols
 * n_bins          1..RC_MAX_WIDE_SYMBOLS (else RC_E_ARG)
 * chunk_hist_dev  NULL or n_chunks*n_bins uint32: row k = counts of chunk k (overwritten)
 * hist_dev        NULL or n_bins uint64: batch counts ADDED into it (zero it first)
 * oob_dev         NULL or one uint64: the number of symbols >= n_bins (65535 included),
 *                 ADDED into it; such symbols are counted nowhere else
 * The batch counts are exact for any batch size.  With all three results NULL the call does
 * nothing (RC_OK).  Without rows the counters live on chip across a workgroup's chunks; asking
 * for rows costs a readout of n_bins counters per chunk, which at n_bins = 4096 is the same
 * order of work as counting a chunk of 16 Ki symbols.                                       */
rc_status rc_histogram_wide(rc_ctx* ctx, const void* syms16_dev, const uint64_t* sym_off_dev,
                            uint32_t n_chunks, uint32_t n_bins, uint32_t* chunk_hist_dev,
                            uint64_t* hist_dev, uint64_t* oob_dev);

/* Pair counts by context class: the counts from which the rows of an order-1 set are quantised
 * (rc_quantize_counts per row, with RC_Q_ALL_SYMBOLS, then rc_model_create_order1_set).
 * hist_dev: n_models x 256 uint64, ADDED into (zero it first).  Row j counts the symbols of all
 * chunks whose context row is j under (ctx_map_host, first_row): first_row for the first symbol
 * of a chunk, ctx_map[previous symbol] for every other one.  Symbols index the map with their
 * full byte value (ctx_map_host: 256 entries, each < n_models <= RC_MAX_SET_MODELS, and
 * first_row < n_models; anything else is RC_E_ARG).  Stream-ordered.                        */
rc_status rc_histogram_order1(rc_ctx* ctx, uint32_t n_models, const uint8_t* ctx_map_host,
                              uint32_t first_row, const uint8_t* syms_dev,
                              const uint64_t* sym_off_dev, uint32_t n_chunks, uint64_t* hist_dev);

/* The full pair histogram of a batch: what a context map is fitted from (rc_cluster_contexts).
 * pair_hist_dev   NULL or 256 x 256 uint64: [p][s] is increased by the number of positions
 *                 i >= 1 of a chunk with sym[i-1] = p and sym[i] = s
 * first_hist_dev  NULL or 256 uint64: [s] is increased by the number of non-empty chunks whose
 *                 symbol 0 is s
 * Chunk boundaries reset the context: the last symbol of a chunk never pairs with the first of
 * the next.  Counts are ADDED into the arrays (zero them first) and are exact for any data.
 * With both results NULL the call does nothing (RC_OK).  Device pointers; stream-ordered.   */
rc_status rc_histogram_pairs(rc_ctx* ctx, const uint8_t* syms_dev, const uint64_t* sym_off_dev,
                             uint32_t n_chunks, uint64_t* pair_hist_dev,
                             uint64_t* first_hist_dev);

/* rc_histogram_pairs with the position in a record as a third index: what the maps of a periodic
 * order-1 set are fitted from, one slice per phase.  period: 1, 2, 4 or 8 (else RC_E_ARG).
 * pair_hist_dev   NULL or period x 256 x 256 uint64: [ph][p][s] is increased by the number of
 *                 positions i >= 1 of a chunk with i mod period = ph, sym[i-1] = p, sym[i] = s
 *                 (i counted from the chunk's first symbol)
 * first_hist_dev  as rc_histogram_pairs
 * Chunk boundaries reset the context; counts are ADDED into the arrays and are exact for any
 * data; with both results NULL the call does nothing (RC_OK).  Summed over ph the pair counts
 * are rc_histogram_pairs'.  Every phase reads the symbols again, so the call takes about
 * `period` times as long.  Device pointers; stream-ordered.                                 */
rc_status rc_histogram_pairs_periodic(rc_ctx* ctx, uint32_t period, const uint8_t* syms_dev,
                                      const uint64_t* sym_off_dev, uint32_t n_chunks,
                                      uint64_t* pair_hist_dev, uint64_t* first_hist_dev);

/* rc_histogram_pairs_periodic with the pairs taken at a distance: what the maps of a lagged
 * order-1 set are fitted from.  period and lag: each 1, 2, 4 or 8 (else RC_E_ARG).
 * pair_hist_dev   NULL or period x 256 x 256 uint64: [ph][p][s] is increased by the number of
 *                 positions i >= lag of a chunk with i mod period = ph, sym[i-lag] = p and
 *                 sym[i] = s (i counted from the chunk's first symbol)
 * first_hist_dev  NULL or 256 uint64: [s] is increased by the number of positions i < lag of a
 *                 chunk with sym[i] = s: a chunk of n symbols adds min(lag, n) counts, the symbols
 *                 that a lagged set codes with first_row
 * So sum(pair) + sum(first) is the number of symbols.  Chunk boundaries reset the context; counts
 * are ADDED into the arrays and are exact for any data; with both results NULL the call does
 * nothing (RC_OK).  With lag 1 the call is rc_histogram_pairs_periodic.  Device pointers;
 * stream-ordered.                                                                            */
rc_status rc_histogram_pairs_lagged(rc_ctx* ctx, uint32_t period, uint32_t lag,
                                    const uint8_t* syms_dev, const uint64_t* sym_off_dev,
                                    uint32_t n_chunks, uint64_t* pair_hist_dev,
                                    uint64_t* first_hist_dev);

/* Pair counts -> a context map of at most max_models classes and a first_row (host only, no
 * device needed; deterministic): greedy agglomerative clustering under the empirical-entropy
 * cost(v) = sum over v_s > 0 of v_s * log2(sum(v) / v_s), in f64.
 * The items are the 256 contexts (row p of pair_hist_host) and a pseudo-context 256, "start of
 * chunk", whose counts are first_hist_host; an item without samples is not clustered.  One
 * cluster per item with samples; while more than max_models remain, the pair (a, b) with the
 * smallest cost(a + b) - cost(a) - cost(b) is merged, ties going to the pair whose (smallest
 * member of a, smallest member of b) is lexicographically smallest.  Rows are numbered by
 * ascending smallest member.
 * ctx_map_out     256 entries: the row of context p; a context without samples gets the row with
 *                 the largest total count (the lowest such row); entries from n_symbols on are 0
 * first_row_out   the row of pseudo-context 256 (without samples: as a context without samples)
 * n_models_out    the number of rows, <= max_models (fewer when fewer items have samples)
 * cost_bits_out   NULL or the sum of the rows' costs: the ideal bits of the counted symbols
 *                 under the exact, unquantised rows
 * RC_E_ARG: a null pointer, max_models outside 1..RC_MAX_SET_MODELS, n_symbols outside 1..256
 * (or counts that sum past 2^63); RC_E_BAD_SYMBOL: a non-zero count in a row or column >=
 * n_symbols; RC_E_BAD_MODEL: every count is zero.                                           */
rc_status rc_cluster_contexts(const uint64_t* pair_hist_host, const uint64_t* first_hist_host,
                              uint32_t n_symbols, uint32_t max_models, uint8_t* ctx_map_out,
                              uint32_t* first_row_out, uint32_t* n_models_out,
                              double* cost_bits_out);

/* rc_cluster_contexts on the device and over the phases of periodic pair counts jointly, so that
 * the phases share the rows.  period: 1, 2, 4 or 8.
 * pair_hist_dev   period x 256 x 256 uint64, as rc_histogram_pairs_periodic writes it (at
 *                 period 1: rc_histogram_pairs' array); first_hist_dev: 256 uint64.  Device
 *                 pointers, read stream-ordered and never written.
 * The items are (phase, context) pairs, item ph * 256 + p being row [ph][p] of the pair counts,
 * and item period * 256, "start of chunk", with the counts of first_hist_dev: 256 period + 1 in
 * all.  The rule is rc_cluster_contexts' over these items (one cluster per item with samples in
 * the slot of its smallest member; the pair with the smallest delta merged while more than
 * max_models remain; ties to the lexicographically smallest (smallest member of a, smallest
 * member of b); rows by ascending smallest member; an item without samples gets the lowest row
 * with the largest total), with the delta taken as cost(a + b) - (cost(a) + cost(b)): symmetric
 * in a and b, each cost one fixed-order f64 sum of non-negative terms.  At period 1 the items and
 * the rule are rc_cluster_contexts' own; the two agree unless two deltas of a merge lie within
 * rounding (about 300 * 2^-52 of cost(a + b)) of each other.
 * ctx_map_out     host, period x 256: [ph * 256 + p] is the row of item ph * 256 + p; entries
 *                 with p >= n_symbols are 0.  The first n_symbols entries of every phase are what
 *                 rc_model_create_order1_set_periodic takes.
 * first_row_out, n_models_out, cost_bits_out (may be NULL): host, as rc_cluster_contexts.
 * RC_E_ARG: a period other than 1, 2, 4, 8, a null pointer, max_models outside
 * 1..RC_MAX_SET_MODELS, n_symbols outside 1..256, counts that sum past 2^63;
 * RC_E_BAD_SYMBOL: a non-zero count in a row or column >= n_symbols (found first);
 * RC_E_BAD_MODEL: every count is zero.
 * The call waits for the stream before it returns (the results go to the host).  Work memory:
 * 8 (256 period + 1)^2 bytes and about 2 KiB per item, from the stream's memory pool.        */
rc_status rc_cluster_contexts_dev(rc_ctx* ctx, uint32_t period, const uint64_t* pair_hist_dev,
                                  const uint64_t* first_hist_dev, uint32_t n_symbols,
                                  uint32_t max_models, uint8_t* ctx_map_out,
                                  uint32_t* first_row_out, uint32_t* n_models_out,
                                  double* cost_bits_out);

/* Batched ideal code length under an order-1 set, straight from the symbols:
 * bits_dev[k] = sum over the symbols i of chunk k of log2(total / c[row_i][sym_i]), f64, with
 * row_0 = first_row and row_i = ctx_map[sym[i-1]] as the order-1 coders pick them (after a
 * symbol >= n_symbols the next row is row 0, as they stage the map); for a periodic set
 * row_i = ctx_map[(i mod P) * n_symbols + sym[i-1]], for a lagged set first_row for i < D and
 * ctx_map[(i mod P) * n_symbols + sym[i-D]] from there on, with the same sums.  A term with c == 0 or a
 * symbol >= n_symbols makes its chunk +inf; an empty chunk is 0.0; nothing is NaN.
 * `o1` must be an order-1 set of this context's device (RC_E_ARG for any other kind of model).
 * Stream-ordered; the call waits for the stream (it reads the set's rows back to price them on
 * the host, as rc_ideal_bits_wide does).
 * Accuracy: each chunk is summed as 64 partial sums, each in runs of 16 consecutive symbols,
 * and a 6-step butterfly, so a finite result is within about (n_k / 64 + 22) * 2^-53 relative
 * of the exact sum of its n_k terms.                                                        */
rc_status rc_ideal_bits_order1(rc_ctx* ctx, const rc_model* o1, const uint8_t* syms_dev,
                               const uint64_t* sym_off_dev, uint32_t n_chunks, double* bits_dev);

/* Counts -> (c, cum, total) table (host only, no device needed).
 * target_total == 0: calc_cum's exact table, c = counts (total must stay < 2^32; with
 * RC_Q_ALL_SYMBOLS absent symbols get c = 1);
 * otherwise c_i = max(1, round(counts_i * T / sum)) for modelled symbols, the difference to T
 * folded into the largest entry (deficit; lowest index on ties) or taken from the largest
 * entries first, never below 1 (excess).  Modelled symbols: counts_i > 0, or every symbol
 * with RC_Q_ALL_SYMBOLS (so symbols absent from the sample stay encodable).
 * Returns RC_E_BAD_MODEL when no table exists (T below the number of modelled symbols, an
 * empty sample without RC_Q_ALL_SYMBOLS, a total >= 2^32).                                  */
#define RC_Q_ALL_SYMBOLS 1u
rc_status rc_quantize_counts(const uint64_t* counts_host, uint32_t n_symbols,
                             uint64_t target_total, uint32_t qflags, uint32_t* c_out_host,
                             uint32_t* cum_out_host, uint32_t* total_out_host);
/* The same rule for the alphabets of wide static models: n_symbols <= RC_MAX_WIDE_SYMBOLS
 * (rc_quantize_counts keeps its own limit of 256 and its results).                          */
rc_status rc_quantize_counts_wide(const uint64_t* counts_host, uint32_t n_symbols,
                                  uint64_t target_total, uint32_t qflags, uint32_t* c_out_host,
                                  uint32_t* cum_out_host, uint32_t* total_out_host);
/* The same rule for the alphabets of wide16 static models: n_symbols <= RC_MAX_WIDE16_SYMBOLS.
 * RC_Q_ALL_SYMBOLS with n_symbols above a nonzero target_total is RC_E_ARG (no table of that
 * total keeps every symbol encodable).  The 16-bit histogram comes from
 * rc_histogram_pairs_periodic(period 2) over the symbols' bytes.          */
rc_status rc_quantize_counts_wide16(const uint64_t* counts_host, uint32_t n_symbols,
                                    uint64_t target_total, uint32_t qflags,
                                    uint32_t* c_out_host, uint32_t* cum_out_host,
                                    uint32_t* total_out_host);
/* The same rule for the totals of wide16 fine models: 65536 < target_total <=
 * RC_MAX_WIDE16_FINE_TOTAL, anything else (0, the exact table, included) is RC_E_ARG.        */
rc_status rc_quantize_counts_wide16_fine(const uint64_t* counts_host, uint32_t n_symbols,
                                         uint64_t target_total, uint32_t qflags,
                                         uint32_t* c_out_host, uint32_t* cum_out_host,
                                         uint32_t* total_out_host);

/* Batched PModel::ideal_code_length (pmodel.rs:14-40): bits_dev[k] = sum over symbols s of
 * chunk k of log2(total / c[s]) = sum_i hist[k][i] * (ln total - ln c_i) / ln 2, in f64,
 * from rc_histogram's chunk rows.  A symbol with c == 0 (no code length in the reference)
 * makes its chunk's sum +inf.  Synchronous with respect to the host table.                 */
rc_status rc_ideal_bits(rc_ctx* ctx, const uint32_t* c_freq_host, uint32_t n_symbols,
                        uint32_t total_freq, const uint32_t* chunk_hist_dev, uint32_t n_chunks,
                        double* bits_dev);

/* Batched PModel::ideal_code_length over a wide model, straight from the symbols:
 * bits_dev[k] = sum over the symbols s of chunk k of log2(total / c[s]), f64.
 * A symbol with c == 0 or s >= n_symbols makes its chunk +inf; an empty chunk is 0.0.
 * `wide` must be a wide static model (RC_E_ARG for any other kind).  syms16_dev and
 * sym_off_dev as in rc_histogram_wide.  Stream-ordered; the call waits for the stream (it reads
 * the model's table back to price it on the host, as rc_ideal_bits prices its host table).
 * Accuracy: each chunk is summed as 64 partial sums and a 6-step butterfly, so a finite result
 * is within about (n_k / 64 + 7) * 2^-53 relative of the exact sum of its n_k terms.        */
rc_status rc_ideal_bits_wide(rc_ctx* ctx, const rc_model* wide, const void* syms16_dev,
                             const uint64_t* sym_off_dev, uint32_t n_chunks, double* bits_dev);

/* ---- chunked container "RCB1"  ----
 * The reference's stream carries neither its symbol count (sample_impl.rs:113-120) nor its
 * model (decoder.rs:38).  The container frames a batch of chunk streams with both:
 *   offset 0          header, RC_CONTAINER_HEADER_BYTES, little-endian:
 *                       0 "RCB1"  4 u32 version 1 | header bytes << 16  8 u32 kind (0 static,
 *                       1 adaptive)  12 u32 n_symbols  16 u32 total_freq (static)
 *                       20/24/28 u32 increment/limit/period (adaptive)  32 u64 n_chunks
 *                       40 u64 symbols in all chunks  48 u64 payload bytes  56 reserved (0)
 *   table_off = 64    static: n_symbols x u32 c_freq (cum rebuilt by calc_cum), zero padded
 *                     to 16 B; adaptive: empty
 *   index_off         n_chunks x {u64 symbol count, u64 code length}
 *   payload_off       = index_off + 16 n_chunks; chunk k's code stream starts at payload_off +
 *                     sum_{j<k} pad16(code length j), zero padded to 16 B
 * A container is produced from encode_batch's slots and read back for decode_batch.        */
#define RC_CONTAINER_HEADER_BYTES 64
typedef struct rc_container_info {
  uint32_t version, kind, n_symbols, total_freq, increment, limit, period, reserved;
  uint64_t n_chunks, n_syms, payload_bytes;
  uint64_t table_off, index_off, payload_off, container_bytes;
} rc_container_info;

/* Pack encoded slots (rc_encode_batch's out/out_off/out_len, chunk sizes from sym_off) and
 * the model into a container at dst_dev.  Synchronous.  *dst_len_host receives the container
 * size; RC_E_CAPACITY (nothing written) when it exceeds dst_cap or dst_dev is NULL.        */
rc_status rc_container_pack(rc_ctx* ctx, const rc_model* m, const uint8_t* slots_dev,
                            const uint64_t* slot_off_dev, const uint64_t* code_len_dev,
                            const uint64_t* sym_off_dev, uint32_t n_chunks, uint8_t* dst_dev,
                            uint64_t dst_cap, uint64_t* dst_len_host);
/* Parse the header (head_host: the first >= RC_CONTAINER_HEADER_BYTES bytes). */
rc_status rc_container_info_parse(const uint8_t* head_host, uint64_t head_len,
                                  rc_container_info* info);
/* Decode arguments from a device-resident container: code_off/code_len (n_chunks each, into
 * the container), sym_off (n_chunks + 1).  Synchronous; RC_E_BAD_CONTAINER when the index does
 * not add up to the header's payload and symbol totals.                                    */
rc_status rc_container_offsets(rc_ctx* ctx, const uint8_t* container_dev,
                               const rc_container_info* info, uint64_t* code_off_dev,
                               uint64_t* code_len_dev, uint64_t* sym_off_dev);

/* ---- chunked container "RCB2": order-1 sets, wide models, per-chunk checksums ----
 * RCB1 frames an order-0 static table or the adaptive model and nothing else, and it stores no
 * check of the decoded data: a damaged payload byte may decode, unflagged, to other symbols.
 * RCB2 is a second format beside it (RCB1 and its entry points are unchanged, and
 * rc_container_info_parse keeps rejecting the magic "RCB2"): it also frames an order-1 set or a
 * wide static model, and it may carry one 32-bit checksum of the decoded symbols per chunk.
 * All fields little-endian; every section starts 16-B aligned and is zero padded to 16 B:
 *   offset 0          header, RC_CONTAINER_HEADER_BYTES:
 *                       0 "RCB2"  4 u32 version 1 | header bytes << 16
 *                       8 u32 kind: 0 static, 1 adaptive, 2 order-1 set, 3 wide static
 *                       12 u32 n_symbols (1..256; 1..RC_MAX_WIDE_SYMBOLS for kind 3)
 *                       16 u32 total_freq (kinds 0, 2, 3)
 *                       20/24/28 u32 kind 1: increment/limit/period; kind 2: n_models K
 *                       (1..RC_MAX_SET_MODELS) / first_row (< K) / 0
 *                       32 u64 n_chunks  40 u64 symbols in all chunks  48 u64 payload bytes
 *                       56 u32 flags: RC_CONTAINER2_F_CHECKSUMS, every other bit 0   60 u32 0
 *   table_off = 64    kinds 0 and 3: n_symbols x u32 c_freq; kind 2: K x n_symbols u32 c_freq,
 *                     row-major, then n_symbols bytes of ctx_map (at most 64 KiB + 256 B);
 *                     kind 1: empty.  cum is always rebuilt by calc_cum.
 *   index_off         n_chunks x {u64 symbol count, u64 code length}, as RCB1
 *   sum_off           n_chunks x u32 checksums; present only with RC_CONTAINER2_F_CHECKSUMS
 *   payload_off       the streams as in RCB1: each starts 16-B aligned, zero padded to 16 B
 * A symbol of kind 3 is two bytes (host byte order = little-endian); all counts are in symbols.
 *
 * The checksum of a chunk.  Take its symbols as bytes: L = count x symbol size, in chunk order.
 *   w_i   = the little-endian u32 of bytes 4i .. 4i+3, zero padded past L, for i < ceil(L / 4)
 *   S     = sum_i fmix32((w_i + (i + 1) * 0x9E3779B1) mod 2^32)  mod 2^32
 *   sum   = fmix32(S ^ (u32)L)
 * with fmix32 MurmurHash3's 32-bit finaliser (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13;
 * h *= 0xC2B2AE35; h ^= h >> 16).  The sum over positions is order-free, so the result does not
 * depend on how a launch splits the chunk; the position term catches moved words; fmix32 is a
 * bijection, so a change confined to one word always changes the result.  It guards against
 * accidents (a damaged byte, a truncated or misplaced stream), NOT against an adversary: a
 * forger can solve for a matching sum, and unrelated damage in several words collides with
 * probability about 2^-32.                                                                  */
#define RC_CONTAINER2_F_CHECKSUMS 1u
typedef struct rc_container2_info {
  uint32_t version, kind, n_symbols, total_freq, increment, limit, period, reserved;
  uint64_t n_chunks, n_syms, payload_bytes;
  uint64_t table_off, index_off, payload_off, container_bytes;
  uint32_t n_models, first_row, flags, sym_bytes;
  uint64_t sum_off;
} rc_container2_info;
/* The rc_container2_* calls below take and fill an rc_container2_info through a void pointer
 * (info2): parse marks the struct it fills (reserved = the magic as a u32), and the calls that
 * read one return RC_E_ARG for a struct without the mark, an rc_container_info included.     */

/* Checksums of n_chunks chunks (device pointers; asynchronous and stream-ordered on the
 * context's stream, like rc_histogram).  off_dev: n_chunks + 1 offsets in symbols; sym_bytes 1 or
 * 2 (else RC_E_ARG); chunk k is the bytes [off[k] * sym_bytes, off[k+1] * sym_bytes) of data_dev,
 * which may start at any address.  sums_dev: n_chunks u32.  No byte outside the chunks is read.*/
rc_status rc_checksum_batch(rc_ctx* ctx, const void* data_dev, const uint64_t* off_dev,
                            uint32_t n_chunks, uint32_t sym_bytes, uint32_t* sums_dev);
/* Parse an RCB2 header (head_host: the first >= RC_CONTAINER_HEADER_BYTES bytes) into *info2.
 * RC_E_BAD_CONTAINER: wrong magic, version or header size, unknown kind, unknown flag bits,
 * n_symbols, n_models or first_row out of range, n_chunks > RC_MAX_CHUNKS, payload bytes not a
 * multiple of 16.                                                                           */
rc_status rc_container2_info_parse(const uint8_t* head_host, uint64_t head_len, void* info2);
/* rc_container_pack for RCB2: m is a static, adaptive, order-1 or wide model (RC_E_ARG for a
 * static set, which has no index stream to frame); sums_dev NULL (no checksum section) or
 * n_chunks u32 from rc_checksum_batch over the symbols.  Same size-query and capacity protocol:
 * *dst_len_host receives the size; RC_E_CAPACITY (nothing written) when it exceeds dst_cap or
 * dst_dev is NULL.  Synchronous.                                                            */
rc_status rc_container2_pack(rc_ctx* ctx, const rc_model* m, const uint8_t* slots_dev,
                             const uint64_t* slot_off_dev, const uint64_t* code_len_dev,
                             const uint64_t* sym_off_dev, uint32_t n_chunks,
                             const uint32_t* sums_dev, uint8_t* dst_dev, uint64_t dst_cap,
                             uint64_t* dst_len_host);
/* rc_container_offsets for RCB2: the same contract. */
rc_status rc_container2_offsets(rc_ctx* ctx, const uint8_t* container_dev, const void* info2,
                                uint64_t* code_off_dev, uint64_t* code_len_dev,
                                uint64_t* sym_off_dev);
/* The container's model, created from its table section by the rc_model_create_* call of its
 * kind (destroy it with rc_model_destroy).  A table that call rejects (a row that does not sum
 * to total_freq, a map entry >= n_models, ...) is RC_E_BAD_CONTAINER.  Synchronous.         */
rc_status rc_container2_model(rc_ctx* ctx, const uint8_t* container_dev, const void* info2,
                              rc_model** out);
/* Compare the checksums of decoded symbols (syms_dev: n_syms symbols of the container's symbol
 * size; sym_off_dev from rc_container2_offsets) with the stored ones.  RC_OK when the container
 * has no checksum section or every chunk matches; else RC_E_CHECKSUM with the lowest
 * mismatching chunk in *first_bad_host.  Synchronous.                                       */
rc_status rc_container2_verify(rc_ctx* ctx, const uint8_t* container_dev, const void* info2,
                               const void* syms_dev, const uint64_t* sym_off_dev,
                               uint64_t* first_bad_host);

#ifdef __cplusplus
}
#endif
#endif /* RANGE_CODER_AMD_H */
