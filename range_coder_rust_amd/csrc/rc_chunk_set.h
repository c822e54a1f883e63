// rc_chunk_set.h — static chunk sets: K static tables of one total, one per
// chunk class.  A launch is grouped by class on the device (rc_chunk_set.hip), so that every
// workgroup holds chunks of one class, stages that class's tables and runs the single-table
// symbol step of k_encode_static / k_decode_static unchanged (their grouped instantiations).
#pragma once
#include "rc_static.h"

// What a grouped coder kernel reads beside its ModelArgs (row 0's): the launch's grouping and the
// distance between two rows' tables.  `tab` rows are 256 entries apart.
struct GroupArgs {
  const u32* order;   // [grid * W] the chunk of every lane slot; ~0u: a dead lane
  const u32* wg_row;  // [grid] the class of every workgroup; ~0u: an unused workgroup
  u32 lut_stride;     // u32 words between two rows' `lut`
  u32 symof_stride;   // bytes between two rows' `symof` (0: the class has none)
};

// A chunk set's shape as the launchers need it (rc_model::cset)
struct ChunkSetArgs {
  u32 k;             // rows (1 .. RC_MAX_SET_MODELS)
  u32 lut_stride;    // as GroupArgs
  u32 symof_stride;
  u32 smv;           // the encoder variant: 2 when every row is complete, else 1
};

// The context's grouping scratch (order, wg_row, the tile counts), grown on demand.  It is the one
// piece of device state a batch call rewrites, and a context may change streams between two calls
// (rc_ctx_set_stream; the Python wrappers bind torch's current stream): `done` is recorded behind
// every grouped coder launch, and a launch on another stream than the last waits for it before it
// regroups, so the earlier coder has read order[] and wg_row[] by then.  Growing frees and
// allocates in stream order (no device-wide synchronise, and legal under stream capture).
struct GroupScratch {
  void* buf = nullptr;
  size_t cap = 0;
  hipStream_t last = nullptr;  // the stream of the last grouped launch (valid with `used`)
  hipEvent_t done = nullptr;   // recorded on `last` behind that launch's coder kernel
  bool used = false;
  u32 last_w = 0, last_lut = 0, last_grid = 0;  // what the last coder launch took (rc_chunk_last_)
};

// chunks per counting tile: one wave counts (then scatters) a tile in rounds of 64
#define GROUP_TILE 2048u

// workgroups of a grouped launch of n chunks in K classes at W lanes: every class is padded to
// whole workgroups, so at most K are partly filled; a bound the host knows without the counts
static inline u32 rc_group_grid(u32 n, u32 K, u32 W) { return (n + W - 1) / W + K; }

// rc_chunk_set.hip.  Groups the launch on `stream` (counts per tile, one scan, a stable scatter:
// three short kernels and a fill, none waiting for another workgroup) and returns the device
// arrays in *ga (strides untouched).  A chunk with class_of >= K appears nowhere in the order;
// its flags entry gets RC_F_BAD_MODEL and, where out_len is given, its length 0.
hipError_t rc_chunk_group_launch(hipStream_t stream, GroupScratch& sc, const uint8_t* class_of,
                                 u32 n, u32 K, u32 W, u32* flags, u64* out_len, GroupArgs* ga);

// rc_chunk_set.hip.  Behind the coder kernel of a grouped launch: records sc.done on `stream` and
// notes the launch's lanes per workgroup, variant (decoder: the LUT; encoder: 0) and grid.
hipError_t rc_chunk_group_done(hipStream_t stream, GroupScratch& sc, u32 W, u32 lut, u32 grid);
// rc_ctx_destroy's: waits for the last grouped launch and frees the scratch and the event
void rc_chunk_group_release(GroupScratch& sc);

// the grouped coders (rc_chunk_set.hip: the encoder; rc_decode_grouped_{pow2,magic}.hip).  `a`:
// row 0's ModelArgs.  The launchers' choices are the static launchers', taken for the padded
// workgroup count.
hipError_t rc_chunk_encode_launch(hipStream_t stream, const RcKnobs& k, const ModelArgs& a,
                                  int div, const ChunkSetArgs& cs, GroupScratch& sc,
                                  const uint8_t* class_of, const uint8_t* syms, const u64* sym_off,
                                  u32 n_chunks, uint8_t* out, const u64* out_off, u64* out_len,
                                  u32* flags);
hipError_t rc_chunk_decode_launch_pow2(hipStream_t stream, const RcKnobs& k, const ModelArgs& a,
                                       const ChunkSetArgs& cs, GroupScratch& sc,
                                       const uint8_t* class_of, const uint8_t* code,
                                       const u64* code_off, const u64* code_len,
                                       uint8_t* syms_out, const u64* sym_off, u32 n_chunks,
                                       u32* flags);
hipError_t rc_chunk_decode_launch_magic(hipStream_t stream, const RcKnobs& k, const ModelArgs& a,
                                        const ChunkSetArgs& cs, GroupScratch& sc,
                                        const uint8_t* class_of, const uint8_t* code,
                                        const u64* code_off, const u64* code_len,
                                        uint8_t* syms_out, const u64* sym_off, u32 n_chunks,
                                        u32* flags);
// the decoder variant and workgroup size such a launch takes (rc_chunk_set_plan_): the LUT in
// *lut, returns the lanes per workgroup when the direct q-to-symbol table is not taken
u32 rc_chunk_decode_class(const ModelArgs& a, int* lut);
