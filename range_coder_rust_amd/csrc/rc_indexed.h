// rc_indexed.h — static model sets (rc_model_create_static_set): K static tables over one
// alphabet and one total_freq, and batch coders that take one model index per symbol
// (rc_encode_batch_indexed / rc_decode_batch_indexed; kernels in rc_indexed.hip).
//
// The set is the small-model regime of DESIGN.md §3 (256 <= total <= 2^16) with a table base that
// changes per symbol.  The total is shared, so range / total is computed once per symbol whatever
// the row and the decoder's carried hint scale G = total / (range / 2^32) does not depend on the
// row; at most 3 bytes settle per symbol, so the margins of both rings hold as they are.
//
// What limits the design is LDS (160 KiB per CU): the encoder's rings cost 148 B per lane and the
// decoder's 72 B, and K tables have to sit beside them.  All the lanes a CU holds therefore run as
// ONE workgroup that stages the K tables once, and the plan below picks the lanes per workgroup
// and the table layout from K.
#pragma once
#include "rc_static.h"

#define SET_ROW_WORDS 257u  // a cum-only row: cum[0 .. 256], entries from n_symbols on = total
#define SET_LDS_BYTES 163840u  // LDS of one gfx950 CU
#define SET_ENC_LANE_BYTES 148u  // encoder: 128-B ring + 16-B EncOut + 4-B rank slot per lane
#define SET_DEC_LANE_BYTES (4u * DEC_RING_ALLOC)  // decoder: the code ring and its mirror

// What the launchers use for a set of K models (rc_set_plan; rc_model_set_plan_ reports it)
struct SetPlan {
  u32 enc_lanes;   // lanes per workgroup, a multiple of 64
  u32 enc_lds;     // dynamic LDS bytes of the workgroup
  u32 enc_layout;  // 0: K + 1 rows of 256 8-B (cum, c) entries; 1: K + 1 cum-only rows
                   //    (c = cum[s + 1] - cum[s] from one two-dword read); row K is the poison
                   //    row an index >= K is clamped to (every entry flagged)
  u32 enc_tab;     // bytes of the tables, rounded up to the rings' 1-KiB alignment
  u32 dec_lanes;
  u32 dec_lds;
  u32 dec_bits;    // log2 of the two-candidate buckets per row (4 B each)
  u32 dec_shift;   // bucket = q >> dec_shift
};
void rc_set_plan(u32 n_models, u32 total, SetPlan* p);

struct SetArgs {
  ModelArgs m;      // n, total, range_par_total's constants, ftotal, the launch's priorities
                    // (lut_bits / lut_shift: the rows' buckets; the table pointers are unused)
  const u32* rows;  // [k][SET_ROW_WORDS] cum rows (device)
  const u32* lut;   // [k][1 << lut_bits] buckets s0 | s1 << 8 | cum[s1] << 16 (device)
  u32 k;            // models in the set (1 .. RC_MAX_SET_MODELS)
  u32 tab_bytes;    // encoder: SetPlan::enc_tab
};

// shared with the wide coders (rc_wide.hip), whose workgroups are sized the same way (as is
// set_allow_lds, which rc_static.h declares): the lanes per workgroup of a launch of n_chunks
// chunks (the plan's, or fewer so that a small launch reaches every CU)
u32 set_launch_lanes(u32 plan_lanes, u32 n_chunks);

hipError_t rc_set_encode_launch(hipStream_t stream, const RcKnobs& k, const SetArgs& a, int div,
                                const SetPlan& p, const uint8_t* syms, const uint8_t* idx,
                                const u64* sym_off, u32 n_chunks, uint8_t* out,
                                const u64* out_off, u64* out_len, u32* flags);
hipError_t rc_set_decode_launch(hipStream_t stream, const RcKnobs& k, const SetArgs& a, int div,
                                const SetPlan& p, const uint8_t* code, const u64* code_off,
                                const u64* code_len, const uint8_t* idx, uint8_t* syms_out,
                                const u64* sym_off, u32 n_chunks, u32* flags);
