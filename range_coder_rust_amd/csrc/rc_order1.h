// rc_order1.h — order-1 sets (rc_model_create_order1_set): the K rows of a static model set
// (rc_indexed.h) plus a context map, and batch coders in which the previous symbol of the chunk
// picks the row: row_0 = first_row, row_i = ctx_map[sym[i-1]] (rc_encode_batch_order1 /
// rc_decode_batch_order1; kernels in rc_order1.hip).
//
// Everything the set's kernels rely on holds unchanged (one total, at most 3 bytes settled per
// symbol, one workgroup per CU staging the rows once).  What is new is the map in LDS, staged as
// premultiplied LDS offsets so that the row of the next symbol costs one dependent LDS read:
//   encoder: 256 x u32, the byte offset of the row (in the place of the indexed encoder's poison
//            row K, which an order-1 set cannot reach: the map is validated at creation), so the
//            encoder's LDS plan is the set's;
//   decoder: 256 x u32 behind the rows, (row byte address >> 2) | (bucket base in words << 16),
//            1 KiB more than the set's plan, counted by rc_order1_plan.
#pragma once
#include "rc_indexed.h"

#define O1_MAP_BYTES 1024u  // 256 premultiplied u32 entries

// Periodic order-1 sets (rc_model_create_order1_set_periodic): the position in a
// record joins the context, row_i = ctx_map[(i mod P) * n_symbols + sym[i-1]] with P in {1, 2, 4,
// 8}.  P == 1 is the set above in every respect.  For P > 1 both kernels stage P maps of 256
// words, slice ph behind slice ph - 1:
//   encoder: P KiB of its own behind the K rows (the indexed encoder's spare row K holds one map,
//            not P), so the lanes and the layout are recomputed per (K, total, P);
//   decoder: P KiB behind the rows in the place of the one.
#define O1_MAX_PERIOD 8u
static inline bool o1_period_ok(u32 period) {
  return period == 1 || period == 2 || period == 4 || period == 8;
}

// The plan of a set of n_models rows coded with `period` maps.  Period 1: the set's plan with the
// decoder's map counted in (enc_*: exactly rc_set_plan's); a period that is not one of 1, 2, 4, 8
// leaves the plan zeroed.
void rc_order1_plan(u32 n_models, u32 total, u32 period, SetPlan* p);

// Lagged sets (rc_model_create_order1_set_lagged): the context is the symbol D
// positions back, row_i = ctx_map[(i mod P) * n_symbols + sym[i-D]] for i >= D and first_row for
// i < D, D in {1, 2, 4, 8} whatever P.  D == 1 is the set above in every respect.  The lag is a
// compile-time constant of the kernels and no field of O1Args (the arguments of the lag-1 kernels
// stay as they are): the model keeps it and hands it to the launchers.  A lagged set stages the
// maps as a periodic set does and carries D contexts in registers, so its plan is the plan of its
// (K, total, P).
static inline bool o1_lag_ok(u32 lag) { return o1_period_ok(lag); }

struct O1Args {
  SetArgs s;           // the rows and buckets, built for rc_order1_plan's dec_bits
  const uint8_t* map;  // [period][256] rows (device): slice ph = the map of the symbols i with
                       // i mod period == ph, entries from n_symbols on = 0
  u32 first_row;       // the row of every chunk's first symbol
  u32 period;          // 1, 2, 4 or 8 (> 1: the launchers take the kernels that stage every slice)
};

// the launchers of one lag > 1 each, defined by rc_order1_lag{2,4,8}.hip (rc_order1_lag.inc)
template <int LAG>
hipError_t rc_order1_encode_launch_lag(hipStream_t stream, const RcKnobs& k, const O1Args& a,
                                       int div, const SetPlan& p, const uint8_t* syms,
                                       const u64* sym_off, u32 n_chunks, uint8_t* out,
                                       const u64* out_off, u64* out_len, u32* flags);
template <int LAG>
hipError_t rc_order1_decode_launch_lag(hipStream_t stream, const RcKnobs& k, const O1Args& a,
                                       int div, const SetPlan& p, const uint8_t* code,
                                       const u64* code_off, const u64* code_len,
                                       uint8_t* syms_out, const u64* sym_off, u32 n_chunks,
                                       u32* flags);

// lag: the set's (1: the kernels of the period alone; else the call goes to the lag's unit)
hipError_t rc_order1_encode_launch(hipStream_t stream, const RcKnobs& k, const O1Args& a, u32 lag,
                                   int div, const SetPlan& p, const uint8_t* syms,
                                   const u64* sym_off, u32 n_chunks, uint8_t* out,
                                   const u64* out_off, u64* out_len, u32* flags);
hipError_t rc_order1_decode_launch(hipStream_t stream, const RcKnobs& k, const O1Args& a, u32 lag,
                                   int div, const SetPlan& p, const uint8_t* code,
                                   const u64* code_off, const u64* code_len, uint8_t* syms_out,
                                   const u64* sym_off, u32 n_chunks, u32* flags);
