// rc_wide.h — wide static models (rc_model_create_static_wide): one static table over an
// alphabet of up to RC_MAX_WIDE_SYMBOLS 16-bit symbols, and the batch coders for it
// (rc_encode_batch_wide / rc_decode_batch_wide; kernels in rc_wide.hip).
//
// A wide table is the small-model regime of DESIGN.md §3 (256 <= total <= 2^16, at most 3 bytes
// settled per symbol, so the margins of both rings hold as they are) with a table too large for
// the single-table coders' 256 entries.  Its LDS shape is that of a model set (rc_indexed.h): up
// to 32 KiB of table beside the rings, so all the lanes a CU holds run as ONE workgroup that
// stages the table once, and the plan below picks the lanes per workgroup, the encoder's table
// layout and the decoder's buckets from n_symbols.
#pragma once
#include "rc_indexed.h"

// What the launchers use for a wide table (rc_wide_plan; rc_model_wide_plan_ reports it)
struct WidePlan {
  u32 enc_lanes;   // lanes per workgroup, a multiple of 64
  u32 enc_lds;     // dynamic LDS bytes of the workgroup
  u32 enc_layout;  // 0: n + 1 8-B (cum | flag << 24, c) entries, entry n the poison entry a
                   //    symbol >= n is clamped to; 1: a cum-only row of n + 2 words with
                   //    cum[n] = cum[n + 1] = total, so a symbol past the alphabet reads c = 0
  u32 enc_tab;     // bytes of the table, rounded up to the rings' 1-KiB alignment
  u32 dec_lanes;
  u32 dec_lds;
  u32 dec_bits;    // log2 of the decoder's buckets (4 B each)
  u32 dec_shift;   // bucket = q >> dec_shift
};
void rc_wide_plan(u32 n_symbols, u32 total, WidePlan* p);

struct WideArgs {
  ModelArgs m;      // n, total, range_par_total's constants, ftotal, the launch's priorities
                    // (lut_bits / lut_shift: the buckets; the table pointers are unused)
  const u32* row;   // cum[0 .. n + 1] (device): cum[n] = cum[n + 1] = total
  const u32* lut;   // [1 << lut_bits] buckets s_lo | s_hi << 16 (device): find_index of the
                    // bucket's first and last frequency
  u32 top_stride;   // first stride of the bucket search: the largest power of two below the
                    // widest bucket's symbol count (0: every bucket names one symbol)
  u32 tab_bytes;    // encoder: WidePlan::enc_tab
};

hipError_t rc_wide_encode_launch(hipStream_t stream, const RcKnobs& k, const WideArgs& a, int div,
                                 const WidePlan& p, const uint16_t* syms, const u64* sym_off,
                                 u32 n_chunks, uint8_t* out, const u64* out_off, u64* out_len,
                                 u32* flags);
hipError_t rc_wide_decode_launch(hipStream_t stream, const RcKnobs& k, const WideArgs& a, int div,
                                 const WidePlan& p, const uint8_t* code, const u64* code_off,
                                 const u64* code_len, uint16_t* syms_out, const u64* sym_off,
                                 u32 n_chunks, u32* flags);
