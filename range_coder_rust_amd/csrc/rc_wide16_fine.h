// rc_wide16_fine.h — wide16 fine models (rc_model_create_static_wide16_fine): one static table over
// an alphabet of up to RC_MAX_WIDE16_SYMBOLS (2^16) 16-bit symbols whose total lies above 2^16, up
// to RC_MAX_WIDE16_FINE_TOTAL (2^24), and the kernels the wide16 batch calls run for such a model
// (k_encode_wide16_fine / k_decode_wide16_fine, rc_wide16_fine.hip).
//
// The regime is the wide one of the 8-bit static coders (SM = 0 in rc_encode.inc / rc_decode.inc:
// 64-bit products, a symbol may settle 4 bytes by no_carry_expansion and 7 more by
// range_reduction_expansion, the decoder keeps DEC_NEED_WIDE bytes staged before every symbol).
// The tables stay in device memory as the wide16 models' do (rc_wide16_fine_tables.h builds them:
// at most 512 KiB of encoder entries, and for the decoder the occupied symbols, their cum row and
// a bucket table over the top bits of q).  The decoder's workgroup stages the bucket table in LDS
// in front of its rings: 2^RC_W16F_BITS buckets (DESIGN.md §9.22 has both forms measured).
#pragma once
#include "rc_wide16.h"

// log2 of the decoder's bucket count: 16 (128 KiB of table, 384 lanes per workgroup, the form
// kept: the faster one at 2^16 chunks of 16 Ki symbols) or, for scratch builds, 15 (64 KiB, 1,024
// lanes, twice the ranks per bucket)
#ifndef RC_W16F_BITS
#define RC_W16F_BITS 16
#endif
static_assert(RC_W16F_BITS == 15 || RC_W16F_BITS == 16, "2^15 or 2^16 buckets");

// the bucket table's bytes in LDS: 2^bits halfwords, the sentinel, padded to 16 B
#define RC_W16F_BUCKET_LDS ((2u << RC_W16F_BITS) + 16u)

// (Wide16Plan's fields; the decoder's bits / shift describe the bucket table)
void rc_wide16_fine_plan(u32 n_symbols, u32 total, Wide16Plan* p);

struct Wide16FineArgs {
  ModelArgs m;             // n, total, range_par_total's constants, ftotal, the priorities
  const uint2* enc;        // encoder entries (cum, c) (device), rc_wide16_fine_tables.h
  const u32* rcum;         // [n_occ + 2] cum of the occupied symbols, then the total twice
  const uint16_t* occ;     // [n_occ] the occupied symbols
  const uint16_t* bucket;  // [2^RC_W16F_BITS + 2] rank of the bucket's first q
  u32 enc_clamp;           // the entry index a symbol is clamped to
  u32 shift;               // bucket = q >> shift
  u32 qmax;                // total - 1
};

hipError_t rc_wide16_fine_encode_launch(hipStream_t stream, const RcKnobs& k,
                                        const Wide16FineArgs& a, int div, const Wide16Plan& p,
                                        const uint16_t* syms, const u64* sym_off, u32 n_chunks,
                                        uint8_t* out, const u64* out_off, u64* out_len,
                                        u32* flags);
hipError_t rc_wide16_fine_decode_launch(hipStream_t stream, const RcKnobs& k,
                                        const Wide16FineArgs& a, int div, const Wide16Plan& p,
                                        const uint8_t* code, const u64* code_off,
                                        const u64* code_len, uint16_t* syms_out,
                                        const u64* sym_off, u32 n_chunks, u32* flags);
// the lanes per workgroup of the last fine encode / decode launch of this process (test hook)
extern "C" void rc_wide16_fine_last_lanes_(uint32_t* out2);
