// rc_wide16.h — wide16 static models (rc_model_create_static_wide16): one static table over an
// alphabet of up to RC_MAX_WIDE16_SYMBOLS (2^16) 16-bit symbols, and the batch coders for it
// (rc_encode_batch_wide16 / rc_decode_batch_wide16; kernels in rc_wide16.hip).
//
// The regime is the wide models' (rc_wide.h: 256 <= total <= 2^16, at most 3 bytes settled per
// symbol), but the tables do not fit a CU's LDS: they stay in device memory (rc_wide16_tables.h
// builds them: at most 512 KiB of encoder entries, 128 KiB of q-to-symbol halfwords and a cum
// row) and are served from the L2.  The encoder's LDS holds the rings alone: 1,024 lanes per
// workgroup at every alphabet.  The decoder's workgroup stages the q-to-symbol halfwords in LDS
// in front of its rings (RC_W16_SYMOF_LDS; 0: read from device memory too), which leaves 384
// lanes above a total of 2^15.
#pragma once
#include "rc_indexed.h"

#ifndef RC_W16_SYMOF_LDS
#define RC_W16_SYMOF_LDS 1
#endif

// What the launchers use (rc_wide16_plan; rc_model_wide16_plan_ reports it in the plan hooks' 8
// words: the table layout is 0, the table bytes are the encoder's entries in device memory, and
// the decoder's bits / shift describe the q-to-symbol table: 2^bits entries, shift 0)
struct Wide16Plan {
  u32 enc_lanes;   // lanes per workgroup
  u32 enc_lds;     // dynamic LDS bytes of the workgroup: the rings alone
  u32 enc_layout;  // 0: 8-B (cum | flag << 24, c) entries
  u32 enc_tab;     // bytes of the encoder's entries in device memory (none of them in LDS)
  u32 dec_lanes;
  u32 dec_lds;     // the q-to-symbol table's bytes (RC_W16_SYMOF_LDS) and the rings
  u32 dec_bits;    // log2 of the q-to-symbol table's entries (2 B each)
  u32 dec_shift;   // 0: one entry per q
};
void rc_wide16_plan(u32 n_symbols, u32 total, Wide16Plan* p);

struct Wide16Args {
  ModelArgs m;            // n, total, range_par_total's constants, ftotal, the launch's priorities
  const uint2* enc;       // encoder entries (device), rc_wide16_tables.h
  const uint16_t* symof;  // [qmask + 1] q-to-symbol (device)
  const u32* row;         // cum[0 .. n + 1] (device): cum[n] = cum[n + 1] = total
  u32 enc_clamp;          // the entry index a symbol is clamped to
  u32 qmask;              // the q-to-symbol table's index mask
};

hipError_t rc_wide16_encode_launch(hipStream_t stream, const RcKnobs& k, const Wide16Args& a,
                                   int div, const Wide16Plan& p, const uint16_t* syms,
                                   const u64* sym_off, u32 n_chunks, uint8_t* out,
                                   const u64* out_off, u64* out_len, u32* flags);
hipError_t rc_wide16_decode_launch(hipStream_t stream, const RcKnobs& k, const Wide16Args& a,
                                   int div, const Wide16Plan& p, const uint8_t* code,
                                   const u64* code_off, const u64* code_len, uint16_t* syms_out,
                                   const u64* sym_off, u32 n_chunks, u32* flags);
// the lanes per workgroup of the last wide16 encode / decode launch of this process (test hook)
extern "C" void rc_wide16_last_lanes_(uint32_t* out2);
