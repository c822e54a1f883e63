// rc_stream_dev.h — device code shared by the resumable-stream units (rc_resume.hip, rc_rows.hip;
// DESIGN.md §9.19): the coder step up to the renormalisation loops, the byte count of those
// loops, and the whole encoder body.  Each is defined here and nowhere else, so a change to a
// flag or an overflow branch reaches every stream kernel.  (rc_host.h stays the one internal host
// header, §9.16; this one is device code on top of it.)
//
// The arithmetic is the reference's, branch for branch, with its panics and endless loops turned
// into sticky flags:
//   total == 0                       -> RC_F_BAD_MODEL (u64 / 0, range_coder.rs:38-40)
//   low + r*cum overflows            -> RC_F_BAD_MODEL (LowerBoundOverflow, :68-81)
//   range == r*c == 0                -> RC_F_ZERO_FREQ / RC_F_CORRUPT (:83-85 never ends)
//   low + range overflows            -> RC_F_BAD_MODEL (upper_bound().unwrap(), :138-146)
//   decoder needs a byte past the end -> RC_F_TRUNCATED (pop_front().unwrap(), decoder.rs:33)
// u64 products wrap (release-build semantics of the reference).
#pragma once
#include "rc_host.h"
#include "rc_udiv.h"

#define RWG 64
#define TOP8 (1ull << 56)  // range_coder.rs:23

namespace {

// RangeCoder::param_update up to the renormalisation loops: the narrowed interval, or a flag
struct Narrow {
  u64 low, range;
  u32 err;
};

// (r = range_par_total, range_coder.rs:38-40)
static __device__ __forceinline__ Narrow narrow_r(u64 low, u64 range, u64 r, u32 c, u32 cum,
                                                  u32 zero_flag) {
  Narrow o{low, range, 0u};
  const u64 nr = r * (u64)c;     // range_coder.rs:65
  const u64 add = r * (u64)cum;  // :68
  const u64 nl = low + add;
  if (nl < add) o.err = RC_F_BAD_MODEL;          // overflowing_add -> Err (:68-81)
  else if (nr == 0) o.err = zero_flag;           // no_carry_expansion never terminates
  else if (nl + nr < nr) o.err = RC_F_BAD_MODEL;  // upper_bound() overflow (:138-146)
  o.low = nl;
  o.range = nr;
  return o;
}
static __device__ __forceinline__ Narrow narrow(u64 low, u64 range, u32 c, u32 cum, u32 total,
                                                u32 zero_flag) {
  if (total == 0) return Narrow{low, range, RC_F_BAD_MODEL};  // range_par_total divides by 0
  return narrow_r(low, range, rc_udiv64(range, total), c, cum, zero_flag);
}

// bytes the two renormalisation loops settle from (low, range), without applying them
static __device__ __forceinline__ u32 settle_count(u64 low, u64 range) {
  u32 k = 0;
  while (((low ^ (low + range)) >> 56) == 0) {  // no_carry_expansion (:110-116)
    low <<= 8;
    range <<= 8;
    ++k;
  }
  while (range < TOP16) {  // range_reduction_expansion (:126-135)
    range = ~low & (TOP16 - 1);
    low <<= 8;
    range <<= 8;
    ++k;
  }
  return k;
}

// byte store into the body's block: global memory (the launch paths) or LDS (the service; the
// pointer is generic, derived from the LDS block, and the compiler infers the address space)
template <bool kLds>
static __device__ __forceinline__ void bstore(uint8_t* p, u32 v) {
  if constexpr (kLds) *p = (uint8_t)v;
  else gstore8(p, v);
}

// Encoder::encode x n (+ finish) for stream k: the body of every stream encoder.
// step(low, range, s0, i) -> Narrow is symbol s0 + i's param_update up to the loops; what it
// reads (a triple, a table row) and which flags it raises before narrowing are the caller's.
template <bool kLds, class Step>
static __device__ __forceinline__ void stream_encode_body(
    u32 k, rc_stream_state* __restrict__ st, const u64* __restrict__ sym_off,
    uint8_t* __restrict__ out, const u64* __restrict__ out_off, u64* __restrict__ out_len,
    uint8_t* __restrict__ nbytes, u32 finish, u32* __restrict__ flags, Step step) {
  rc_stream_state S = st[k];
  const u64 s0 = sym_off[k], n = sym_off[k + 1] - s0;
  uint8_t* o = out + out_off[k];
  const u64 cap = out_off[k + 1] - out_off[k];
  out_len[k] = 0;
  if (S.flags) {  // the reference panicked (or hung) at an earlier call
    flags[k] = S.flags;
    return;
  }
  if (S.stage == 2) {  // Encoder::finish took the encoder by value (encoder.rs:40)
    S.flags = RC_F_FINISHED;
    st[k] = S;
    flags[k] = S.flags;
    return;
  }
  if (cap < RC_STREAM_MAX_BYTES(n, finish)) {  // not sticky: the caller retries, nothing changed
    flags[k] = RC_F_CAPACITY;
    return;
  }
  u64 low = S.lower_bound, range = S.range, w = 0;
  for (u64 i = 0; i < n; ++i) {  // Encoder::encode (encoder.rs:24-37)
    const Narrow q = step(low, range, s0, i);
    if (q.err) {
      S.flags = q.err;
      break;
    }
    low = q.low;
    range = q.range;
    u32 nb = 0;
    while (((low ^ (low + range)) >> 56) == 0) {  // no_carry_expansion (:110-116)
      bstore<kLds>(o + w++, (u32)(low >> 56));  // left_shift (:95-100)
      low <<= 8;
      range <<= 8;
      ++nb;
    }
    while (range < TOP16) {  // range_reduction_expansion (:126-135)
      range = ~low & (TOP16 - 1);
      bstore<kLds>(o + w++, (u32)(low >> 56));
      low <<= 8;
      range <<= 8;
      ++nb;
    }
    if (nbytes) bstore<kLds>(nbytes + s0 + i, nb);  // encode()'s return value (encoder.rs:34-36)
    S.n += 1;
  }
  if (finish && !S.flags) {  // Encoder::finish: 8 x left_shift (encoder.rs:40-46)
    for (int j = 0; j < 8; ++j) {
      bstore<kLds>(o + w++, (u32)(low >> 56));
      low <<= 8;
      range <<= 8;
    }
    S.stage = 2;
  } else if (S.stage == 0) {
    S.stage = 1;
  }
  S.lower_bound = low;
  S.range = range;
  S.pos += w;
  st[k] = S;
  out_len[k] = w;
  flags[k] = S.flags;
}

}  // namespace
