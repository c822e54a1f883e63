// rc_cuwg.inc — what the three coder families with one workgroup per CU share around their hot
// loops (rc_indexed.hip, rc_order1.hip, rc_wide.hip; included after rc_encode.inc and
// rc_decode.inc): the encoder's slot geometry, state and finish, the decoder's chunk flag, the
// table entry reads and the exact fix-up walk, and on the host the decoder's LDS plan and the
// launch.  The symbol, tile and phase loops, the table staging and the decoder's prologue stay in
// their files (DESIGN.md §9.9, which also gives the rule a change here is checked against).
#pragma once
#include <string.h>

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// the waves' rings, the lanes' output geometry and the waves' rank tables, behind the tables
struct CuwgEncLds {
  u32* ring;
  EncOut* out;
  u32* rank;
};
static __device__ __forceinline__ CuwgEncLds cuwg_enc_lds(u32* s_enc, u32 tab_bytes, u32 lanes) {
  CuwgEncLds l;
  l.ring = s_enc + tab_bytes / 4;
  l.out = reinterpret_cast<EncOut*>(l.ring + (lanes >> 6) * ENC_RING * 64);
  l.rank = reinterpret_cast<u32*>(l.out + lanes);
  return l;
}

// a lane's chunk and its output slot
struct CuwgChunk {
  u64 s0, n;      // first symbol, symbols (0 for a dead lane and for a chunk that is too long)
  u64 cap;        // writable bytes of the slot
  u32 al;         // pad bytes in front of the slot, down to the flush unit
  bool too_long;
};

// Chunk k's geometry, and the lane's EncOut entry written; the kernel's __syncthreads() follows.
static __device__ __forceinline__ CuwgChunk cuwg_enc_begin(EncOut* so, uint8_t* out,
                                                           const u64* sym_off,
                                                           const u64* out_off, u32 k, bool live) {
  CuwgChunk c;
  u64 o0 = 0, o1 = 0;
  c.s0 = 0;
  c.n = 0;
  if (live) {
    c.s0 = sym_off[k];
    c.n = sym_off[k + 1] - c.s0;
    o0 = out_off[k];
    o1 = out_off[k + 1];
  }
  // B (bit position) is 32-bit: a longer chunk is flagged, not read, and its slot not written
  c.too_long = c.n > RC_MAX_CHUNK_SYMBOLS;
  if (c.too_long) {
    c.n = 0;
    o1 = o0;
  }
  c.al = (u32)(((uintptr_t)out + o0) & (ENC_UNIT - 1));
  c.cap = o1 - o0;
  if (c.cap > 0xFFFFFF00ull - c.al) c.cap = 0xFFFFFF00ull - c.al;
  so->gbase = out + o0 - c.al;
  so->lo_ok = c.al;
  so->hi_ok = c.al + (u32)c.cap;
  return c;
}

static __device__ __forceinline__ void cuwg_enc_init(Enc& e, u32 al, u32 tab_bytes, u32 wave,
                                                     u32 lane) {
  e.low = 0;  // RangeCoder::default (range_coder.rs:13-20)
  e.range = ~0ull;
  e.acc = 0;
  e.B = 8 * al;  // pad bytes in front of the slot (never stored)
  e.fthr = 8u * FLUSH_AT;  // fpos = 0
  e.err = 0;
  e.ring = tab_bytes + 4u * (wave * ENC_RING * 64 + ring_col(lane));
}

// The tiles every live lane of the wave has (0 without a live lane): the wave-uniform (scalar)
// trip count of the loop that runs with every lane active.
static __device__ __forceinline__ u32 cuwg_tmin(bool live, u32 ntile) {
  u32 tm = live ? ntile : ~0u;
#pragma unroll
  for (int o = 32; o; o >>= 1) tm = min(tm, (u32)__shfl_xor((int)tm, o));
  if (tm == ~0u) tm = 0;  // no live lane in this wave
  return __builtin_amdgcn_readfirstlane(tm);
}

// Encoder::finish (encoder.rs:40-46): 8 x left_shift, the last partial dword and the final flush
// rounds, clipped to the stream end.  Returns the stream's length in bytes.
static __device__ __forceinline__ u32 cuwg_enc_finish(Enc& e, EncOut* so, u32 al, u32 lane,
                                                      const u32* wring, const EncOut* wout,
                                                      u32* wrank) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    enc_emit_byte(e, (u32)(e.low >> 56));
    e.low <<= 8;
  }
  const u32 len = (e.B >> 3) - al;
  u32 wend = enc_wpos(e);
  if (e.B & 31) {  // the last, incomplete dword
    ring_put(e.ring, (e.B >> 5) & (ENC_RING - 1), (u32)(e.acc << (32 - (e.B & 31))));
    wend += 4;
  }
  // final rounds: the last (partial) units, clipped to the stream end
  const u32 end = al + len;
  if (end < so->hi_ok) so->hi_ok = end;
  while (__any((int)(enc_fpos(e) < wend)))
    enc_round(e, enc_fpos(e) < wend, lane, wring, wout, wrank);
  return len;
}

// a live lane's results; err: the family's *_first_error when the coder met a flagged entry
static __device__ __forceinline__ void cuwg_enc_report(const CuwgChunk& c, u32 k, u32 len,
                                                       u32 err, u64* out_len, u32* flags) {
  if (!err && (u64)len > c.cap) err = RC_F_CAPACITY;
  out_len[k] = c.too_long ? 0u : len;
  flags[k] = c.too_long ? RC_F_TOO_LONG : err;
}

// the (cum, c) entry of symbol s in the row at LDS byte offset ro, in enc_core's SM 1 form: a
// symbol the reference cannot encode carries a flag byte above its cum and c = 1.  Layout 0: the
// 8-B entry as staged, one ds_read_b64.  Layout 1: a cum-only row, c = cum[s + 1] - cum[s] (one
// ds_read2_b32); c = 0 covers zero frequencies, symbols past the alphabet (their cum is the
// total) and a poison row (zeros) alike.
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
template <int LAYOUT>
static __device__ __forceinline__ uint2 cuwg_enc_entry(u32 ro, u32 s) {
  if (LAYOUT == 0) {
    const u32x2 v = *(const __attribute__((address_space(3))) u32x2*)(uintptr_t)(ro + (s << 3));
    return make_uint2(v.x, v.y);
  }
  const l_u32* rp = (const l_u32*)(uintptr_t)(ro + (s << 2));
  const u32 c0 = rp[0], c1 = rp[1];
  const u32 c = c1 - c0;
  return make_uint2(c0 | ((c - 1u) & 0xFF000000u), max(c, 1u));
}

// ------------------------------------------------------------------------------------------
// Decoder
// ------------------------------------------------------------------------------------------

// (Decoder::new -- the two early exits, the state, the ring priming, set_data and the exact hint
// scale -- stays restated in the three kernels: moved into a helper here it changed the code of
// their loops' surroundings and cost the order-1 decoder 0.5 % at K = 64, DESIGN.md §9.9.)

// the chunk's flag: shift_left_buffer panics once more bytes are needed than the stream holds
// (decoder.rs:33)
template <class D>
static __device__ __forceinline__ u32 cuwg_dec_flag(D& d) {
  if (!d.err && d.bpos > d.limb) d.err = RC_F_TRUNCATED;
  return d.err;
}

// (cum, c) of symbol s from the cum-only row at LDS byte address rowa: c = cum[s + 1] - cum[s]
// (the row holds the total from its alphabet's end on), one ds_read2_b32
static __device__ __forceinline__ uint2 cuwg_cum_entry(u32 rowa, u32 s) {
  const l_u32* rp = (const l_u32*)(uintptr_t)(rowa + (s << 2));
  const u32 c0 = rp[0], c1 = rp[1];
  return make_uint2(c0, c1 - c0);
}

// dec_fix (rc_decode.inc) over a cum-only row: the exact index s = #{ j in [1, n-1] :
// r * cum[j] <= x } (FreqTable::find_index), walked from the candidate (down, it ends at s = 0
// at the latest: cum[0] = 0).  BYTE_SYM: one-byte symbols, the candidate masked to 8 bits first.
// dec_fix itself reads 8-B (cum, c) entries and stays as it is: both a second entry form selected
// by its template value and one shared walk taking a loader functor changed the generated code
// of every k_decode_static instantiation (disassembly diff), which must not change.
template <bool BYTE_SYM>
static __device__ __forceinline__ void cuwg_dec_fix(u32& s, uint2& t, u64& A, u64& B, u64 x,
                                                    u64 r, u32 rowa, u32 n) {
  if (BYTE_SYM) s &= 255u;
  if (A > x) {
    do {
      --s;
      t = cuwg_cum_entry(rowa, s);
      A = r * (u64)t.x;
    } while (A > x);
    B = r * (u64)t.y;
  } else {
    while (s + 1 < n && x - A >= B) {
      ++s;
      t = cuwg_cum_entry(rowa, s);
      A = r * (u64)t.x;
      B = r * (u64)t.y;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host: the decoder's LDS plan and the launch
// ------------------------------------------------------------------------------------------

// The decoder half of a plan (SetPlan / WidePlan): `fixed` bytes of rows (and map) and `tables`
// bucket tables of 2^bits 4-B buckets each beside the rings; bits is capped by 2^12 (the
// single-table decoders' finest) and by the total.  The first of 1,024, 768 and 512 lanes that
// leaves every table at least 2^min(cap, accept) buckets, else the one that leaves the most.
template <class Plan>
static void cuwg_dec_plan(Plan* p, u32 total, u32 fixed, u32 tables, u32 accept) {
  const u32 bl = bitlen(total - 1);
  const u32 cap = bl < 12u ? bl : 12u;
  u32 best_lanes = 0;
  int best = -1;
  for (u32 lanes = 1024; lanes >= 512; lanes -= 256) {
    int b = -1;
    for (u32 t = 0; t <= cap; ++t)
      if (fixed + lanes * SET_DEC_LANE_BYTES + tables * (4u << t) <= SET_LDS_BYTES) b = (int)t;
    if (b > best) {
      best_lanes = lanes;
      best = b;
    }
    if (b >= (int)(cap < accept ? cap : accept)) break;
  }
  p->dec_lanes = best_lanes;
  p->dec_bits = (u32)best;
  p->dec_shift = bl > p->dec_bits ? bl - p->dec_bits : 0u;
  p->dec_lds = fixed + tables * (4u << p->dec_bits) + best_lanes * SET_DEC_LANE_BYTES;
}

// One launch of `kern` over n_chunks chunks, one lane each: the lanes per workgroup
// (set_launch_lanes of the plan's), the plan's dynamic LDS less the lanes not run, the kernel
// allowed that much LDS, the launch's priorities into m (a member of a) and the launch itself.
template <class Kern, class Args, class... Rest>
static hipError_t cuwg_launch(Kern kern, hipStream_t stream, const RcKnobs& k, Args& a,
                              ModelArgs& m, PrioPolicy prio, u32 plan_lanes, u32 lane_bytes,
                              u32 plan_lds, u32 n_chunks, Rest... rest) {
  const u32 lanes = set_launch_lanes(plan_lanes, n_chunks);
  const u32 lds = plan_lds - (plan_lanes - lanes) * lane_bytes;
  const dim3 grid((n_chunks + lanes - 1) / lanes), block(lanes);
  const hipError_t lds_err = set_allow_lds(reinterpret_cast<const void*>(kern));
  if (lds_err != hipSuccess) return lds_err;
  rc_prio_policy(m, prio, grid.x,
                 rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)lanes, lds), k);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, a, rest...);
  return hipGetLastError();
}
