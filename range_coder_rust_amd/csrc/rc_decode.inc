// rc_decode.inc — k_decode_static, the static-model decoder; included by rc_decode_pow2.hip and
// rc_decode_magic.hip with RC_DEC_DIV set (see rc_static.h for the shared design notes).
#include "rc_static.h"
#include "rc_chunk_set.h"


// ------------------------------------------------------------------------------------------
// Decoder
//
// Per lane: one chunk.  The code stream is staged through a per-lane 64-B LDS ring (DEC_RING
// dwords, + DEC_MIRROR mirror dwords so a symbol's 2-3 dword window never wraps), refilled 32 B
// at a time from 64-B load bursts: at each 16-symbol phase boundary a lane commits the next
// 32 B of its pending burst into the ring if the ring has room, and issues the next burst once
// the pending one is used up, so a burst is waited for a phase or more after it was issued.
// Ring checks between phases (every DEC_CHECK_SPAN symbols) and after each rare path refill
// synchronously the lanes that could otherwise read past the staged bytes (DESIGN.md §5).
// ------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) u32 l_u32;

// RC_DEC_SHARED_ONLY (rc_indexed.hip): the per-lane machinery alone (code ring, dec_apply,
// dec_fix, dec_rare), without k_decode_static and its launchers
// RC_DEC_GROUPED (rc_decode_grouped_pow2.hip, rc_decode_grouped_magic.hip): the chunk sets'
// grouped instantiations of the decoder body and their launcher, without k_decode_static
#ifdef RC_DEC_SHARED_ONLY
#elif defined(RC_DEC_GROUPED) && RC_DEC_DIV == 0
#define RC_DEC_TU dec_grp_pow2
RC_STAMP_DEFINE(dec_grp_pow2)
#elif defined(RC_DEC_GROUPED)
#define RC_DEC_TU dec_grp_magic
RC_STAMP_DEFINE(dec_grp_magic)
#elif RC_DEC_DIV == 0  // (scratch -DRC_STAMP builds: one stamp buffer per translation unit)
#define RC_DEC_TU dec_pow2
RC_STAMP_DEFINE(dec_pow2)
#else
#define RC_DEC_TU dec_magic
RC_STAMP_DEFINE(dec_magic)
#endif

// Ring layout.  Column-major (round 4): a lane's dword j at LDS dword 64 j + lane of its wave's
// ring, stride 256 B, one and plus one v_lshl_add_u32 from bpos per symbol.  Rows (DEC_ROWS, the
// direct-table decoder): a wave's ring holds 8 lane groups of 1 KiB (lanes 8g .. 8g+7); in a
// group dword j is the 32-B row j (rows 16, 17 the mirror) and lane L's dword sits at byte
// 4 (L & 7) of it.  The column base has no bits in the row field (byte bits 5-8), so the
// symbol's ring address is base | (bpos & 0x1E0): one v_and_or_b32.  8 KiB per wave (4.5 KiB
// column-major): the direct-table workgroup takes 38 KiB, 4 per CU (4 waves per SIMD, and
// 2^20 chunks are 4 even rounds) instead of 5.
#ifndef DEC_ROWS
#define DEC_ROWS 0
#endif
#define DEC_ROW_WAVE_BYTES 8192u

template <int LD, int ROWS = 0>  // LD: 16-B blocks per load burst (DEC_LD, or per variant)
struct Dec {
  static constexpr int kLD = LD;
  static constexpr u32 kS = ROWS ? 8u : 64u;  // dwords between a lane's ring dwords j, j + 1
  u64 low, range;  // RangeCoder (decoder.rs:6-12)
  // Decoder::data (decoder.rs:6-12) itself; find_index wants x = data - lower_bound (mod 2^64,
  // sample_impl.rs:29), which the symbol step never forms whole: its hint takes x's high half
  // as hi(data) - hi(low) (one subtract; at most one too large, a hint), and its verification
  // x - r cum = data - (low + r cum) reuses the new lower bound, so no separate r cum product.
  // (The step builds the high half by a 64-bit shift, data << k8, and the low half by one
  // v_perm_b32 into the same register pair.)
  u64 dat;
  float G;  // 16-B direct tables: 16 * total / (range / 2^32), carried from symbol to symbol
  __device__ __forceinline__ u32 dhi() const { return hi32(dat); }
  __device__ __forceinline__ u64 data() const { return dat; }
  __device__ __forceinline__ void set_data(u64 v) { dat = v; }
  __device__ __forceinline__ u64 x() const { return dat - low; }
  // Stream positions are in BITS (byte-granular), relative to the 16-B aligned base of the code
  // stream: a symbol adds its k8 to bpos as it is, the ring dword is bpos >> 5, and
  // v_alignbit_b32 takes bpos & 31 directly.  (At most 2^29 code bytes are ever read: 8 + 12 n
  // for n <= 2^25 symbols, so bit positions fit 32 bits.)
  u32 bpos;   // bits consumed
  u32 fillb;  // bits staged into the ring
  u32 limb;   // bpos > limb: more bytes consumed than the stream holds
  u32 err;
#ifdef RC_FILL
  rc_fill_t fill;  // scratch builds: the filler instructions' register
#endif
  u32 pend_ok;           // 32-B refills still held in pend[] (a load burst gives LD / DEC_PF)
  l_u32* ring;           // this lane's ring column: dword j at ring[j * kS] (LDS pointer)
  const uint4* gbase;    // 16-B aligned base of the stream
  u32 gnext;             // next 16-B block (index from gbase)
  u32 glast;             // first block of the last load segment (fetch clamp, dec_issue)
  uint4 pend[LD];
};

template <class D>
static __device__ __forceinline__ void dec_issue(D& d) {
  // One 16 * LD-byte aligned segment per burst (gbase is that aligned, gnext a multiple of LD),
  // clamped as a whole to the segment that holds the stream's last byte (glast is the first
  // block of that segment): one v_min_u32 per burst, and the blocks load at immediate offsets.
  // The segment lies in the page of a byte of the stream, so its blocks past the stream's end
  // are mapped; their bytes are reached only by a decode already past the end (flagged
  // RC_F_TRUNCATED, like any read past limb).
  const uint4* p = d.gbase + min(d.gnext, d.glast);
#pragma unroll
  for (int q = 0; q < D::kLD; ++q) {
    const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)(p + q);  // global, not flat
    d.pend[q] = make_uint4(v.x, v.y, v.z, v.w);
  }
  d.gnext += D::kLD;
  d.pend_ok = D::kLD / DEC_PF;
}

// move the next DEC_PF pending blocks into the ring (pend[0..DEC_PF) hold them)
template <class D>
static __device__ __forceinline__ void dec_commit(D& d) {
  const u32 j = (d.fillb >> 5) & (DEC_RING - 1);
  constexpr u32 S = D::kS;
  l_u32* rp = d.ring + j * S;
#pragma unroll
  for (int q = 0; q < DEC_PF; ++q) {
    rp[(4 * q + 0) * S] = d.pend[q].x;
    rp[(4 * q + 1) * S] = d.pend[q].y;
    rp[(4 * q + 2) * S] = d.pend[q].z;
    rp[(4 * q + 3) * S] = d.pend[q].w;
  }
  if (j == 0) {  // mirror slots
    rp[DEC_RING * S] = d.pend[0].x;
    rp[(DEC_RING + 1) * S] = d.pend[0].y;
    if (DEC_MIRROR > 2) rp[(DEC_RING + 2) * S] = d.pend[0].z;
    if (DEC_MIRROR > 3) rp[(DEC_RING + 3) * S] = d.pend[0].w;
  }
#pragma unroll
  for (int q = 0; q + DEC_PF < D::kLD; ++q) d.pend[q] = d.pend[q + DEC_PF];
  d.fillb += 128 * DEC_PF;
  d.pend_ok -= 1;
}

// phase boundary: commit the pending load, issue the next one if the ring has room
// (the ring has room for a refill once at most 4 * DEC_RING - 16 * DEC_PF bytes are unread;
// a 64-B load burst feeds two refills, so every lane's global reads are whole 64-B segments)
template <class D>
static __device__ __forceinline__ void dec_phase(D& d) {
  if (d.pend_ok && (int)(d.fillb - d.bpos) <= 32 * DEC_RING - 128 * DEC_PF) dec_commit(d);
  if (!d.pend_ok) dec_issue(d);
}

// a lane about to read past the staged bytes: commit / load synchronously (rare)
template <class D>
static __device__ __forceinline__ void dec_sync(D& d, u32 need) {  // need: bytes
  while ((int)(d.fillb - d.bpos) < (int)(8 * need)) {
    if (!d.pend_ok) dec_issue(d);
    dec_commit(d);
  }
}

// the 8 code bytes ending at bpos, big-endian (Decoder::new's priming, decoder.rs:14-23)
template <class D>
static __device__ __forceinline__ u64 dec_read8_before(const D& d) {
  const u32 p = d.bpos - 64;
  const l_u32* rp = d.ring + ((p >> 5) & (DEC_RING - 1)) * D::kS;
  const u32 d0 = rp[0], d1 = rp[D::kS], d2 = rp[2 * D::kS];
  const u32 w0 = __builtin_amdgcn_alignbit(d1, d0, p);
  const u32 w1 = __builtin_amdgcn_alignbit(d2, d1, p);
  return ((u64)__builtin_bswap32(w0) << 32) | __builtin_bswap32(w1);
}

// range_reduction_expansion (range_coder.rs:126-135): each iteration settles one more byte,
// which Decoder::shift_left_buffer (decoder.rs:31-35) shifts into data (so into x = data-low)
template <class D>
static __device__ __forceinline__ void dec_rare(D& d, u32 need) {
  u32 m = 0;
  while (d.range < TOP16) {
    d.range = ~d.low & (TOP16 - 1);
    d.low <<= 8;
    d.range <<= 8;
    ++m;
  }
  dec_sync(d, m + need);
  for (u32 j = 0; j < m; ++j, d.bpos += 8) {
#ifdef RC_RING_GUARD
    if (d.bpos + 8 > d.fillb) d.err |= RC_F_RING_GUARD;
#endif
    const u32 w = d.ring[((d.bpos >> 5) & (DEC_RING - 1)) * D::kS];
    d.set_data((d.data() << 8) | ((w >> (d.bpos & 31u)) & 255u));
  }
}

// the exact index: s = #{ j in [1, n-1] : r * cum[j] <= x }  (FreqTable::find_index)
// (TS: u32 per (cum, c) table entry)
template <u32 TS>
static __device__ __forceinline__ void dec_fix(u32& s, uint2& t, u64& A, u64& B, u64 x,
                                                        u64 r, const u32* s_tab, u32 n) {
  s &= 255u;
  if (A > x) {
    do {
      --s;
      t = *(const uint2*)(s_tab + TS * s);
      A = r * (u64)t.x;
    } while (A > x);
    B = r * (u64)t.y;
  } else {
    while (s + 1 < n && x - A >= B) {
      ++s;
      t = *(const uint2*)(s_tab + TS * s);
      A = r * (u64)t.x;
      B = r * (u64)t.y;
    }
  }
}

// A VALU read of an SGPR (VCC included) that a VALU wrote needs 2 wait states on gfx950: hipcc
// puts an s_nop 1 between its own v_cmp -> v_cndmask_b32 pairs, and pads nothing inside an
// asm string.  The candidate selects below write VCC and read it in one asm block, so they
// carry the wait themselves (round 4 shipped them without it: a select that read a stale VCC
// took a wrong candidate, which the exact verification turned into a redo of the symbol, so
// the output stayed exact).  -DRC_NO_VCC_WAIT restores the round-4 form for A/B builds.
#ifdef RC_NO_VCC_WAIT
#define RC_VCC_WAIT ""
#else
#define RC_VCC_WAIT "s_nop 1\n\t"
#endif

// Decoder::decode (decoder.rs:38-54) with FreqTable::find_index (sample_impl.rs:27-45).
// SM: 256 <= total <= 2^16 (then range >= 2^32 after narrowing, so at most 3 bytes settle).
// u32 -> f32 as the single instruction; written out because hipcc otherwise widens a
// (float)hi32(v) back into its multi-instruction u64 -> f32 sequence
static __device__ __forceinline__ float cvt_f32(u32 v) {
  float f;
  asm("v_cvt_f32_u32 %0, %1" : "=v"(f) : "v"(v));
  return f;
}

// float -> u32 as the single instruction, which saturates (negative -> 0, >= 2^32 -> 2^32 - 1)
static __device__ __forceinline__ u32 cvt_u32_sat(float f) {
  u32 v;
  asm("v_cvt_u32_f32 %0, %1" : "=v"(v) : "v"(f));
  return v;
}

// floor(X * G) for 0 <= X * G < 2^22, plus 0x4B400000 (read the low 22 bits; every hint mask and
// field below stays under bit 22): one v_fma_f32 in place of v_mul_f32 + v_cvt_u32_f32.
// X * G + 1.5 * 2^23 lies in [2^23, 2^24), where a float's ulp is 1, and the decoder runs with
// f32 rounding toward zero (k_decode_static's prologue), so the sum lands on 1.5 * 2^23 +
// floor(X * G).  A larger product (corrupt input only) gives some other in-range hint.
static __device__ __forceinline__ u32 hint_floor(float X, float G) {
  // (a builtin, not inline asm: the hazard recognizer cannot see into asm and pads the next
  // dependent VOP1/VOP2 instruction with an s_nop)
  return __float_as_uint(__builtin_fmaf(X, G, 12582912.0f));
}

// Code bytes the ring must hold for the symbols up to the next ring check (DESIGN.md §5).
// SM models settle at most 3 bytes per symbol by no_carry_expansion and check the ring every
// DEC_CHECK_SPAN symbols inside a phase (every 4 in the head and tail), so a check stages
// 3 * DEC_CHECK_SPAN bytes.  A range_reduction_expansion of m <= 7 bytes inside a span stages
// m + DEC_NEED_SM before it reads its bytes: the rest of the span (at most DEC_CHECK_SPAN - 1
// symbols after the rare one) is then covered whatever the span offset.  dec_sync commits 32 B
// at a time while fewer than m + DEC_NEED_SM bytes are unread, which a 4 * DEC_RING-byte ring
// allows only while that need is at most 4 * DEC_RING - 32 (+1: the loop runs while short).
// Wide models check after every symbol (a symbol of theirs settles at most 5 bytes).
// (DEC_NEED_SM / DEC_NEED_SPAN are overridable for scratch RC_RING_GUARD builds only, which
// check that the guard fires where tests/ring_sim.py predicts an under-run.)
#ifndef DEC_NEED_SPAN
#define DEC_NEED_SPAN (3u * DEC_CHECK_SPAN)
#endif
#ifndef DEC_NEED_SM
#define DEC_NEED_SM (3u * DEC_CHECK_SPAN)
#endif
#ifndef DEC_NEED_WIDE
#define DEC_NEED_WIDE 8u
#endif
#define DEC_NEED_HEAD 12u  // the head and tail: a check every 4 symbols
static_assert(7u + DEC_NEED_SM <= 4u * DEC_RING - 32u + 1u,
              "rare-path ring need exceeds what a refill may stage");
static_assert(DEC_NEED_SPAN <= 4u * DEC_RING - 32u + 1u,
              "span ring need exceeds what a refill may stage");
static_assert(DEC_CHECK_SPAN == 4 || DEC_CHECK_SPAN == 8, "phase checks assume span 4 or 8");

// byte j of w = byte 0 of v, other bytes kept (j = 0: cleared): one v_mov_b32_sdwa
static __device__ __forceinline__ u32 put_byte(u32 w, u32 v, int j) {
  switch (j) {
    case 0:
      asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0"
          : "=v"(w) : "v"(v));
      break;
    case 1:
      asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0"
          : "+v"(w) : "v"(v));
      break;
    case 2:
      asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0"
          : "+v"(w) : "v"(v));
      break;
    default:
      asm("v_mov_b32_sdwa %0, %1 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0"
          : "+v"(w) : "v"(v));
  }
  return w;
}

// Decoders that carry the hint scale G from symbol to symbol instead of recomputing it: the
// 16-B direct tables (G = 16 total / (range / 2^32), the table's byte stride folded in) and the
// bucket tables of small models (G = total / (range / 2^32), with total / c per symbol in a 16-B
// (cum, c) table entry)
template <int SM, int LUT>
struct GCarry {
  static constexpr bool on =
      LUT == 2 || LUT == 5 || ((LUT == 0 || LUT == 3 || LUT == 4 || LUT == 6) && SM);
  static constexpr float scale = LUT == 2 ? 16.0f : 1.0f;
  static constexpr u32 tab_stride = ((LUT == 0 || LUT == 4 || LUT == 6) && SM) ? 4u : 2u;  // u32 per entry
};

// the carried hint scale, exactly (from the top 32 bits of range)
template <int SM, int LUT, class D>
static __device__ __forceinline__ void dec_gexact(D& d, const ModelArgs& m) {
  if (GCarry<SM, LUT>::on)
    d.G = (GCarry<SM, LUT>::scale * m.ftotal) * __builtin_amdgcn_rcpf(cvt_f32(hi32(d.range)));
}

// param_update (range_coder.rs:53-92) from the chosen symbol's products: L = low + r cum and
// B = r c; then the closed-form no_carry_expansion, the carried hint scale and
// shift_left_buffer's bytes into data (dat: data before the symbol).  D0..D2: the ring dwords at
// bpos.
template <int SM, int LUT, class D>
static __device__ __forceinline__ void dec_apply(D& d, u64 L, u64 B, u64 dat, float tc, u32 D0,
                                                 u32 D1, u32 D2) {
  typedef GCarry<SM, LUT> GC;
  // param_update (range_coder.rs:53-92); L = low + A
  d.low = L;
  d.range = B;
  // closed-form no_carry_expansion (DESIGN.md §3); SM: range >= 2^32 here, so the high halves
  // differ and k8 <= 24
  const u32 k8 = SM ? ((u32)__builtin_clz(hi32(d.low) ^ hi32(d.low + d.range)) & 24u)
                    : ((u32)__clzll(d.low ^ (d.low + d.range)) & 56u);
  d.low <<= k8;
  d.range <<= k8;
  // G * tc * 2^-k8 by the exponent field (G stays a normal float, ~2^-20 .. 2^-4)
  if (GC::on) {  // one v_mad_i32_i24 (from C: a shift and a subtract)
    u32 gb;
    asm("v_mad_i32_i24 %0, %1, %2, %3"
        : "=v"(gb) : "v"(k8), "s"(-(1 << 23)), "v"(__float_as_int(d.G * tc)));
    d.G = __int_as_float(gb);
  }
  // data' = data << k8 | the k8 / 8 code bytes at bpos (shift_left_buffer, decoder.rs:31-35):
  // the high half of data << k8, and the high half of (data_lo : next 4 code bytes) << k8
  // (alignbit uses bpos & 31 only)
  if (SM) {  // k8 = 8n <= 24
    // xl = data_lo << 8n | the n code bytes at bpos, first byte highest: ONE v_perm_b32 over
    // {data_lo, W} (W = the 4 code bytes at bpos, first byte in byte 0) whose selector is
    // hi32(0x0706050400010203 << 8n): byte j takes data_lo byte j - n (j >= n) or W byte
    // n - 1 - j (j < n).  (No byte swap, no register pair to assemble.)
    const u32 W = __builtin_amdgcn_alignbit(D1, D0, d.bpos);
    const u32 sel = hi32(0x0706050400010203ull << k8);
    // (the perm's output tied to the low half of data << k8, which it replaces: the new data
    // then stays in that register pair instead of costing a v_mov of the high half per symbol)
    const u64 t = dat << k8;
    u32 xl;
    asm("v_perm_b32 %0, %1, %2, %3" : "=v"(xl) : "v"((u32)dat), "v"(W), "v"(sel), "0"((u32)t));
    d.dat = (t & 0xFFFFFFFF00000000ull) | xl;
  } else {   // k8 <= 56
    const u32 w0 = __builtin_bswap32(__builtin_amdgcn_alignbit(D1, D0, d.bpos));
    const u64 b = ((u64)w0 << 32) | __builtin_bswap32(__builtin_amdgcn_alignbit(D2, D1, d.bpos));
    d.set_data((dat << k8) | (k8 ? b >> (64 - k8) : 0ull));
  }
#ifdef RC_RING_GUARD  // scratch builds: flag a symbol whose bytes reach past the staged ones
  if (d.bpos + k8 > d.fillb) d.err |= RC_F_RING_GUARD;
#endif
  d.bpos += k8;
}

template <int DIV, int SM, int LUT, class D>
static __device__ __forceinline__ u32 dec_sym(D& d, const ModelArgs& m, const u32* s_tab,
                                              const u32* s_lut) {
  typedef GCarry<SM, LUT> GC;
#ifdef RC_FILL
  RC_FILLER(d.fill);
#endif
  // the code bytes at bpos (the ring holds the ones this symbol can settle); they are shifted
  // into x at the end.  Ring dword (bpos >> 5) mod DEC_RING is at byte 256 (bpos >> 5) of the
  // lane's column: one and + one v_lshl_add_u32 from bpos (written out: from C the compiler
  // makes it a shift, an and and an add); in rows at byte 32 (bpos >> 5): one v_and_or_b32.
  // (SELFILL: the LUT 4 candidate select's two wait states hold the ring address and
  // range / total instead of an s_nop, so those two come from its asm block, below)
  constexpr bool SELFILL = DEC_SEL_FILL && LUT == 4 && DIV == DIV_POW2 && SM && D::kS == 64;
  u32 raddr = 0, roff = 0, D0 = 0, D1 = 0, D2 = 0;
  u64 r = 0;
  if (SELFILL) {
    asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
  } else {
    if (D::kS == 8) {
      raddr = (d.bpos & ((DEC_RING - 1) << 5)) | (u32)(uintptr_t)d.ring;
    } else {
      asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
      asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(raddr) : "v"(roff), "v"((u32)(uintptr_t)d.ring));
    }
    const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
    D0 = rp[0];
    D1 = rp[D::kS];
    D2 = SM ? 0u : rp[2 * D::kS];
    r = range_par_total<DIV, SM>(d.range, m);
  }
  // hint q ~ x / r ~ x * total / range from the top 32 bits of x and range.  Direct tables
  // (total <= 2048) take the high halves as they are: range >= 2^48, so the relative error is
  // <= 2^-15 (and ~2^-24 for the usual range >= 2^56), far inside one frequency step.  Bucket
  // tables (totals up to 2^32) first shift both by clz(range), for a relative error ~2^-22.
  // Small bucket models carry G too and take x's high half as it is: range is >= 2^56 after all
  // but ~1/256 of the symbols, so the hint's error stays far below a frequency step but for
  // those, where a miss only costs the exact fix-up.
  float X, R;
  if (GC::on) {
    // (a plain conversion of the u32 difference: no u64 for the compiler to widen it to, and no
    // asm for the hazard recognizer to pad)
    X = (float)(d.dhi() - hi32(d.low));
    R = 1.0f;  // unused: the scale G is carried
  } else if (LUT) {
    X = cvt_f32(d.dhi() - hi32(d.low));
    R = cvt_f32(hi32(d.range));
  } else {
    const u32 e = (u32)__builtin_clz(hi32(d.range));
    X = cvt_f32(hi32(d.x() << e));
    R = cvt_f32(hi32(d.range << e));
  }
  // The table index is masked, not clamped: the tables are padded to a power of two with valid
  // entries, so an out-of-range hint (corrupt streams, x >= range; or rounding to q == total)
  // only starts the exact fix-up below from another symbol, whose result does not depend on
  // where it starts.  (A v_mul_f32 clamp modifier was tried instead and gave wrong hints.)
  const float rR = GC::on ? 1.0f : __builtin_amdgcn_rcpf(R);
  u32 s;
  uint2 t;
  float tc = 0.0f;  // GC::on: total / c of the coded symbol, as a float
  if (LUT == 2) {  // 16-B direct entries {cum, c, s, total/c}: one ds_read_b128, no unpacking
    // G = 16 total / (range / 2^32) is not recomputed per symbol: range' = r c 2^k, so
    // G' = G (total / c) 2^-k (one multiply, one ldexp instead of a convert and a reciprocal);
    // it is recomputed exactly at every phase and after any rare path
    const u32 q16 = hint_floor(X, d.G) & (m.lut_max << 4);
    const u32x4 ent = *(const __attribute__((address_space(3))) u32x4*)(uintptr_t)q16;
    s = ent.z;
    t = make_uint2(ent.x, ent.y);
    tc = __uint_as_float(ent.w);
  } else if (LUT == 5) {  // the flat model (c = 1, cum[s] = s, total 256): the hint is the symbol
    // (no table read; a hint past 255, corrupt input only, starts the exact fix-up elsewhere)
    s = hint_floor(X, d.G) & 255u;
    t = make_uint2(s, 1u);
    tc = 256.0f;
  } else if (LUT == 3) {  // pair buckets: both candidates of the bucket in ONE 16-B read
    // qh = q (buckets of 16: the entry's byte offset is q & 0xFFF0, no shift); the candidate
    // by q < cum1 (no split: both candidates are s0); the symbol pair is a u16 read off the same
    // offset.  The compare goes to VCC with SDWA word selects, and each field is one
    // v_cndmask_b32 (VCC ? src1 : src0) whose SDWA source selects unpack the entries' u16 halves
    // and the pair's bytes on the way (one asm block: VCC cannot be an asm operand).
    const u32 qh = hint_floor(X, d.G);
    const u32 ea = qh & ((PAIR_BUCKETS - 1) << 4);
    const u32x4 e = *(const __attribute__((address_space(3))) u32x4*)(uintptr_t)(ea + PAIR_ENT_OFF);
    const u32 sp = *(const __attribute__((address_space(3))) unsigned short*)(uintptr_t)(ea >> 3);
    u32 cum, c, tcb;
    asm("v_cmp_lt_u32_sdwa vcc, %4, %5 src0_sel:WORD_0 src1_sel:WORD_0\n\t" RC_VCC_WAIT
        "v_cndmask_b32_sdwa %0, %5, %6, vcc dst_sel:DWORD dst_unused:UNUSED_PAD "
        "src0_sel:WORD_0 src1_sel:WORD_0\n\t"
        "v_cndmask_b32_sdwa %1, %5, %6, vcc dst_sel:DWORD dst_unused:UNUSED_PAD "
        "src0_sel:WORD_1 src1_sel:WORD_1\n\t"
        "v_cndmask_b32_e32 %2, %7, %8, vcc\n\t"
        "v_cndmask_b32_sdwa %3, %9, %9, vcc dst_sel:DWORD dst_unused:UNUSED_PAD "
        "src0_sel:BYTE_1 src1_sel:BYTE_0"
        : "=&v"(cum), "=&v"(c), "=&v"(tcb), "=&v"(s)
        : "v"(qh), "v"(e.y), "v"(e.x), "v"(e.w), "v"(e.z), "v"(sp)
        : "vcc");
    tc = __uint_as_float(tcb);
    t = make_uint2(cum, c);
  } else if (LUT == 4) {
    // small bucket models: the 8-B bucket at (q >> la_shift) & la_mask (past the symbol table,
    // an immediate offset) holds the candidates' byte addresses 16 s as u16 halves and
    // hint_floor's bits of cum[s1] (0x4B400000 + cum[s1]); the candidate's 16-B entry
    // {cum, c, total/c, s} is then one ds_read_b128 at that address
    const u32 qh = hint_floor(X, d.G);
    // the bucket's byte address from a second fma whose ulp is 2^la_shift (round-toward-zero:
    // its low bits are floor(q / 2^la_shift)), beside the hint's rather than after it: the
    // table read waits for one op less
    const u32 la = __float_as_uint(__builtin_fmaf(X, d.G, m.la_magic)) & m.la_mask;
    typedef u32 u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 e = *(const __attribute__((address_space(3))) u32x2*)(uintptr_t)(la + SMB_LUT_OFF);
    // before s1 starts (q < cum[s1], compared as hint_floor bits): s0, the low half, else s1.
    // One compare into VCC and one v_cndmask_b32 whose SDWA source selects take the halves
    // (VCC ? src1 : src0); from C the compiler unpacks both halves first.
    u32 ta;
    if (SELFILL) {  // the two wait states: range >> lg and the ring address (2 VALU, no s_nop)
      asm("v_cmp_lt_u32_e32 vcc, %3, %4\n\t"
          "v_lshrrev_b64 %1, %6, %7\n\t"
          "v_lshl_add_u32 %2, %8, 3, %9\n\t"
          "v_cndmask_b32_sdwa %0, %5, %5, vcc dst_sel:DWORD dst_unused:UNUSED_PAD "
          "src0_sel:WORD_1 src1_sel:WORD_0"
          : "=v"(ta), "=&v"(r), "=&v"(raddr)
          : "v"(qh), "v"(e.y), "v"(e.x), "s"(m.lg), "v"(d.range), "v"(roff),
            "v"((u32)(uintptr_t)d.ring)
          : "vcc");
    } else {
      asm("v_cmp_lt_u32_e32 vcc, %1, %2\n\t" RC_VCC_WAIT
          "v_cndmask_b32_sdwa %0, %3, %3, vcc dst_sel:DWORD dst_unused:UNUSED_PAD "
          "src0_sel:WORD_1 src1_sel:WORD_0"
          : "=v"(ta)
          : "v"(qh), "v"(e.y), "v"(e.x)
          : "vcc");
    }
    const u32x4 te = *(const __attribute__((address_space(3))) u32x4*)(uintptr_t)ta;
    if (SELFILL) {
      const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
      D0 = rp[0];
      D1 = rp[D::kS];
    }
    t = make_uint2(te.x, te.y);
    tc = __uint_as_float(te.z);
    s = te.w;
  } else if (LUT == 6) {
    // small bucket models, one byte per q: the symbol at the masked hint (the table is the
    // kernel's first LDS object, so q is its byte address), then the symbol's 16-B entry
    // {cum, c, total/c, 0} right after the table, at byte symof_mask + 1 + 16 s (one
    // v_lshl_add_u32: the base is wave-uniform).  No entry of this table straddles a symbol
    // boundary, so there is no candidate to choose: no compare, no select, no VCC.
    const u32 q = hint_floor(X, d.G) & m.symof_mask;
    s = *(const __attribute__((address_space(3))) uint8_t*)(uintptr_t)q;
    // (written out: from C the compiler splits it into a shift and an add of the mask, with
    // the + 1 as the read's offset)
    u32 ta;
    asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(ta) : "v"(s), "s"(m.symof_mask + 1u));
    const u32x4 te = *(const __attribute__((address_space(3))) u32x4*)(uintptr_t)ta;
    t = make_uint2(te.x, te.y);
    tc = __uint_as_float(te.z);
  } else if (LUT) {  // direct table: candidate symbol and its (cum, c) in one LDS read at byte 4q
    // the LUT is the kernel's first LDS object (address 0): q4 is its LDS byte address
    const u32 q4 = hint_floor(X, (4.0f * m.ftotal) * rR) & (m.lut_max << 2);
    const u32 ent = *(const __attribute__((address_space(3))) u32*)(uintptr_t)q4;
    s = ent;  // the symbol is its low byte (callers take byte 0; dec_fix masks it)
    t = make_uint2((ent >> 8) & 0xFFFu, ent >> 20);
  } else {  // bucket table, then the (cum, c) table
    // bucket = lut_bits bits of qh from lut_shift (bucket tables always hold 2^lut_bits
    // entries: total > 2048 makes (total - 1) >> lut_shift >= 2^(lut_bits - 1), padded to a
    // power of two; 11 bits for small models, 12 for wide ones), the
    // candidate by the offset inside the bucket against the entry's split, as a sign mask and a
    // bit-field extract (a compare and a select would read VCC), extracted already masked
    const u32 qh = SM ? hint_floor(X, GC::on ? d.G : m.ftotal * rR)
                       : cvt_u32_sat(X * (GC::on ? d.G : m.ftotal * rR));
    // (the width is a compile-time constant: a second SGPR operand would cost a v_mov; the LUT
    // is at LDS address 0, so its byte address is the index times 4: one v_lshlrev_b32, not the
    // compiler's v_lshl_add_u32 with a zero base)
    u32 la;
    asm("v_lshlrev_b32 %0, 2, %1"
        : "=v"(la) : "v"(__builtin_amdgcn_ubfe(qh, m.lut_shift, SM ? SM_LUT_BITS : LUT_BITS)));
    const u32 ent = *(const __attribute__((address_space(3))) u32*)(uintptr_t)la;
    // ~0: s0.  Small models store s1's absolute cum (< 2^16) in the entry, wide ones its
    // offset inside the bucket
    const u32 below = SM ? smask((qh & 0xFFFFu) - (ent >> 16))
                         : smask((qh & ((1u << m.lut_shift) - 1u)) - (ent >> 16));
    s = __builtin_amdgcn_ubfe(ent, mselc(below, 0u, 8u), 8);
    if (GC::on) {  // 16-B entries {cum, c, total / c, 0}: one ds_read_b128
      const uint4 e4 = *(const uint4*)(s_tab + 4 * s);
      t = make_uint2(e4.x, e4.y);
      tc = __uint_as_float(e4.z);
    } else {
      t = *(const uint2*)(s_tab + 2 * s);
    }
  }
  u64 B = LUT == 5 ? r : mul_rv<SM>(r, t.y);  // (flat: c = 1)
  if (LUT == 3 || (DEC_SPEC && SM)) {
    // Pair buckets run the latency-bound shapes, so this step is arranged for its dependency
    // chain: param_update goes ahead on the hint's candidate and the verification joins the
    // rare test at the end (no branch before the renormalisation), and low + A comes from one
    // multiply-add (v_mad_u64_u32 takes low as its addend).  A lane whose hint was off redoes
    // the symbol from the state saved before it.
    const D d0 = d;
    const u64 L = mad_rv<SM>(r, t.x, d.low);
    // x - r cum < r c (mod 2^64) as L <= data < L + B: two compares against the new bounds,
    // whose upper one the renormalisation forms anyway.  (Were L + B to reach 2^64 the wrapped
    // bound would fail every lane: a fix-up, never a wrong symbol.)
    // (as lane masks: from a bool the compiler goes through a v_cndmask_b32 and back)
    const u64 U = L + B;
    // the failing lanes directly: a compare leaves inactive lanes 0, so no exec & ~ok
#ifndef RC_DEC_OKM  // (scratch A/B builds: the round-4 form, ok-mask then exec & ~ok)
    const u64 badm = __builtin_amdgcn_ballot_w64(d.dat < L) | __builtin_amdgcn_ballot_w64(d.dat >= U);
#else
    const u64 okm = __builtin_amdgcn_ballot_w64(d.dat >= L) & __builtin_amdgcn_ballot_w64(d.dat < U);
    const u64 badm = __builtin_amdgcn_ballot_w64(true) & ~okm;
#endif
    dec_apply<SM, LUT>(d, L, B, d0.dat, tc, D0, D1, D2);
    // the lanes with range < 2^48, as a 32-bit compare of the high half written out (the
    // compiler folds it into a 64-bit compare of the shifted pair), joined with the failed
    // verifications into one wave-uniform branch
    u64 rm;
    asm("v_cmp_gt_u32_e64 %0, %1, %2" : "=s"(rm) : "s"(0x10000u), "v"(hi32(d.range)));
    if (__builtin_expect((badm | rm) != 0, 0)) {
      if (!((d0.dat >= L) & (d0.dat < U))) {
        d = d0;
        u64 A = mul_rv<SM>(r, t.x);
        dec_fix<GC::tab_stride>(s, t, A, B, d.x(), r, s_tab, m.n);
        tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));
        if (t.y == 0) {  // corrupt input (see below)
          d.err = d.err ? d.err : (d.bpos > d.limb ? RC_F_TRUNCATED : RC_F_CORRUPT);
          B = r;
        }
        dec_apply<SM, LUT>(d, d.low + A, B, d.dat, tc, D0, D1, D2);
      }
      if (hi32(d.range) < 0x10000u) {
        dec_rare(d, DEC_NEED_SM);
        dec_gexact<SM, LUT>(d, m);
      }
    }
    return s;
  }
  // exact verification r*cum[s] <= x < r*cum[s+1] as ONE unsigned test: A + B <= range < 2^64,
  // so when A > x the wrapped difference x - A is >= 2^64 - A > B.  The hint is rarely off.
  // (At s = n - 1 the test fails only on corrupt input, x >= r * total: dec_fix keeps s = n-1.)
  u64 A = mul_rv<SM>(r, t.x);
  u64 dx = sub64((u32)d.dat, d.dhi(), d.low + A);  // x - r cum
  if (__builtin_expect(__any((int)(dx >= B)), 0)) {
    if (dx >= B) {
      dec_fix<GC::tab_stride>(s, t, A, B, d.x(), r, s_tab, m.n);
      if (GC::on) tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));
      // the tables only hold symbols with c > 0, so c == 0 can only come from dec_fix: corrupt
      // input (the reference loops forever); an over-read, if any, came first
      if (t.y == 0) {
        d.err = d.err ? d.err : (d.bpos > d.limb ? RC_F_TRUNCATED : RC_F_CORRUPT);
        B = r;
      }
    }
  }
  dec_apply<SM, LUT>(d, d.low + A, B, d.dat, tc, D0, D1, D2);
  // rare: range_reduction_expansion, or (wide models) the ring runs short for the next symbol
  const bool rare = SM ? (hi32(d.range) < 0x10000u)
                       : ((hi32(d.range) < 0x10000u) | ((int)(d.fillb - d.bpos) < (int)(8 * DEC_NEED_WIDE)));
  if (__builtin_expect(__any((int)rare), 0)) {
    if (rare) {
      dec_rare(d, SM ? DEC_NEED_SM : DEC_NEED_WIDE);
      dec_gexact<SM, LUT>(d, m);
    }
  }
  return s;
}

// SM models: the ring check for the symbols up to the next check, NEED bytes (at most 3 per
// symbol; wave-uniform call sites)
template <int SM, u32 NEED = DEC_NEED_HEAD, class D>
static __device__ __forceinline__ void dec_check4(D& d) {
  if (!SM) return;
  constexpr u32 need = NEED;
  const bool low = (int)(d.fillb - d.bpos) < (int)(8 * need);
  if (__builtin_expect(__any((int)low), 0)) {
    if (low) dec_sync(d, need);
  }
}

// 16 symbols into one 16-B block (byte j of word q = symbol 4q + j), with the ring checks
template <int DIV, int SM, int LUT, class D>
static __device__ __forceinline__ uint4 dec_phase16(D& d, const ModelArgs& m,
                                                    const u32* s_tab, const u32* s_lut) {
  dec_gexact<SM, LUT>(d, m);  // bounds the drift of the carried scale to 16 symbols
  u32 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[q] = put_byte(w[q], dec_sym<DIV, SM, LUT>(d, m, s_tab, s_lut), j);
    // (DEC_CHECK_SPAN symbols between ring checks inside the phase: 4, or 8 with a 24-B need)
    if (q < 3 && ((q + 1) * 4) % DEC_CHECK_SPAN == 0) dec_check4<SM, DEC_NEED_SPAN>(d);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

#ifndef RC_DEC_SHARED_ONLY
#ifdef RC_DEC_WAVES  // scratch builds: the occupancy the compiler must fit (DESIGN.md §6)
#define RC_DEC_ATTR __attribute__((amdgpu_waves_per_eu(RC_DEC_WAVES, RC_DEC_WAVES)))
#else
#define RC_DEC_ATTR
#endif
// k_decode_static, and with RC_DEC_GROUPED its grouped twin k_decode_static_grouped (static chunk
// sets, rc_chunk_set.h): the lane's chunk comes from g.order, and the workgroup stages the tables
// of its class, row g.wg_row[blockIdx.x] of the set.  The preprocessor makes the difference, so
// that k_decode_static compiles from the tokens it had before there were chunk sets.
#ifdef RC_DEC_GROUPED
#define RC_DEC_KERNEL k_decode_static_grouped
#define RC_DEC_GRP_PARAM GroupArgs g,
#else
#define RC_DEC_KERNEL k_decode_static
#define RC_DEC_GRP_PARAM
#endif
template <int DIV, int SM, int LUT, int WGS = WG, int LD = DEC_LD>
__global__ __launch_bounds__(WGS) RC_DEC_ATTR void RC_DEC_KERNEL(
    ModelArgs m, RC_DEC_GRP_PARAM const uint8_t* __restrict__ code, const u64* __restrict__ code_off,
    const u64* __restrict__ code_len, uint8_t* __restrict__ syms_out,
    const u64* __restrict__ sym_off, u32 n_chunks, u32* __restrict__ flags) {
  // small models always carry LUT 4's 8-B buckets (rc_model_create_static); the LUT 0 bucket
  // path reads the old 4-B format and is reached only by large models
  static_assert(!(SM && LUT == 0), "small models decode through LUT 3 or LUT 4");
  RC_STAMP_BEGIN();
  rc_set_prio(m);
#ifdef RC_DEC_GROUPED
  {  // a workgroup with no class leaves before staging
    const u32 row = g.wg_row[blockIdx.x];
    if (row == ~0u) return;
    m.tab += (size_t)row * 256;
    m.lut += (size_t)row * g.lut_stride;
    if (LUT == 6) m.symof += (size_t)row * g.symof_stride;
  }
#endif
  // All LDS is dynamic, sized at launch (the WG's footprint sets how many WGs share a CU):
  // the LUT (lut_max + 1 entries) first, at LDS address 0, so a table read is a ds_read at the
  // hint's byte offset with no base add; then the (cum, c) table and the code rings.
  // (LUT 4: the 16-B symbol table comes first, at address 0, and the buckets after it)
  extern __shared__ u32 s_dyn[];
  u32* s_lut = LUT == 4 ? s_dyn + SMB_TAB_WORDS : s_dyn;
  // LUT words (pair buckets: the symbol pairs, then the 16-B entries; LUT 4: 8-B buckets)
  // (LUT 6: the q-to-symbol bytes, a power of two >= 4096 of them)
  const u32 lut_n = LUT == 5 ? 0u
                    : LUT == 6 ? (m.symof_mask + 1) / 4u
                    : LUT == 3 ? PAIR_WORDS : (m.lut_max + 1) * (LUT == 2 ? 4u : LUT == 4 ? 2u : 1u);
  const u32 lut_words = (lut_n + 3) & ~3u;                    // 16-B aligned s_tab
  // (direct tables hold (cum, c) themselves, and pair buckets both candidates: then only the
  // rare exact fix-up reads the table, from global memory)
  constexpr bool tab_lds = !LUT || LUT == 4 || LUT == 6 || (DEC_TAB_LDS && LUT != 3);
  typedef GCarry<SM, LUT> GC;
  const u32* s_tab = LUT == 4 ? s_dyn : tab_lds ? s_dyn + lut_words : (const u32*)m.tab;
  const u32* lut_src = LUT == 3 ? m.pair : LUT == 6 ? (const u32*)m.symof : m.lut;
  const u32 tid = threadIdx.x;
  if (tab_lds && tid < 256) {
    const uint2 e = m.tab[tid];
    if (LUT == 4) {  // {cum, c, total / c (hint only: any rounding), the symbol}
      u32* te = s_dyn + 4 * tid;
      te[0] = e.x;
      te[1] = e.y;
      te[2] = __float_as_uint(m.ftotal / (float)e.y);
      te[3] = tid;
    } else {
      u32* te = s_dyn + lut_words + GC::tab_stride * tid;
      te[0] = e.x;
      te[1] = e.y;
      if (GC::tab_stride == 4) {  // total / c for the carried hint scale (hint only)
        te[2] = __float_as_uint(m.ftotal / (float)e.y);
        te[3] = 0u;
      }
    }
  }
  for (u32 j = tid; j < lut_n; j += WGS) s_lut[j] = lut_src[j];
  __syncthreads();
#ifdef RC_DEC_GROUPED
  const u32 k = g.order[blockIdx.x * WGS + tid];
  if (k == ~0u) return;  // a dead lane
#else
  const u32 k = blockIdx.x * WGS + tid;
  if (k >= n_chunks) return;
#endif
  // f32 rounding toward zero from here on (MODE.FP_ROUND f32 bits = 3), for hint_floor.  The
  // other float operations only form hints and the carried hint scale, which the exact
  // verification backs, so their rounding direction does not matter.
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3");
#ifndef RC_DEC_WAVES
  RC_VGPR_FLOOR_96();
#endif
  const u32 lane = tid & 63, wave = tid >> 6;

  const u64 c0 = code_off[k];
  const u64 clen = code_len[k];
  const u64 n = sym_off[k + 1] - sym_off[k];
  uint8_t* op = syms_out + sym_off[k];
  if (n > RC_MAX_CHUNK_SYMBOLS) {  // 32-bit stream positions (include/range_coder.h)
    flags[k] = RC_F_TOO_LONG;
    return;
  }
  if (clen < 8) {  // Decoder::new panics (decoder.rs:21, :33)
    flags[k] = RC_F_TRUNCATED;
    return;
  }
  const uint8_t* cp = code + c0;
  // load bursts start on 16 * DEC_LD-byte boundaries of the address space: a burst never
  // straddles two 128-B lines, so each line is fetched by 128 / (16 * DEC_LD) bursts, not more
  constexpr u32 GAL = 16 * LD;
  const u32 a = (u32)((uintptr_t)cp & (GAL - 1));

  constexpr int ROWS = DEC_ROWS && LUT == 2;
  Dec<LD, ROWS> d;
#ifdef RC_FILL
  d.fill = 0;
#endif
  d.low = 0;
  d.range = ~0ull;
  d.err = 0;
  d.fillb = 0;
  d.pend_ok = 0;
  // the ring as a plain LDS address (s_dyn is at 0), one register: no per-access base math
  u32 ring0 = (LUT == 4 ? SMB_TAB_WORDS + lut_words
                         : lut_words + (tab_lds ? 256 * GC::tab_stride : 0)) * 4;
  if (ROWS) {  // 1-KiB aligned (rc_static_decode_lds sizes the same)
    ring0 = (ring0 + 1023u) & ~1023u;
    d.ring = (l_u32*)(uintptr_t)ring0 + wave * (DEC_ROW_WAVE_BYTES / 4) + (lane >> 3) * 256 +
             (lane & 7);
  } else {
    d.ring = (l_u32*)(uintptr_t)ring0 + wave * DEC_RING_ALLOC * 64 + lane;
  }
  d.gbase = reinterpret_cast<const uint4*>(cp - a);
  d.gnext = 0;
  // n <= 2^25 symbols consume at most 8 + 12 n < 2^29 bytes: code past 2^29 is never read
  const u32 lim = (u32)(clen < (1ull << 29) - a ? a + clen : 1ull << 29);
  d.glast = ((lim - 1) >> 4) & ~(u32)(LD - 1);  // (the last segment's first block)
  d.bpos = 8 * (a + 8);  // Decoder::new primes 8 bytes (decoder.rs:21)
  d.limb = 8 * lim;
  // fill the whole ring, and have the next load burst in flight
#pragma unroll
  for (int h = 0; h < DEC_RING / (4 * DEC_PF); ++h) {
    if (!d.pend_ok) dec_issue(d);
    dec_commit(d);
  }
  // a stream starting late in its first burst: stage the primed bytes and the first symbol's
  // (the wide models' ring check comes after a symbol); < 32 B more than that are staged, so
  // the ring still holds the primed bytes
  while ((int)(d.fillb - d.bpos) < (int)(8 * DEC_NEED_HEAD)) {
    if (!d.pend_ok) dec_issue(d);
    dec_commit(d);
  }
  if (!d.pend_ok) dec_issue(d);
  d.set_data(dec_read8_before(d));  // Decoder::new's data (low = 0)
  dec_gexact<SM, LUT>(d, m);

  u64 i = 0;
  // head: single symbols until the output is 64-B aligned
  constexpr u32 OUT_ALIGN = 16 * DEC_OUT_BURST;  // (symbols before the first aligned burst)
  u64 head = (OUT_ALIGN - ((uintptr_t)op & (OUT_ALIGN - 1))) & (OUT_ALIGN - 1);
  if (head > n) head = n;
  dec_check4<SM>(d);
  for (; i < head; ++i) {
    op[i] = (uint8_t)dec_sym<DIV, SM, LUT>(d, m, s_tab, s_lut);
    dec_check4<SM>(d);
  }
  dec_check4<SM, DEC_NEED_SPAN>(d);
  // body: 16-symbol phases (after each: commit a refill, maybe issue the next load burst).
  // Decoded symbols leave in 64-B bursts per lane (4 phases, four back-to-back 16-B stores to
  // one 64-B segment): HBM sees whole 64-B writes, not 16-B partial ones.
  uint4* ob = reinterpret_cast<uint4*>(op + i);
  const u64 nbu = DEC_OUT_BURST > 1 ? (n - i) / (16 * DEC_OUT_BURST) : 0;
  for (u64 b = 0; b < nbu; ++b) {
    rc_prio_rotate(m.prio_rot);
    // written out: the compiler declines to unroll a 64-symbol loop and would then index the
    // blocks through scratch
#define RC_DEC_PHASE(o)                                          \
  const uint4 o = dec_phase16<DIV, SM, LUT>(d, m, s_tab, s_lut); \
  dec_phase(d);                                                  \
  dec_check4<SM, DEC_NEED_SPAN>(d);
    RC_DEC_PHASE(o0) RC_DEC_PHASE(o1) RC_DEC_PHASE(o2) RC_DEC_PHASE(o3)
    uint4* ob_b = ob + DEC_OUT_BURST * b;
    if (DEC_OUT_BURST == 8) {
      RC_DEC_PHASE(o4) RC_DEC_PHASE(o5) RC_DEC_PHASE(o6) RC_DEC_PHASE(o7)
      ob_b[0] = o0; ob_b[1] = o1; ob_b[2] = o2; ob_b[3] = o3;
      ob_b[4] = o4; ob_b[5] = o5; ob_b[6] = o6; ob_b[7] = o7;
    } else {
      ob_b[0] = o0; ob_b[1] = o1; ob_b[2] = o2; ob_b[3] = o3;
    }
#undef RC_DEC_PHASE
  }
  i += nbu * 16 * DEC_OUT_BURST;
  ob += DEC_OUT_BURST * nbu;
  const u64 nph = (n - i) >> 4;
  for (u64 b = 0; b < nph; ++b) {
    ob[b] = dec_phase16<DIV, SM, LUT>(d, m, s_tab, s_lut);
    dec_phase(d);
    dec_check4<SM, DEC_NEED_SPAN>(d);
  }
  i += nph << 4;
  for (; i < n; ++i) {
    op[i] = (uint8_t)dec_sym<DIV, SM, LUT>(d, m, s_tab, s_lut);
    dec_check4<SM>(d);
  }
  // shift_left_buffer panics once more bytes are needed than the stream holds (decoder.rs:33)
  if (!d.err && d.bpos > d.limb) d.err = RC_F_TRUNCATED;
  RC_STAMP_END(RC_DEC_TU, blockIdx.x * (WGS / 64) + wave, lane, n);
  flags[k] = d.err;
}


// RC_DEC_DIV selects the variants this translation unit instantiates (rc_decode_pow2.hip,
// rc_decode_magic.hip)
namespace {
// Pair-bucket variant and its workgroup size for a launch: 0 (the default: the small
// bucket-model decoder, LUT 4, with 2^12 buckets in 512-lane workgroups is as fast or faster at
// every shape measured, 2^17 to 2^20 chunks, DESIGN.md §5), or 512 / 1024 when the context was
// created with RC_DEC_PAIR set (tests and measurements).
u32 pair_wgs(const RcKnobs& k, const ModelArgs& a, int sm) {
  if (!a.pair || !sm || a.direct) return 0;
  return k.dec_pair == 512 || k.dec_pair == 1024 ? k.dec_pair : 0;
}

// Whether a launch of a small bucket model decodes through the direct q-to-symbol table (LUT 6,
// SYMOF_WG lanes, one workgroup per CU) instead of the buckets (LUT 4).  RC_DEC_PAIR=6 / =4 force
// one or the other for every model that carries the table (tests and measurements).  Otherwise
// the models with 2^12 buckets (LUT 4's 512-lane class) take it once the grid gives every
// workgroup slot of the device SYMOF_MIN_ROUNDS workgroups; `resident` is what the device holds
// of them at once (its CU count, from the runtime).  A smaller launch, the 2^17-chunk shard
// among them, would leave CUs idle at 1,024 lanes and keeps LUT 4 (DESIGN.md §5.2).
#ifndef SYMOF_MIN_ROUNDS
#define SYMOF_MIN_ROUNDS 1u
#endif
bool symof_launch(const RcKnobs& k, const ModelArgs& a, u32 n_chunks, u32 resident) {
  if (k.dec_pair == 6) return true;
  if (!resident) return false;
  return (n_chunks + SYMOF_WG - 1) / SYMOF_WG >= SYMOF_MIN_ROUNDS * resident;
}
// (the launches that can take it at all: the model carries the table, and the switch does not
// force the buckets; unforced, only LUT 4's 512-lane class)
bool symof_candidate(const RcKnobs& k, const ModelArgs& a, int sm) {
  if (!a.symof || !sm || a.direct || k.dec_pair == 4) return false;
  return k.dec_pair == 6 || SMB_WG(a.lut_max + 1) == 512;
}
}  // namespace

#ifdef RC_DEC_GROUPED
// The variant a chunk set's rows decode through when the direct q-to-symbol table is not taken
// (no row is flat, none carries pair tables: DESIGN.md §9.20), and its lanes per workgroup
static u32 rc_chunk_decode_class_(const ModelArgs& a, int* lut) {
  *lut = a.direct == 2 ? 2 : a.direct ? 1 : 4;
  return !a.direct && SMB_WG(a.lut_max + 1) == 512 ? 512u : (u32)WG;
}

#if RC_DEC_DIV == 0
u32 rc_chunk_decode_class(const ModelArgs& a, int* lut) { return rc_chunk_decode_class_(a, lut); }
hipError_t rc_chunk_decode_launch_pow2(
#else
hipError_t rc_chunk_decode_launch_magic(
#endif
    hipStream_t stream, const RcKnobs& k, const ModelArgs& a_in, const ChunkSetArgs& cs,
    GroupScratch& sc, const uint8_t* class_of, const uint8_t* code, const u64* code_off,
    const u64* code_len, uint8_t* syms_out, const u64* sym_off, u32 n_chunks, u32* flags) {
  ModelArgs a = a_in;
  // k_decode_static's launch (below) at the padded workgroup count, after the grouping for the
  // variant's workgroup size
  auto go = [&](auto kern, u32 wgs, size_t lds, PrioPolicy dflt, u32 lut_of) {
    GroupArgs g{nullptr, nullptr, cs.lut_stride, cs.symof_stride};
    const hipError_t e =
        rc_chunk_group_launch(stream, sc, class_of, n_chunks, cs.k, wgs, flags, nullptr, &g);
    if (e != hipSuccess) return e;
    const dim3 grid(rc_group_grid(n_chunks, cs.k, wgs)), block(wgs);
    rc_prio_policy(a, dflt, grid.x,
                   rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)wgs, lds), k);
    hipLaunchKernelGGL(kern, grid, block, lds, stream, a, g, code, code_off, code_len, syms_out,
                       sym_off, n_chunks, flags);
    const hipError_t le = hipGetLastError();
    const hipError_t de = rc_chunk_group_done(stream, sc, wgs, lut_of, grid.x);
    return le != hipSuccess ? le : de;
  };
  // (RC_DEC_PAIR=512 / 1024 finds no pair table here and falls through to LUT 4)
  if (symof_candidate(k, a, 1)) {
    const auto kern = k_decode_static_grouped<RC_DEC_DIV, 1, 6, SYMOF_WG>;
    const size_t lds = rc_static_decode_lds(a, 6, SYMOF_WG);
    const hipError_t e = set_allow_lds(reinterpret_cast<const void*>(kern));
    if (e != hipSuccess) return e;
    if (symof_launch(k, a, rc_group_grid(n_chunks, cs.k, SYMOF_WG) * SYMOF_WG,
                     rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)SYMOF_WG, lds)))
      return go(kern, SYMOF_WG, lds, kPrioDecoder1024, 6);
  }
  int lut = 0;
  const u32 wgs = rc_chunk_decode_class_(a, &lut);
  const size_t lds = rc_static_decode_lds(a, 0, wgs);
  if (wgs == 512)
    return go(k_decode_static_grouped<RC_DEC_DIV, 1, 4, 512>, 512, lds, kPrioDecoder512, 4);
  if (lut == 2) return go(k_decode_static_grouped<RC_DEC_DIV, 1, 2>, WG, lds, kPrioDecoder, 2);
  if (lut == 1) return go(k_decode_static_grouped<RC_DEC_DIV, 1, 1>, WG, lds, kPrioDecoder, 1);
  return go(k_decode_static_grouped<RC_DEC_DIV, 1, 4>, WG, lds, kPrioDecoder, 4);
}
#else  // RC_DEC_GROUPED

#if RC_DEC_DIV == 0
hipError_t rc_static_decode_launch_pow2(
#else
hipError_t rc_static_decode_launch_magic(
#endif
    hipStream_t stream, const RcKnobs& k, const ModelArgs& a_in, int sm, const uint8_t* code,
    const u64* code_off,
    const u64* code_len, uint8_t* syms_out, const u64* sym_off, u32 n_chunks, u32* flags) {
  ModelArgs a = a_in;
  // one launch of kernel `kern` in workgroups of `wgs` lanes, with the launch's wave priorities
  // (rc_static.h, DESIGN.md §5)
  auto go = [&](auto kern, u32 wgs, size_t lds, PrioPolicy dflt) {
    const dim3 grid((n_chunks + wgs - 1) / wgs), block(wgs);
    rc_prio_policy(a, dflt, grid.x,
                   rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)wgs, lds), k);
    hipLaunchKernelGGL(kern, grid, block, lds, stream, a, code, code_off, code_len, syms_out,
                       sym_off, n_chunks, flags);
    return hipGetLastError();
  };
  const u32 pw = pair_wgs(k, a, sm);
  if (pw) {
    const size_t lds = rc_static_decode_lds(a, 3, pw);
    if (pw == 1024) return go(k_decode_static<RC_DEC_DIV, 1, 3, 1024>, 1024, lds, kPrioDecoder512);
    return go(k_decode_static<RC_DEC_DIV, 1, 3, 512, DEC_PAIR512_LD>, 512, lds, kPrioDecoder512);
  }
  if (symof_candidate(k, a, sm)) {
    const auto kern = k_decode_static<RC_DEC_DIV, 1, 6, SYMOF_WG>;
    const size_t lds = rc_static_decode_lds(a, 6, SYMOF_WG);
    // (more than 64 KiB of dynamic LDS: allowed once per device, before the occupancy query)
    const hipError_t e = set_allow_lds(reinterpret_cast<const void*>(kern));
    if (e != hipSuccess) return e;
    if (symof_launch(k, a, n_chunks,
                     rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)SYMOF_WG, lds)))
      return go(kern, SYMOF_WG, lds, kPrioDecoder1024);
  }
#ifdef RC_SMB_WG  // scratch builds: every small bucket model in workgroups of RC_SMB_WG lanes
  if (sm && !a.direct)
    return go(k_decode_static<RC_DEC_DIV, 1, 4, RC_SMB_WG>, RC_SMB_WG,
              rc_static_decode_lds(a, 0, RC_SMB_WG), kPrioDecoder512);
#endif
  if (sm && !a.direct && SMB_WG(a.lut_max + 1) == 512)  // 2^12 buckets (rc_static.h)
    return go(k_decode_static<RC_DEC_DIV, 1, 4, 512>, 512, rc_static_decode_lds(a, 0, 512),
              kPrioDecoder512);
  const size_t lds = rc_static_decode_lds(a, 0, WG);
#define RC_DEC_LAUNCH(S, L) return go(k_decode_static<RC_DEC_DIV, S, L>, WG, lds, kPrioDecoder)
  const bool dl = a.direct != 0, dl2 = a.direct == 2;
  // (direct == 2 implies sm)
  if constexpr (RC_DEC_DIV == DIV_POW2) {  // the flat model (total 256: a power of two)
    if (a.flat) RC_DEC_LAUNCH(1, 5);
  }
#ifdef RC_DEV_ONLY
  if (RC_DEC_DIV != DIV_POW2 || !sm) return hipErrorInvalidValue;
  if (dl2) RC_DEC_LAUNCH(1, 2);
  else if (dl) RC_DEC_LAUNCH(1, 1); else RC_DEC_LAUNCH(1, 4);
#else
  if (dl2) RC_DEC_LAUNCH(1, 2);
  else if (sm) { if (dl) RC_DEC_LAUNCH(1, 1); else RC_DEC_LAUNCH(1, 4); }
  else    { if (dl) RC_DEC_LAUNCH(0, 1); else RC_DEC_LAUNCH(0, 0); }
#endif
#undef RC_DEC_LAUNCH
}

#if RC_DEC_DIV == 0
size_t rc_static_decode_lds(const ModelArgs& a, int lut, u32 wgs) {
  // LUT (8-B aligned), the (cum, c) table (16-B entries for small bucket models, which carry
  // total / c too; none for pair buckets), the code rings
  const size_t rings = (wgs / 64) * DEC_RING_ALLOC * 64 * sizeof(u32);
  if (lut == 3) return PAIR_WORDS * sizeof(u32) + rings;
  // the q-to-symbol bytes, the 16-B entries, the rings (at most 143,360 B: rc_static.h)
  if (lut == 6) return (size_t)a.symof_mask + 1 + 256 * 16 + rings;
  const bool dl = a.direct != 0, dl2 = a.direct == 2;
  const bool sm = rc_static_sm(a.total);
  const bool smb = sm && !dl;  // LUT 4: 8-B buckets and the 16-B symbol table
  const bool rows = DEC_ROWS && dl2 && !a.flat;  // (direct == 2 implies sm)
  const size_t lut_n = a.flat ? 0 : ((size_t)a.lut_max + 1) * (dl2 ? 4 : smb ? 2 : 1);  // (smb: 16-B table)
  const size_t tab = !dl ? (sm ? 16 : 8) : (DEC_TAB_LDS ? 8 : 0);
  // -DRC_DEC_LDS_PAD=bytes (scratch builds, measurements): extra LDS per workgroup, to set the
  // occupancy by LDS with the same code
#ifdef RC_DEC_LDS_PAD
  const size_t extra = (size_t)(RC_DEC_LDS_PAD);
#else
  const size_t extra = 0;
#endif
  const size_t head = ((lut_n + 3) & ~(size_t)3) * sizeof(u32) + 256 * tab;
  if (rows) return ((head + 1023) & ~(size_t)1023) + (wgs / 64) * DEC_ROW_WAVE_BYTES + extra;
  return head + rings + extra;
}
#endif
#endif  // RC_DEC_GROUPED
#endif  // RC_DEC_SHARED_ONLY
