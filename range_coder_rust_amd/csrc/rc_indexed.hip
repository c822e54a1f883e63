// rc_indexed.hip — k_encode_indexed / k_decode_indexed: the small-model static coders with a
// table that changes per symbol (static model sets, rc_indexed.h).  Symbol i of a chunk is coded
// exactly as encoder.encode(&models[idx[i]], sym[i]) / decoder.decode(&models[idx[i]]).  The
// arithmetic, the encoder's accumulator, ring and ranked flush rounds and the decoder's code
// ring, dec_apply and dec_rare are those of the single-table coders (rc_encode.inc,
// rc_decode.inc, rc_static.h); what is new is the per-symbol table base, the index stream beside
// the symbols and one large workgroup per CU that stages the K tables once.
#define RC_DEC_SHARED_ONLY
#include "rc_indexed.h"

#include <mutex>
#include <set>
#include <utility>

#include "rc_encode.inc"
#include "rc_decode.inc"
#include "rc_cuwg.inc"

typedef u32x4 u32x4_a1 __attribute__((aligned(1)));

// dummy symbol and index tiles of dead lanes (zeros; index 0 is a row of every set)
__device__ uint4 g_isink[4];

// 16 index bytes at any alignment (the index stream is congruent to the symbols mod 16 on the
// fast path; any other alignment is one unaligned global load)
static __device__ __forceinline__ uint4 gload16u(const uint8_t* p) {
  const u32x4 v = *(const __attribute__((address_space(1))) u32x4_a1*)p;
  return make_uint4(v.x, v.y, v.z, v.w);
}

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// the (cum, c) entry of symbol s in row j (cuwg_enc_entry).  An index >= K reads row K, the
// poison row (every entry flagged).
template <int LAYOUT>
static __device__ __forceinline__ uint2 set_entry(u32 K, u32 j, u32 s) {
  const u32 row = min(j, K);
  return cuwg_enc_entry<LAYOUT>(LAYOUT == 0 ? row << 11 : row * (4u * SET_ROW_WORDS), s);
}

// 16 symbols and their 16 indexes (one 16-B load each), as enc16: the table entry is read two
// symbols ahead, pairs share one rare test, a flush check after every 8 symbols
template <int DIV, int LAYOUT>
static __device__ __forceinline__ void set_enc16(Enc& e, const ModelArgs& m, u32 K, uint4 v,
                                                 uint4 x, bool act, u32 lane, const u32* wring,
                                                 const EncOut* wout, u32* wrank) {
  u32 w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
  u32 x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
  uint2 t = set_entry<LAYOUT>(K, x0 & 255u, w0 & 255u);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      const uint2 t1 = set_entry<LAYOUT>(K, (x0 >> (8 * (i + 1))) & 255u,
                                         (w0 >> (8 * (i + 1))) & 255u);
      const u32 sn = i < 2 ? (w0 >> (8 * (i + 2))) & 255u : w1 & 255u;
      const u32 xn = i < 2 ? (x0 >> (8 * (i + 2))) & 255u : x1 & 255u;
      const uint2 tn = set_entry<LAYOUT>(K, xn, sn);  // (past the tile's end: a harmless read)
      enc_sym2<DIV, 1>(e, m, t, t1, act, lane, wring, wout, wrank);
      t = tn;
    }
    if (q & 1) enc_flush(e, lane, wring, wout, wrank);
    w0 = w1;
    w1 = w2;
    w2 = w3;
    x0 = x1;
    x1 = x2;
    x2 = x3;
  }
}

// one symbol fetched byte-wise (unaligned head / tail of a chunk)
template <int DIV, int LAYOUT>
static __device__ __forceinline__ void set_enc_byte(Enc& e, const ModelArgs& m, u32 K,
                                                    const uint8_t* sp, const uint8_t* ip, u64 i,
                                                    bool act, u32 lane, const u32* wring,
                                                    const EncOut* wout, u32* wrank) {
  const u32 sym = act ? (u32)sp[i] : 0u;
  const u32 j = act ? (u32)ip[i] : 0u;
  enc_sym<DIV, 1>(e, m, set_entry<LAYOUT>(K, j, sym), act, lane, wring, wout, wrank);
}

// the first symbol of a chunk the reference cannot encode (rare: flagged chunks only).  The
// model is looked up first (models[idx[i]]), then the symbol in it.
// (scalars, not the argument struct by reference: an out-of-line call would copy it to scratch)
static __device__ u32 set_first_error(const u32* rows, u32 K, u32 n_symbols, const uint8_t* sp,
                                      const uint8_t* ip, u64 n) {
  for (u64 i = 0; i < n; ++i) {
    const u32 j = ip[i], s = sp[i];
    if (j >= K) return RC_F_BAD_MODEL;
    if (s >= n_symbols) return RC_F_BAD_SYMBOL;
    const u32* row = rows + j * SET_ROW_WORDS;
    if (row[s + 1] == row[s]) return RC_F_ZERO_FREQ;
  }
  return 0;
}

template <int DIV, int LAYOUT>
__global__ __launch_bounds__(1024) void k_encode_indexed(
    SetArgs a, const uint8_t* __restrict__ syms, const uint8_t* __restrict__ idx,
    const u64* __restrict__ sym_off, u32 n_chunks, uint8_t* __restrict__ out,
    const u64* __restrict__ out_off, u64* __restrict__ out_len, u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS, sized by the plan: the K + 1 rows at address 0, then (1-KiB aligned: a ring
  // column base has no bits in the row field) 8 KiB of rings per wave, the lanes' output
  // geometry and the waves' rank tables
  extern __shared__ __attribute__((aligned(1024))) u32 s_enc[];
  const u32 tid = threadIdx.x, lanes = blockDim.x, K = a.k;
  const ModelArgs& m = a.m;
  if (LAYOUT == 0) {
    for (u32 en = tid; en < (K + 1) * 256u; en += lanes) {
      const u32 row = en >> 8, s = en & 255u;
      uint2 t = make_uint2(RC_F_BAD_MODEL << 24, 1u);
      if (row < K) {
        const u32 c0 = a.rows[row * SET_ROW_WORDS + s], c1 = a.rows[row * SET_ROW_WORDS + s + 1];
        t = s >= m.n ? make_uint2(RC_F_BAD_SYMBOL << 24, 1u)
            : c1 == c0 ? make_uint2(RC_F_ZERO_FREQ << 24, 1u) : make_uint2(c0, c1 - c0);
      }
      s_enc[2 * en] = t.x;
      s_enc[2 * en + 1] = t.y;
    }
  } else {
    for (u32 en = tid; en < (K + 1) * SET_ROW_WORDS; en += lanes)
      s_enc[en] = en < K * SET_ROW_WORDS ? a.rows[en] : 0u;
  }
  const CuwgEncLds l = cuwg_enc_lds(s_enc, a.tab_bytes, lanes);
  const u32 lane = tid & 63, wave = tid >> 6;
  const u32 k = blockIdx.x * lanes + tid;
  const bool live = k < n_chunks;  // dead lanes still take part in the wave's flush rounds
  RC_VGPR_FLOOR_128();

  const CuwgChunk ch = cuwg_enc_begin(&l.out[tid], out, sym_off, out_off, k, live);
  __syncthreads();
  const u32* wring = l.ring + wave * ENC_RING * 64;
  const EncOut* wout = l.out + wave * 64;
  u32* const wrank = l.rank + wave * 64;

  Enc e;
  cuwg_enc_init(e, ch.al, a.tab_bytes, wave, lane);

  const uint8_t* sp = syms + ch.s0;
  const uint8_t* ip = idx + ch.s0;
  // (n <= 2^25 here: the symbol counters are 32-bit, which keeps the tile registers free)
  const u32 nn = (u32)ch.n;
  u32 head = (64 - ((u32)(uintptr_t)sp & 63)) & 63;  // symbols before the first 64-B aligned tile
  if (head > nn) head = nn;
  const u32 ntile = (nn - head) >> 6;
  // head: byte-wise, all lanes in step (flush rounds are wave-wide)
  for (u32 i = 0; __any((int)(i < head)); ++i) {
    set_enc_byte<DIV, LAYOUT>(e, m, K, sp, ip, i, i < head, lane, wring, wout, wrank);
    if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }
  // body, part 1: the tiles every live lane of the wave has, with every lane active; dead lanes
  // run along on a dummy tile and a slot with no writable bytes
  const u32 tmin = cuwg_tmin(live, ntile);
  const uint8_t* tp = live ? sp + head : reinterpret_cast<const uint8_t*>(g_isink);
  const uint8_t* xp = live ? ip + head : reinterpret_cast<const uint8_t*>(g_isink);
  // 64-symbol tiles of symbols and of indexes, 4 x 16 B per lane each, the next tile of both
  // in flight while the current one is coded (explicit registers, as in k_encode_static)
  const u32 tstep = live ? 64 : 0;  // bytes per tile
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
  uint4 x0 = c0, x1 = c0, x2 = c0, x3 = c0;
  if (tmin) {
    const uint4* q = reinterpret_cast<const uint4*>(tp);
    c0 = q[0];
    c1 = q[1];
    c2 = q[2];
    c3 = q[3];
    x0 = gload16u(xp);
    x1 = gload16u(xp + 16);
    x2 = gload16u(xp + 32);
    x3 = gload16u(xp + 48);
  }
  for (u32 t = 0; t < tmin; ++t) {
    rc_prio_rotate(m.prio_rot);
    uint4 n0 = c0, n1 = c1, n2 = c2, n3 = c3, y0 = x0, y1 = x1, y2 = x2, y3 = x3;
    if (t + 1 < tmin) {
      const uint4* q = reinterpret_cast<const uint4*>(tp + (u64)(t + 1) * tstep);
      const uint8_t* xq = xp + (u64)(t + 1) * tstep;
      n0 = q[0];
      n1 = q[1];
      n2 = q[2];
      n3 = q[3];
      y0 = gload16u(xq);
      y1 = gload16u(xq + 16);
      y2 = gload16u(xq + 32);
      y3 = gload16u(xq + 48);
    }
    set_enc16<DIV, LAYOUT>(e, m, K, c0, x0, true, lane, wring, wout, wrank);
    set_enc16<DIV, LAYOUT>(e, m, K, c1, x1, true, lane, wring, wout, wrank);
    set_enc16<DIV, LAYOUT>(e, m, K, c2, x2, true, lane, wring, wout, wrank);
    set_enc16<DIV, LAYOUT>(e, m, K, c3, x3, true, lane, wring, wout, wrank);
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    x0 = y0;
    x1 = y1;
    x2 = y2;
    x3 = y3;
  }
  // body, part 2 (ragged waves): the remaining 16-symbol blocks of the tiles, lanes masked
  const u32 nblk = ntile * 4;
  for (u32 b = tmin * 4; __any((int)(b < nblk)); ++b) {
    const bool act = b < nblk;
    uint4 v = make_uint4(0, 0, 0, 0), x = v;
    if (act) {
      v = reinterpret_cast<const uint4*>(tp)[b];
      x = gload16u(xp + 16ull * b);
    }
    set_enc16<DIV, LAYOUT>(e, m, K, v, x, act, lane, wring, wout, wrank);
  }
  const u32 tail0 = head + (ntile << 6);
  for (u32 j = 0; __any((int)(tail0 + j < nn)); ++j) {  // j is wave-uniform
    set_enc_byte<DIV, LAYOUT>(e, m, K, sp, ip, tail0 + j, tail0 + j < nn, lane, wring, wout,
                              wrank);
    if ((j & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }

  const u32 len = cuwg_enc_finish(e, &l.out[tid], ch.al, lane, wring, wout, wrank);
  if (live)
    cuwg_enc_report(ch, k, len,
                    (e.err >> 24) ? set_first_error(a.rows, K, m.n, sp, ip, ch.n) : 0u, out_len,
                    flags);
}

// ------------------------------------------------------------------------------------------
// Decoder
// ------------------------------------------------------------------------------------------
#ifdef RC_SET_STATS
// Scratch builds only (-DRC_SET_STATS, tools/kbench_indexed.py; not part of the C ABI): how often
// the decoder's wave takes the exact fix-up branch.  g_set_stats[0] counts lane-symbols,
// [1] the lane-symbols on which the lane's wave took the branch (every lane active at the
// branch counts, whether or not its own candidate failed).
__device__ unsigned long long g_set_stats[2];
extern "C" int rc_set_stats_read_(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_set_stats), sizeof g_set_stats) != hipSuccess)
    return -1;
  const unsigned long long zero[2] = {0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_set_stats), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
struct SetDec : Dec<DEC_LD, 0> {
  u32 st_steps, st_fix;
};
#else
typedef Dec<DEC_LD, 0> SetDec;
#endif

// Decoder::decode(&models[j]) with FreqTable::find_index over row j: the hint q from the carried
// scale G (row-independent: the total is shared), row j's two-candidate bucket, the candidate's
// (cum, c) from the cum-only row, the exact u64 verification r cum <= x < r (cum + c), and the
// wave-uniform exact fix-up (cuwg_dec_fix over row j) when a lane's candidate fails it.  j < K.
template <int DIV>
static __device__ __forceinline__ u32 set_dec_sym(SetDec& d, const SetArgs& a, u32 rows_off,
                                                  u32 j) {
  const ModelArgs& m = a.m;
  u32 roff, raddr;
  asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
  asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(raddr) : "v"(roff), "v"((u32)(uintptr_t)d.ring));
  const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
  const u32 D0 = rp[0], D1 = rp[SetDec::kS];
  const u64 r = range_par_total<DIV, 1>(d.range, m);
  const float X = (float)(d.dhi() - hi32(d.low));
  const u32 qh = hint_floor(X, d.G);
  // row j's bucket (the buckets are at LDS address 0, 2^lut_bits 4-B entries per row): s0 holds
  // the bucket's first frequency, s1 is the next symbol with c > 0 that starts inside the
  // bucket, taken from cum[s1] on (s1 = s0 and cum 0 without one)
  const u32 la = (j << (m.lut_bits + 2)) + (__builtin_amdgcn_ubfe(qh, m.lut_shift, m.lut_bits) << 2);
  const u32 ent = *(const l_u32*)(uintptr_t)la;
  const u32 below = smask((qh & 0xFFFFu) - (ent >> 16));
  u32 s = __builtin_amdgcn_ubfe(ent, mselc(below, 0u, 8u), 8);
  const u32 rowa = rows_off + j * (4u * SET_ROW_WORDS);
  uint2 t = cuwg_cum_entry(rowa, s);
  float tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));  // (hint only)
  u64 B = mul_rv<1>(r, t.y);
  u64 A = mul_rv<1>(r, t.x);
  const u64 dx = sub64((u32)d.dat, d.dhi(), d.low + A);  // x - r cum
#ifdef RC_SET_STATS
  d.st_steps += 1;
#endif
  if (__builtin_expect(__any((int)(dx >= B)), 0)) {
#ifdef RC_SET_STATS
    d.st_fix += 1;
#endif
    if (dx >= B) {
      cuwg_dec_fix<true>(s, t, A, B, d.x(), r, rowa, m.n);
      tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));
      // the buckets only hold symbols with c > 0, so c == 0 can only come from the fix-up: corrupt
      // input (the reference loops forever); an over-read, if any, came first
      if (t.y == 0) {
        d.err = d.err ? d.err : (d.bpos > d.limb ? RC_F_TRUNCATED : RC_F_CORRUPT);
        B = r;
      }
    }
  }
  dec_apply<1, 4>(d, d.low + A, B, d.dat, tc, D0, D1, 0u);
  const bool rare = hi32(d.range) < 0x10000u;  // range_reduction_expansion
  if (__builtin_expect(__any((int)rare), 0)) {
    if (rare) {
      dec_rare(d, DEC_NEED_SM);
      dec_gexact<1, 4>(d, m);
    }
  }
  return s;
}

// one symbol with the index checked: an index >= K flags the chunk (unless an earlier error or
// an over-read came first) and decodes on with row 0, so that nothing out of bounds is touched
template <int DIV>
static __device__ __forceinline__ u32 set_dec_sym_checked(SetDec& d, const SetArgs& a,
                                                          u32 rows_off, u32 j) {
  if (j >= a.k) {
    d.err = d.err ? d.err : (d.bpos > d.limb ? RC_F_TRUNCATED : RC_F_BAD_MODEL);
    j = 0;
  }
  return set_dec_sym<DIV>(d, a, rows_off, j);
}

// some byte of w is >= K (1 <= K <= 64)
static __device__ __forceinline__ bool any_byte_ge(u32 w, u32 K) {
  return ((((w & 0x7F7F7F7Fu) + (0x80u - K) * 0x01010101u) | w) & 0x80808080u) != 0;
}

// 16 symbols into one 16-B block, with the ring checks; x: their 16 indexes
template <int DIV>
static __device__ __forceinline__ uint4 set_phase16(SetDec& d, const SetArgs& a, u32 rows_off,
                                                    uint4 x) {
  dec_gexact<1, 4>(d, a.m);  // bounds the drift of the carried scale to 16 symbols
  const bool bad = any_byte_ge(x.x, a.k) | any_byte_ge(x.y, a.k) | any_byte_ge(x.z, a.k) |
                   any_byte_ge(x.w, a.k);
  if (__builtin_expect(__any((int)bad), 0)) {
    // (rare: a flagged chunk in the wave) symbol by symbol, every index checked; rolled, the
    // words rotate down instead of being indexed
    u32 x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w, o0 = 0, o1 = 0, o2 = 0, o3 = 0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      u32 w = 0;
#pragma unroll 1
      for (int jj = 0; jj < 4; ++jj) {
        w = (w >> 8) | (set_dec_sym_checked<DIV>(d, a, rows_off, x0 & 255u) << 24);
        x0 >>= 8;
      }
      dec_check4<1>(d);
      o0 = o1;
      o1 = o2;
      o2 = o3;
      o3 = w;
      x0 = x1;
      x1 = x2;
      x2 = x3;
    }
    dec_check4<1, DEC_NEED_SPAN>(d);
    return make_uint4(o0, o1, o2, o3);
  }
  const u32 xw[4] = {x.x, x.y, x.z, x.w};
  u32 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
      w[q] = put_byte(w[q], set_dec_sym<DIV>(d, a, rows_off, (xw[q] >> (8 * jj)) & 255u), jj);
    if (q < 3 && ((q + 1) * 4) % DEC_CHECK_SPAN == 0) dec_check4<1, DEC_NEED_SPAN>(d);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DIV>
__global__ __launch_bounds__(1024) void k_decode_indexed(
    SetArgs a, const uint8_t* __restrict__ code, const u64* __restrict__ code_off,
    const u64* __restrict__ code_len, const uint8_t* __restrict__ idx,
    uint8_t* __restrict__ syms_out, const u64* __restrict__ sym_off, u32 n_chunks,
    u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS, sized by the plan: the K rows' buckets at address 0 (a bucket read needs no
  // base add), the K cum-only rows, then the code rings
  extern __shared__ u32 s_dyn[];
  const u32 tid = threadIdx.x, lanes = blockDim.x, K = a.k;
  const ModelArgs& m = a.m;
  const u32 lut_words = K << m.lut_bits;
  for (u32 j = tid; j < lut_words; j += lanes) s_dyn[j] = a.lut[j];
  for (u32 j = tid; j < K * SET_ROW_WORDS; j += lanes) s_dyn[lut_words + j] = a.rows[j];
  __syncthreads();
  const u32 k = blockIdx.x * lanes + tid;
  if (k >= n_chunks) return;
  // f32 rounding toward zero from here on (MODE.FP_ROUND f32 bits = 3), for hint_floor
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3");
  RC_VGPR_FLOOR_128();
  const u32 lane = tid & 63, wave = tid >> 6;
  const u32 rows_off = 4u * lut_words;

  const u64 c0 = code_off[k];
  const u64 clen = code_len[k];
  const u64 s0 = sym_off[k];
  const u64 n64 = sym_off[k + 1] - s0;
  uint8_t* op = syms_out + s0;
  const uint8_t* ip = idx + s0;
  if (n64 > RC_MAX_CHUNK_SYMBOLS) {  // 32-bit stream positions (include/range_coder.h)
    flags[k] = RC_F_TOO_LONG;
    return;
  }
  if (clen < 8) {  // Decoder::new panics (decoder.rs:21, :33)
    flags[k] = RC_F_TRUNCATED;
    return;
  }
  const u32 n = (u32)n64;  // (<= 2^25: the counters below are 32-bit)
  const uint8_t* cp = code + c0;
  constexpr u32 GAL = 16 * DEC_LD;  // load bursts are whole aligned 64-B segments
  const u32 al = (u32)((uintptr_t)cp & (GAL - 1));

  SetDec d;
#ifdef RC_SET_STATS
  d.st_steps = d.st_fix = 0;
#endif
  d.low = 0;
  d.range = ~0ull;
  d.err = 0;
  d.fillb = 0;
  d.pend_ok = 0;
  d.ring = (l_u32*)(uintptr_t)(rows_off + 4u * K * SET_ROW_WORDS) + wave * DEC_RING_ALLOC * 64 +
           lane;
  d.gbase = reinterpret_cast<const uint4*>(cp - al);
  d.gnext = 0;
  // n <= 2^25 symbols consume at most 8 + 12 n < 2^29 bytes: code past 2^29 is never read
  const u32 lim = (u32)(clen < (1ull << 29) - al ? al + clen : 1ull << 29);
  d.glast = ((lim - 1) >> 4) & ~(u32)(DEC_LD - 1);  // (the last segment's first block)
  d.bpos = 8 * (al + 8);  // Decoder::new primes 8 bytes (decoder.rs:21)
  d.limb = 8 * lim;
  // fill the whole ring, and have the next load burst in flight (as k_decode_static)
#pragma unroll
  for (int h = 0; h < DEC_RING / (4 * DEC_PF); ++h) {
    if (!d.pend_ok) dec_issue(d);
    dec_commit(d);
  }
  while ((int)(d.fillb - d.bpos) < (int)(8 * DEC_NEED_HEAD)) {
    if (!d.pend_ok) dec_issue(d);
    dec_commit(d);
  }
  if (!d.pend_ok) dec_issue(d);
  d.set_data(dec_read8_before(d));  // Decoder::new's data (low = 0)
  dec_gexact<1, 4>(d, m);

  u32 i = 0;
  // head: single symbols until the output is 64-B aligned
  constexpr u32 OUT_ALIGN = 16 * DEC_OUT_BURST;
  static_assert(DEC_OUT_BURST == 4, "bursts of four phases");
  u32 head = (OUT_ALIGN - ((u32)(uintptr_t)op & (OUT_ALIGN - 1))) & (OUT_ALIGN - 1);
  if (head > n) head = n;
  dec_check4<1>(d);
  for (; i < head; ++i) {
    op[i] = (uint8_t)set_dec_sym_checked<DIV>(d, a, rows_off, ip[i]);
    dec_check4<1>(d);
  }
  dec_check4<1, DEC_NEED_SPAN>(d);
  // body: 16-symbol phases.  The indexes are side information, known in advance: the 16 of the
  // next phase are loaded while the current one is decoded, like the code ring's refills.
  uint4* ob = reinterpret_cast<uint4*>(op + i);
  const uint8_t* ib = ip + i;
  const u32 nfull = (n - i) >> 4;  // whole phases (bursts of four, then single ones)
  const u32 nbu = nfull / DEC_OUT_BURST;
  uint4 xc = make_uint4(0, 0, 0, 0);
  if (nfull) xc = gload16u(ib);
  u32 g = 0;  // phase
#define RC_SET_PHASE(o)                                                         \
  const uint4 xn_##o = gload16u(ib + 16 * min(g + 1, nfull - 1));       \
  const uint4 o = set_phase16<DIV>(d, a, rows_off, xc);                         \
  xc = xn_##o;                                                                  \
  ++g;                                                                          \
  dec_phase(d);                                                                 \
  dec_check4<1, DEC_NEED_SPAN>(d);
  for (u32 b = 0; b < nbu; ++b) {
    rc_prio_rotate(m.prio_rot);
    RC_SET_PHASE(o0) RC_SET_PHASE(o1) RC_SET_PHASE(o2) RC_SET_PHASE(o3)
    uint4* ob_b = ob + DEC_OUT_BURST * b;
    ob_b[0] = o0;
    ob_b[1] = o1;
    ob_b[2] = o2;
    ob_b[3] = o3;
  }
  while (g < nfull) {
    const u32 gb = g;
    RC_SET_PHASE(o)
    ob[gb] = o;
  }
#undef RC_SET_PHASE
  i += nfull << 4;
  for (; i < n; ++i) {
    op[i] = (uint8_t)set_dec_sym_checked<DIV>(d, a, rows_off, ip[i]);
    dec_check4<1>(d);
  }
#ifdef RC_SET_STATS
  atomicAdd(&g_set_stats[0], (unsigned long long)d.st_steps);
  atomicAdd(&g_set_stats[1], (unsigned long long)d.st_fix);
#endif
  flags[k] = cuwg_dec_flag(d);
}

// ------------------------------------------------------------------------------------------
// Host: the plan and the launchers
// ------------------------------------------------------------------------------------------
void rc_set_plan(u32 K, u32 total, SetPlan* p) {
  memset(p, 0, sizeof *p);
  if (K < 1 || K > RC_MAX_SET_MODELS || total < 256 || total > 65536) return;
  // encoder: as many lanes as fit beside the K + 1 rows (the register allocation allows 1,024
  // per CU); at equal lanes the 8-B entries, which cost the symbol step less
  for (u32 lanes = 1024; lanes >= 256 && !p->enc_lanes; lanes -= 256) {
    const u32 rings = lanes * SET_ENC_LANE_BYTES;
    const u32 t8 = (K + 1) * 2048u;
    const u32 t4 = ((K + 1) * 4u * SET_ROW_WORDS + 1023u) & ~1023u;
    if (t8 + rings <= SET_LDS_BYTES) {
      p->enc_lanes = lanes;
      p->enc_layout = 0;
      p->enc_tab = t8;
    } else if (t4 + rings <= SET_LDS_BYTES) {
      p->enc_lanes = lanes;
      p->enc_layout = 1;
      p->enc_tab = t4;
    }
    p->enc_lds = p->enc_tab + rings;
  }
  // decoder: K cum-only rows and 2^bits 4-B buckets per row beside the rings; bits is capped by
  // 2^12 (the single-table decoders' finest) and by the total.  The first of 1,024, 768 and 512
  // lanes that leaves the rows at least 2^8 buckets, else the one that leaves them the most.
  cuwg_dec_plan(p, total, K * 4u * SET_ROW_WORDS, K, 8u);
}

// The indexed kernels (and the wide ones, rc_wide.hip) take up to a whole CU's LDS as dynamic
// LDS: allowed once per (device, kernel), not per launch; a refusal is the launch's error.
hipError_t set_allow_lds(const void* kernel) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({dev, kernel})) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)SET_LDS_BYTES);
  if (e == hipSuccess) done.insert({dev, kernel});
  return e;
}

// Lanes per workgroup of a launch: the plan's, which is what one CU holds, unless the launch's
// chunks would then leave CUs idle; then smaller workgroups (never under 256 lanes) so that the
// grid reaches every CU, each staging the tables for itself.
u32 set_launch_lanes(u32 plan_lanes, u32 n_chunks) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    return plan_lanes;
  const u32 per = ((n_chunks + (u32)cus - 1) / (u32)cus + 63u) & ~63u;
  return per < 256u ? (plan_lanes < 256u ? plan_lanes : 256u) : (per < plan_lanes ? per : plan_lanes);
}

hipError_t rc_set_encode_launch(hipStream_t stream, const RcKnobs& k, const SetArgs& a_in,
                                int div, const SetPlan& p, const uint8_t* syms,
                                const uint8_t* idx, const u64* sym_off, u32 n_chunks,
                                uint8_t* out, const u64* out_off, u64* out_len, u32* flags) {
  SetArgs a = a_in;
  a.tab_bytes = p.enc_tab;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioEncoder, p.enc_lanes, SET_ENC_LANE_BYTES,
                       p.enc_lds, n_chunks, syms, idx, sym_off, n_chunks, out, out_off, out_len,
                       flags);
  };
  if (div == DIV_POW2)
    return p.enc_layout == 0 ? go(k_encode_indexed<DIV_POW2, 0>) : go(k_encode_indexed<DIV_POW2, 1>);
  return p.enc_layout == 0 ? go(k_encode_indexed<DIV_MAGIC, 0>) : go(k_encode_indexed<DIV_MAGIC, 1>);
}

hipError_t rc_set_decode_launch(hipStream_t stream, const RcKnobs& k, const SetArgs& a_in,
                                int div, const SetPlan& p, const uint8_t* code,
                                const u64* code_off, const u64* code_len, const uint8_t* idx,
                                uint8_t* syms_out, const u64* sym_off, u32 n_chunks,
                                u32* flags) {
  SetArgs a = a_in;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioDecoder512, p.dec_lanes, SET_DEC_LANE_BYTES,
                       p.dec_lds, n_chunks, code, code_off, code_len, idx, syms_out, sym_off,
                       n_chunks, flags);
  };
  return div == DIV_POW2 ? go(k_decode_indexed<DIV_POW2>) : go(k_decode_indexed<DIV_MAGIC>);
}
