// rc_wide.hip — k_encode_wide / k_decode_wide: the small-model static coders over one table of up
// to RC_MAX_WIDE_SYMBOLS 16-bit symbols (wide static models, rc_wide.h).  Symbol i of a chunk is
// coded exactly as encoder.encode(&table, sym[i]) / decoder.decode(&table).  The arithmetic, the
// encoder's accumulator, ring and ranked flush rounds and the decoder's code ring, dec_apply and
// dec_rare are those of the single-table coders (rc_encode.inc, rc_decode.inc, rc_static.h); what
// is new is the 16-bit symbol stream, a table of up to 32 KiB staged once by one large workgroup
// per CU, and the decoder's index search: a bucket names a range of symbols, not two candidates.
#define RC_DEC_SHARED_ONLY
#include "rc_wide.h"

#include "rc_encode.inc"
#include "rc_decode.inc"

typedef u32 u32x2 __attribute__((ext_vector_type(2)));

// dummy symbol tile of dead lanes (zeros: symbol 0 is in every alphabet)
__device__ uint4 g_wsink[4];

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// the (cum, c) entry of symbol s, in enc_core's SM 1 form: a symbol the reference cannot encode
// carries a flag byte above its cum and c = 1.  A symbol >= n reads entry n.  Layout 0: the 8-B
// entry as staged (entry n the poison entry), one ds_read_b64.  Layout 1: the cum-only row,
// c = cum[s + 1] - cum[s] (one ds_read2_b32); c = 0 covers zero frequencies and symbols past the
// alphabet (cum[n] = cum[n + 1] = total) alike.
template <int LAYOUT>
static __device__ __forceinline__ uint2 wide_entry(u32 n, u32 s) {
  const u32 sc = min(s, n);
  if (LAYOUT == 0) {
    const u32x2 v = *(const __attribute__((address_space(3))) u32x2*)(uintptr_t)(sc << 3);
    return make_uint2(v.x, v.y);
  }
  const l_u32* rp = (const l_u32*)(uintptr_t)(sc << 2);
  const u32 c0 = rp[0], c1 = rp[1];
  const u32 c = c1 - c0;
  return make_uint2(c0 | ((c - 1u) & 0xFF000000u), max(c, 1u));
}

// 8 symbols from one 16-B load, as enc16's quarters: the table entry is read two symbols ahead,
// pairs share one rare test, a flush check after the 8 symbols
template <int DIV, int LAYOUT>
static __device__ __forceinline__ void wide_enc8(Enc& e, const ModelArgs& m, uint4 v, bool act,
                                                 u32 lane, const u32* wring, const EncOut* wout,
                                                 u32* wrank) {
  const u32 w[4] = {v.x, v.y, v.z, v.w};
  uint2 t = wide_entry<LAYOUT>(m.n, w[0] & 0xFFFFu);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint2 t1 = wide_entry<LAYOUT>(m.n, w[p] >> 16);
    const uint2 tn = p < 3 ? wide_entry<LAYOUT>(m.n, w[p + 1] & 0xFFFFu) : t1;
    enc_sym2<DIV, 1>(e, m, t, t1, act, lane, wring, wout, wrank);
    t = tn;
  }
  enc_flush(e, lane, wring, wout, wrank);
}

// one symbol fetched on its own (unaligned head / tail of a chunk)
template <int DIV, int LAYOUT>
static __device__ __forceinline__ void wide_enc_one(Enc& e, const ModelArgs& m,
                                                    const uint16_t* sp, u32 i, bool act, u32 lane,
                                                    const u32* wring, const EncOut* wout,
                                                    u32* wrank) {
  const u32 sym = act ? (u32)sp[i] : 0u;
  enc_sym<DIV, 1>(e, m, wide_entry<LAYOUT>(m.n, sym), act, lane, wring, wout, wrank);
}

// the first symbol of a chunk the reference cannot encode (rare: flagged chunks only)
// (scalars, not the argument struct by reference: an out-of-line call would copy it to scratch)
static __device__ u32 wide_first_error(const u32* row, u32 n_symbols, const uint16_t* sp, u64 n) {
  for (u64 i = 0; i < n; ++i) {
    const u32 s = sp[i];
    if (s >= n_symbols) return RC_F_BAD_SYMBOL;
    if (row[s + 1] == row[s]) return RC_F_ZERO_FREQ;
  }
  return 0;
}

template <int DIV, int LAYOUT>
__global__ __launch_bounds__(1024) void k_encode_wide(
    WideArgs a, const uint16_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_chunks,
    uint8_t* __restrict__ out, const u64* __restrict__ out_off, u64* __restrict__ out_len,
    u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS, sized by the plan: the table at address 0, then (1-KiB aligned: a ring column
  // base has no bits in the row field) 8 KiB of rings per wave, the lanes' output geometry and
  // the waves' rank tables
  extern __shared__ __attribute__((aligned(1024))) u32 s_enc[];
  const u32 tid = threadIdx.x, lanes = blockDim.x;
  const ModelArgs& m = a.m;
  if (LAYOUT == 0) {
    for (u32 s = tid; s <= m.n; s += lanes) {
      uint2 t = make_uint2(RC_F_BAD_SYMBOL << 24, 1u);
      if (s < m.n) {
        const u32 c0 = a.row[s], c1 = a.row[s + 1];
        t = c1 == c0 ? make_uint2(RC_F_ZERO_FREQ << 24, 1u) : make_uint2(c0, c1 - c0);
      }
      s_enc[2 * s] = t.x;
      s_enc[2 * s + 1] = t.y;
    }
  } else {
    for (u32 s = tid; s < m.n + 2; s += lanes) s_enc[s] = a.row[s];
  }
  const u32 nw = lanes >> 6;
  u32* const s_ring = s_enc + a.tab_bytes / 4;
  EncOut* const s_out = reinterpret_cast<EncOut*>(s_ring + nw * ENC_RING * 64);
  u32* const s_rank = reinterpret_cast<u32*>(s_out + lanes);
  const u32 lane = tid & 63, wave = tid >> 6;
  const u32 k = blockIdx.x * lanes + tid;
  const bool live = k < n_chunks;  // dead lanes still take part in the wave's flush rounds
  RC_VGPR_FLOOR_128();

  u64 s0 = 0, n = 0, o0 = 0, o1 = 0;
  if (live) {
    s0 = sym_off[k];
    n = sym_off[k + 1] - s0;
    o0 = out_off[k];
    o1 = out_off[k + 1];
  }
  // B (bit position) is 32-bit: a longer chunk is flagged, not read, and its slot not written
  const bool too_long = n > RC_MAX_CHUNK_SYMBOLS;
  if (too_long) {
    n = 0;
    o1 = o0;
  }
  const u32 al = (u32)(((uintptr_t)out + o0) & (ENC_UNIT - 1));
  u64 cap = o1 - o0;
  if (cap > 0xFFFFFF00ull - al) cap = 0xFFFFFF00ull - al;
  s_out[tid].gbase = out + o0 - al;
  s_out[tid].lo_ok = al;
  s_out[tid].hi_ok = al + (u32)cap;
  __syncthreads();
  const u32* wring = s_ring + wave * ENC_RING * 64;
  const EncOut* wout = s_out + wave * 64;
  u32* const wrank = s_rank + wave * 64;

  Enc e;
  e.low = 0;  // RangeCoder::default (range_coder.rs:13-20)
  e.range = ~0ull;
  e.acc = 0;
  e.B = 8 * al;  // pad bytes in front of the slot (never stored)
  e.fthr = 8u * FLUSH_AT;  // fpos = 0
  e.err = 0;
  e.ring = a.tab_bytes + 4u * (wave * ENC_RING * 64 + ring_col(lane));

  const uint16_t* sp = syms + s0;
  // (n <= 2^25 here: the symbol counters are 32-bit, which keeps the tile registers free)
  const u32 nn = (u32)n;
  // symbols before the first 64-B aligned tile (the stream is 2-B aligned)
  u32 head = ((64 - ((u32)(uintptr_t)sp & 63)) & 63) >> 1;
  if (head > nn) head = nn;
  const u32 ntile = (nn - head) >> 5;  // 64-B tiles of 32 symbols
  // head: symbol-wise, all lanes in step (flush rounds are wave-wide)
  for (u32 i = 0; __any((int)(i < head)); ++i) {
    wide_enc_one<DIV, LAYOUT>(e, m, sp, i, i < head, lane, wring, wout, wrank);
    if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }
  // body, part 1: the tiles every live lane of the wave has, with every lane active; dead lanes
  // run along on a dummy tile and a slot with no writable bytes
  u32 tm = live ? ntile : ~0u;
#pragma unroll
  for (int o = 32; o; o >>= 1) tm = min(tm, (u32)__shfl_xor((int)tm, o));
  if (tm == ~0u) tm = 0;  // no live lane in this wave
  const u32 tmin = __builtin_amdgcn_readfirstlane(tm);  // wave-uniform (scalar) trip count
  const uint8_t* tp = live ? reinterpret_cast<const uint8_t*>(sp + head)
                           : reinterpret_cast<const uint8_t*>(g_wsink);
  // 32-symbol tiles, 4 x 16 B per lane, the next tile in flight while the current one is coded
  // (explicit registers, as in k_encode_static)
  const u32 tstep = live ? 64 : 0;  // bytes per tile
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
  if (tmin) {
    const uint4* q = reinterpret_cast<const uint4*>(tp);
    c0 = q[0];
    c1 = q[1];
    c2 = q[2];
    c3 = q[3];
  }
  for (u32 t = 0; t < tmin; ++t) {
    rc_prio_rotate(m.prio_rot);
    uint4 n0 = c0, n1 = c1, n2 = c2, n3 = c3;
    if (t + 1 < tmin) {
      const uint4* q = reinterpret_cast<const uint4*>(tp + (u64)(t + 1) * tstep);
      n0 = q[0];
      n1 = q[1];
      n2 = q[2];
      n3 = q[3];
    }
    wide_enc8<DIV, LAYOUT>(e, m, c0, true, lane, wring, wout, wrank);
    wide_enc8<DIV, LAYOUT>(e, m, c1, true, lane, wring, wout, wrank);
    wide_enc8<DIV, LAYOUT>(e, m, c2, true, lane, wring, wout, wrank);
    wide_enc8<DIV, LAYOUT>(e, m, c3, true, lane, wring, wout, wrank);
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
  }
  // body, part 2 (ragged waves): the remaining 8-symbol blocks of the tiles, lanes masked
  const u32 nblk = ntile * 4;
  for (u32 b = tmin * 4; __any((int)(b < nblk)); ++b) {
    const bool act = b < nblk;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (act) v = reinterpret_cast<const uint4*>(tp)[b];
    wide_enc8<DIV, LAYOUT>(e, m, v, act, lane, wring, wout, wrank);
  }
  const u32 tail0 = head + (ntile << 5);
  for (u32 j = 0; __any((int)(tail0 + j < nn)); ++j) {  // j is wave-uniform
    wide_enc_one<DIV, LAYOUT>(e, m, sp, tail0 + j, tail0 + j < nn, lane, wring, wout, wrank);
    if ((j & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }

  // Encoder::finish (encoder.rs:40-46): 8 x left_shift
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
  if (end < s_out[tid].hi_ok) s_out[tid].hi_ok = end;
  while (__any((int)(enc_fpos(e) < wend)))
    enc_round(e, enc_fpos(e) < wend, lane, wring, wout, wrank);
  if (live) {
    e.err = (e.err >> 24) ? wide_first_error(a.row, m.n, sp, n) : 0u;
    if (!e.err && (u64)len > cap) e.err = RC_F_CAPACITY;
    out_len[k] = too_long ? 0u : len;
    flags[k] = too_long ? RC_F_TOO_LONG : e.err;
  }
}

// ------------------------------------------------------------------------------------------
// Decoder
// ------------------------------------------------------------------------------------------
#ifdef RC_WIDE_STATS
// Scratch builds only (-DRC_WIDE_STATS, tools/kbench_wide.py; not part of the C ABI): how often
// the decoder's wave takes the exact-walk branch.  g_wide_stats[0] counts lane-symbols, [1] the
// lane-symbols on which the lane's wave took the branch.
__device__ unsigned long long g_wide_stats[2];
extern "C" int rc_wide_stats_read_(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide_stats), sizeof g_wide_stats) != hipSuccess)
    return -1;
  const unsigned long long zero[2] = {0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_wide_stats), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
struct WideDec : Dec<DEC_LD, 0> {
  u32 st_steps, st_fix;
};
#else
typedef Dec<DEC_LD, 0> WideDec;
#endif

// (cum, c) of symbol s from the cum-only row at LDS byte address rowa: c = cum[s + 1] - cum[s]
// (the row holds cum[0 .. n], cum[n] the total), one ds_read2_b32
static __device__ __forceinline__ uint2 wide_row_entry(u32 rowa, u32 s) {
  const l_u32* rp = (const l_u32*)(uintptr_t)(rowa + (s << 2));
  const u32 c0 = rp[0], c1 = rp[1];
  return make_uint2(c0, c1 - c0);
}

// dec_fix (rc_decode.inc) over the wide cum-only row: the exact index s = #{ j in [1, n-1] :
// r * cum[j] <= x } (FreqTable::find_index), walked from the candidate.  A copy, not a second
// form of dec_fix or set_dec_fix (which mask the symbol to 8 bits): changing those changes the
// generated code of the existing kernels.
static __device__ __forceinline__ void wide_dec_fix(u32& s, uint2& t, u64& A, u64& B, u64 x,
                                                    u64 r, u32 rowa, u32 n) {
  if (A > x) {
    do {  // (ends at s = 0 at the latest: cum[0] = 0)
      --s;
      t = wide_row_entry(rowa, s);
      A = r * (u64)t.x;
    } while (A > x);
    B = r * (u64)t.y;
  } else {
    while (s + 1 < n && x - A >= B) {
      ++s;
      t = wide_row_entry(rowa, s);
      A = r * (u64)t.x;
      B = r * (u64)t.y;
    }
  }
}

// Decoder::decode(&table) with FreqTable::find_index: the hint q from the carried scale G, q's
// bucket (the buckets are at LDS address 0), which names the symbols [s_lo, s_hi] that find_index
// returns for the bucket's frequencies, a binary search for the last symbol of that range whose
// cum is <= q (strides from a.top_stride down, the count that settles the table's widest bucket,
// so the loop is wave-uniform and scalar; a settled lane probes on without moving), the
// candidate's (cum, c), the exact u64 verification r cum <= x < r (cum + c), and the exact walk
// (wide_dec_fix) when a lane's candidate fails it.  Every probe stays inside [s_lo, s_hi],
// whatever the hint.
template <int DIV>
static __device__ __forceinline__ u32 wide_dec_sym(WideDec& d, const WideArgs& a, u32 rowa) {
  const ModelArgs& m = a.m;
  u32 roff, raddr;
  asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
  asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(raddr) : "v"(roff), "v"((u32)(uintptr_t)d.ring));
  const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
  const u32 D0 = rp[0], D1 = rp[WideDec::kS];
  const u64 r = range_par_total<DIV, 1>(d.range, m);
  const float X = (float)(d.dhi() - hi32(d.low));
  const u32 qh = hint_floor(X, d.G);
  const u32 q = qh & 0x3FFFFFu;
  const u32 ent =
      *(const l_u32*)(uintptr_t)(__builtin_amdgcn_ubfe(qh, m.lut_shift, m.lut_bits) << 2);
  u32 s = ent & 0xFFFFu;
  const u32 hi = ent >> 16;
  // the last symbol in [s, hi] whose cum is <= q (s itself when there is none: a hint that was
  // off), by strides that halve: the probe is min(s + stride, hi), so it never leaves the range
  for (u32 stride = a.top_stride; stride; stride >>= 1) {
    const u32 cand = min(s + stride, hi);
    const u32 cm = *(const l_u32*)(uintptr_t)(rowa + (cand << 2));
    s = mselc(smask(q - cm), s, cand);  // (sign set: cum[cand] > q; both are below 2^23)
  }
  uint2 t = wide_row_entry(rowa, s);
  float tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));  // (hint only)
  u64 B = mul_rv<1>(r, t.y);
  u64 A = mul_rv<1>(r, t.x);
  const u64 dx = sub64((u32)d.dat, d.dhi(), d.low + A);  // x - r cum
#ifdef RC_WIDE_STATS
  d.st_steps += 1;
#endif
  if (__builtin_expect(__any((int)(dx >= B)), 0)) {
#ifdef RC_WIDE_STATS
    d.st_fix += 1;
#endif
    if (dx >= B) {
      wide_dec_fix(s, t, A, B, d.x(), r, rowa, m.n);
      tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));
      // the search only lands on symbols with c > 0, so c == 0 can only come from the walk:
      // corrupt input (the reference loops forever); an over-read, if any, came first
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

// 8 symbols into one 16-B block (half j of word q = symbol 2q + j)
template <int DIV>
static __device__ __forceinline__ uint4 wide_block8(WideDec& d, const WideArgs& a, u32 rowa) {
  u32 w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32 s0 = wide_dec_sym<DIV>(d, a, rowa);
    const u32 s1 = wide_dec_sym<DIV>(d, a, rowa);
    w[q] = s0 | (s1 << 16);
    if (q == 1 && DEC_CHECK_SPAN == 4) dec_check4<1, DEC_NEED_SPAN>(d);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DIV>
__global__ __launch_bounds__(1024) void k_decode_wide(
    WideArgs a, const uint8_t* __restrict__ code, const u64* __restrict__ code_off,
    const u64* __restrict__ code_len, uint16_t* __restrict__ syms_out,
    const u64* __restrict__ sym_off, u32 n_chunks, u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS, sized by the plan: the buckets at address 0 (a bucket read needs no base add),
  // the cum-only row cum[0 .. n], then the code rings
  extern __shared__ u32 s_dyn[];
  const u32 tid = threadIdx.x, lanes = blockDim.x;
  const ModelArgs& m = a.m;
  const u32 lut_words = 1u << m.lut_bits, row_words = m.n + 1;
  for (u32 j = tid; j < lut_words; j += lanes) s_dyn[j] = a.lut[j];
  for (u32 j = tid; j < row_words; j += lanes) s_dyn[lut_words + j] = a.row[j];
  __syncthreads();
  const u32 k = blockIdx.x * lanes + tid;
  if (k >= n_chunks) return;
  // f32 rounding toward zero from here on (MODE.FP_ROUND f32 bits = 3), for hint_floor
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3");
  RC_VGPR_FLOOR_128();
  const u32 lane = tid & 63, wave = tid >> 6;
  const u32 rowa = 4u * lut_words;

  const u64 c0 = code_off[k];
  const u64 clen = code_len[k];
  const u64 s0 = sym_off[k];
  const u64 n64 = sym_off[k + 1] - s0;
  uint16_t* op = syms_out + s0;
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

  WideDec d;
#ifdef RC_WIDE_STATS
  d.st_steps = d.st_fix = 0;
#endif
  d.low = 0;
  d.range = ~0ull;
  d.err = 0;
  d.fillb = 0;
  d.pend_ok = 0;
  d.ring = (l_u32*)(uintptr_t)(rowa + 4u * row_words) + wave * DEC_RING_ALLOC * 64 + lane;
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
  // head: single symbols until the output is 64-B aligned (it is 2-B aligned)
  u32 head = ((64 - ((u32)(uintptr_t)op & 63)) & 63) >> 1;
  if (head > n) head = n;
  dec_check4<1>(d);
  for (; i < head; ++i) {
    op[i] = (uint16_t)wide_dec_sym<DIV>(d, a, rowa);
    dec_check4<1>(d);
  }
  dec_check4<1, DEC_NEED_SPAN>(d);
  // body: 16-symbol phases of two 16-B blocks, written in 64-B bursts of two phases
  uint4* ob = reinterpret_cast<uint4*>(op + i);
  const u32 nfull = (n - i) >> 4;  // whole phases (bursts of two, then a single one)
#define RC_WIDE_PHASE(oa, ob_)                          \
  dec_gexact<1, 4>(d, m);                               \
  const uint4 oa = wide_block8<DIV>(d, a, rowa);        \
  dec_check4<1, DEC_NEED_SPAN>(d);                      \
  const uint4 ob_ = wide_block8<DIV>(d, a, rowa);       \
  dec_phase(d);                                         \
  dec_check4<1, DEC_NEED_SPAN>(d);
  for (u32 b = 0; b < nfull / 2; ++b) {
    rc_prio_rotate(m.prio_rot);
    RC_WIDE_PHASE(o0, o1) RC_WIDE_PHASE(o2, o3)
    uint4* ob_b = ob + 4 * b;
    ob_b[0] = o0;
    ob_b[1] = o1;
    ob_b[2] = o2;
    ob_b[3] = o3;
  }
  if (nfull & 1) {
    RC_WIDE_PHASE(o0, o1)
    uint4* ob_b = ob + 2 * (nfull - 1);
    ob_b[0] = o0;
    ob_b[1] = o1;
  }
#undef RC_WIDE_PHASE
  i += nfull << 4;
  for (; i < n; ++i) {
    op[i] = (uint16_t)wide_dec_sym<DIV>(d, a, rowa);
    dec_check4<1>(d);
  }
  // shift_left_buffer panics once more bytes are needed than the stream holds (decoder.rs:33)
  if (!d.err && d.bpos > d.limb) d.err = RC_F_TRUNCATED;
#ifdef RC_WIDE_STATS
  atomicAdd(&g_wide_stats[0], (unsigned long long)d.st_steps);
  atomicAdd(&g_wide_stats[1], (unsigned long long)d.st_fix);
#endif
  flags[k] = d.err;
}

// ------------------------------------------------------------------------------------------
// Host: the plan and the launchers
// ------------------------------------------------------------------------------------------
static u32 wide_bitlen(u32 v) { return v ? 32u - (u32)__builtin_clz(v) : 0u; }

void rc_wide_plan(u32 n, u32 total, WidePlan* p) {
  memset(p, 0, sizeof *p);
  if (n < 1 || n > RC_MAX_WIDE_SYMBOLS || total < 256 || total > 65536) return;
  // encoder (as rc_set_plan): as many lanes as fit beside the table (the register allocation
  // allows 1,024 per CU); at equal lanes the 8-B entries, which cost the symbol step less
  for (u32 lanes = 1024; lanes >= 256 && !p->enc_lanes; lanes -= 256) {
    const u32 rings = lanes * SET_ENC_LANE_BYTES;
    const u32 t8 = ((n + 1) * 8u + 1023u) & ~1023u;
    const u32 t4 = ((n + 2) * 4u + 1023u) & ~1023u;
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
  // decoder: the cum-only row cum[0 .. n] and 2^bits 4-B buckets beside the rings; bits is capped
  // by 2^12 (the single-table decoders' finest) and by the total.  The first of 1,024, 768 and
  // 512 lanes that leaves the cap's buckets room (1,024 at every accepted n: 16 KiB + 16 KiB +
  // 72 KiB at most), else the one that leaves the most.
  const u32 bl = wide_bitlen(total - 1);
  const u32 cap = bl < 12u ? bl : 12u;
  auto bits_at = [&](u32 lanes) -> int {
    const u32 fixed = (n + 1) * 4u + lanes * SET_DEC_LANE_BYTES;
    int b = -1;
    for (u32 t = 0; t <= cap; ++t)
      if (fixed + (4u << t) <= SET_LDS_BYTES) b = (int)t;
    return b;
  };
  u32 best_lanes = 0;
  int best = -1;
  for (u32 lanes = 1024; lanes >= 512; lanes -= 256) {
    const int b = bits_at(lanes);
    if (b >= (int)cap) {
      best_lanes = lanes;
      best = b;
      break;
    }
    if (b > best) {
      best_lanes = lanes;
      best = b;
    }
  }
  p->dec_lanes = best_lanes;
  p->dec_bits = (u32)best;
  p->dec_shift = bl > p->dec_bits ? bl - p->dec_bits : 0u;
  p->dec_lds = (n + 1) * 4u + (4u << p->dec_bits) + best_lanes * SET_DEC_LANE_BYTES;
}

hipError_t rc_wide_encode_launch(hipStream_t stream, const RcKnobs& k, const WideArgs& a_in,
                                 int div, const WidePlan& p, const uint16_t* syms,
                                 const u64* sym_off, u32 n_chunks, uint8_t* out,
                                 const u64* out_off, u64* out_len, u32* flags) {
  WideArgs a = a_in;
  a.tab_bytes = p.enc_tab;
  hipError_t lds_err = hipSuccess;
  const u32 lanes = set_launch_lanes(p.enc_lanes, n_chunks);
  const u32 lds = p.enc_tab + lanes * SET_ENC_LANE_BYTES;
  const dim3 grid((n_chunks + lanes - 1) / lanes), block(lanes);
  auto go = [&](auto kern) {
    if ((lds_err = set_allow_lds(reinterpret_cast<const void*>(kern))) != hipSuccess) return;
    rc_prio_policy(a.m, kPrioEncoder, grid.x,
                   rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)lanes, lds), k);
    hipLaunchKernelGGL(kern, grid, block, lds, stream, a, syms, sym_off, n_chunks, out, out_off,
                       out_len, flags);
  };
  if (div == DIV_POW2) {
    if (p.enc_layout == 0) go(k_encode_wide<DIV_POW2, 0>);
    else go(k_encode_wide<DIV_POW2, 1>);
  } else {
    if (p.enc_layout == 0) go(k_encode_wide<DIV_MAGIC, 0>);
    else go(k_encode_wide<DIV_MAGIC, 1>);
  }
  return lds_err != hipSuccess ? lds_err : hipGetLastError();
}

hipError_t rc_wide_decode_launch(hipStream_t stream, const RcKnobs& k, const WideArgs& a_in,
                                 int div, const WidePlan& p, const uint8_t* code,
                                 const u64* code_off, const u64* code_len, uint16_t* syms_out,
                                 const u64* sym_off, u32 n_chunks, u32* flags) {
  WideArgs a = a_in;
  hipError_t lds_err = hipSuccess;
  const u32 lanes = set_launch_lanes(p.dec_lanes, n_chunks);
  const u32 lds = p.dec_lds - (p.dec_lanes - lanes) * SET_DEC_LANE_BYTES;
  const dim3 grid((n_chunks + lanes - 1) / lanes), block(lanes);
  auto go = [&](auto kern) {
    if ((lds_err = set_allow_lds(reinterpret_cast<const void*>(kern))) != hipSuccess) return;
    rc_prio_policy(a.m, kPrioDecoder512, grid.x,
                   rc_resident_wgs(reinterpret_cast<const void*>(kern), (int)lanes, lds), k);
    hipLaunchKernelGGL(kern, grid, block, lds, stream, a, code, code_off, code_len, syms_out,
                       sym_off, n_chunks, flags);
  };
  if (div == DIV_POW2) go(k_decode_wide<DIV_POW2>);
  else go(k_decode_wide<DIV_MAGIC>);
  return lds_err != hipSuccess ? lds_err : hipGetLastError();
}
