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
#include "rc_cuwg.inc"

// dummy symbol tile of dead lanes (zeros: symbol 0 is in every alphabet)
__device__ uint4 g_wsink[4];

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// the (cum, c) entry of symbol s (cuwg_enc_entry of the one table at LDS address 0).  A symbol
// >= n reads entry n: the poison entry (layout 0), or cum[n] = cum[n + 1] = total, so c = 0
// (layout 1).
template <int LAYOUT>
static __device__ __forceinline__ uint2 wide_entry(u32 n, u32 s) {
  return cuwg_enc_entry<LAYOUT>(0u, min(s, n));
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

  const uint16_t* sp = syms + ch.s0;
  // (n <= 2^25 here: the symbol counters are 32-bit, which keeps the tile registers free)
  const u32 nn = (u32)ch.n;
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
  const u32 tmin = cuwg_tmin(live, ntile);
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

  const u32 len = cuwg_enc_finish(e, &l.out[tid], ch.al, lane, wring, wout, wrank);
  if (live)
    cuwg_enc_report(ch, k, len, (e.err >> 24) ? wide_first_error(a.row, m.n, sp, ch.n) : 0u,
                    out_len, flags);
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

// Decoder::decode(&table) with FreqTable::find_index: the hint q from the carried scale G, q's
// bucket (the buckets are at LDS address 0), which names the symbols [s_lo, s_hi] that find_index
// returns for the bucket's frequencies, a binary search for the last symbol of that range whose
// cum is <= q (strides from a.top_stride down, the count that settles the table's widest bucket,
// so the loop is wave-uniform and scalar; a settled lane probes on without moving), the
// candidate's (cum, c), the exact u64 verification r cum <= x < r (cum + c), and the exact walk
// (cuwg_dec_fix) when a lane's candidate fails it.  Every probe stays inside [s_lo, s_hi],
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
  uint2 t = cuwg_cum_entry(rowa, s);
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
      cuwg_dec_fix<false>(s, t, A, B, d.x(), r, rowa, m.n);
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
#ifdef RC_WIDE_STATS
  atomicAdd(&g_wide_stats[0], (unsigned long long)d.st_steps);
  atomicAdd(&g_wide_stats[1], (unsigned long long)d.st_fix);
#endif
  flags[k] = cuwg_dec_flag(d);
}

// ------------------------------------------------------------------------------------------
// Host: the plan and the launchers
// ------------------------------------------------------------------------------------------
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
  cuwg_dec_plan(p, total, (n + 1) * 4u, 1u, 12u);
}

hipError_t rc_wide_encode_launch(hipStream_t stream, const RcKnobs& k, const WideArgs& a_in,
                                 int div, const WidePlan& p, const uint16_t* syms,
                                 const u64* sym_off, u32 n_chunks, uint8_t* out,
                                 const u64* out_off, u64* out_len, u32* flags) {
  WideArgs a = a_in;
  a.tab_bytes = p.enc_tab;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioEncoder, p.enc_lanes, SET_ENC_LANE_BYTES,
                       p.enc_lds, n_chunks, syms, sym_off, n_chunks, out, out_off, out_len, flags);
  };
  if (div == DIV_POW2)
    return p.enc_layout == 0 ? go(k_encode_wide<DIV_POW2, 0>) : go(k_encode_wide<DIV_POW2, 1>);
  return p.enc_layout == 0 ? go(k_encode_wide<DIV_MAGIC, 0>) : go(k_encode_wide<DIV_MAGIC, 1>);
}

hipError_t rc_wide_decode_launch(hipStream_t stream, const RcKnobs& k, const WideArgs& a_in,
                                 int div, const WidePlan& p, const uint8_t* code,
                                 const u64* code_off, const u64* code_len, uint16_t* syms_out,
                                 const u64* sym_off, u32 n_chunks, u32* flags) {
  WideArgs a = a_in;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioDecoder512, p.dec_lanes, SET_DEC_LANE_BYTES,
                       p.dec_lds, n_chunks, code, code_off, code_len, syms_out, sym_off, n_chunks,
                       flags);
  };
  return div == DIV_POW2 ? go(k_decode_wide<DIV_POW2>) : go(k_decode_wide<DIV_MAGIC>);
}
