// rc_wide16.hip — k_encode_wide16 / k_decode_wide16: the small-model static coders over one table
// of up to RC_MAX_WIDE16_SYMBOLS (2^16) 16-bit symbols whose tables stay in device memory
// (wide16 static models, rc_wide16.h).  Symbol i of a chunk is coded exactly as
// encoder.encode(&table, sym[i]) / decoder.decode(&table).  The arithmetic, the encoder's
// accumulator, ring and ranked flush rounds and the decoder's code ring, dec_apply and dec_rare
// are those of the single-table coders (rc_encode.inc, rc_decode.inc, rc_static.h), the loops
// around them those of the wide coders (rc_wide.hip).  What is new: a symbol's entry comes from
// global memory (the L2), so the encoder issues the entry loads of 8 symbols together and a block
// ahead of their use, the decoder reads a q-to-symbol halfword (staged in LDS) and then the
// candidate's cum pair, and the fix-up after a missed hint walks in q space, from one occupied symbol to the next.
#define RC_DEC_SHARED_ONLY
#include "rc_wide16.h"

#include "rc_encode.inc"
#include "rc_decode.inc"
#include "rc_cuwg.inc"

// dummy symbol tile of dead lanes (zeros: symbol 0 is in every alphabet)
__device__ uint4 g_w16sink[4];

// Blocks of 8 symbols the encoder's entry loads run ahead of the symbol steps (1: the loads of
// block b + 1 are issued before block b is coded; 0: a block's loads are issued together, then
// the block is coded).  DESIGN.md §9.21 has the two measured.
#ifndef RC_W16_ENC_AHEAD
#define RC_W16_ENC_AHEAD 1
#endif

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// the 8 (cum | flag << 24, c) entries of the 8 symbols of one 16-B block, all loads issued
// together.  A symbol >= n reads the poison entry n (a.enc_clamp; at n = 2^16 there is none and
// no 16-bit value needs one).
struct W16Ent8 {
  uint2 t[8];
};
static __device__ __forceinline__ void wide16_load8(W16Ent8& E, const Wide16Args& a, uint4 v) {
  const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    E.t[2 * p] = a.enc[min(w[p] & 0xFFFFu, a.enc_clamp)];
    E.t[2 * p + 1] = a.enc[min(w[p] >> 16, a.enc_clamp)];
  }
}

// 8 symbols from their entries, as wide_enc8: pairs share one rare test, a flush check after the
// 8 symbols
template <int DIV>
static __device__ __forceinline__ void wide16_enc8(Enc& e, const ModelArgs& m, const W16Ent8& E,
                                                   bool act, u32 lane, const u32* wring,
                                                   const EncOut* wout, u32* wrank) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
    enc_sym2<DIV, 1>(e, m, E.t[2 * p], E.t[2 * p + 1], act, lane, wring, wout, wrank);
  enc_flush(e, lane, wring, wout, wrank);
}

// one symbol fetched on its own (unaligned head / tail of a chunk)
template <int DIV>
static __device__ __forceinline__ void wide16_enc_one(Enc& e, const Wide16Args& a,
                                                      const uint16_t* sp, u32 i, bool act,
                                                      u32 lane, const u32* wring,
                                                      const EncOut* wout, u32* wrank) {
  const u32 sym = act ? (u32)sp[i] : 0u;
  enc_sym<DIV, 1>(e, a.m, a.enc[min(sym, a.enc_clamp)], act, lane, wring, wout, wrank);
}

// the first symbol of a chunk the reference cannot encode (rare: flagged chunks only)
// (scalars, not the argument struct by reference: an out-of-line call would copy it to scratch)
static __device__ u32 wide16_first_error(const u32* row, u32 n_symbols, const uint16_t* sp,
                                         u64 n) {
  for (u64 i = 0; i < n; ++i) {
    const u32 s = sp[i];
    if (s >= n_symbols) return RC_F_BAD_SYMBOL;
    if (row[s + 1] == row[s]) return RC_F_ZERO_FREQ;
  }
  return 0;
}

template <int DIV>
__global__ __launch_bounds__(1024) void k_encode_wide16(
    Wide16Args a, const uint16_t* __restrict__ syms, const u64* __restrict__ sym_off,
    u32 n_chunks, uint8_t* __restrict__ out, const u64* __restrict__ out_off,
    u64* __restrict__ out_len, u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS: 8 KiB of rings per wave at address 0, the lanes' output geometry and the waves'
  // rank tables; no table
  extern __shared__ __attribute__((aligned(1024))) u32 s_enc[];
  const u32 tid = threadIdx.x, lanes = blockDim.x;
  const ModelArgs& m = a.m;
  const CuwgEncLds l = cuwg_enc_lds(s_enc, 0u, lanes);
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
  cuwg_enc_init(e, ch.al, 0u, wave, lane);

  const uint16_t* sp = syms + ch.s0;
  // (n <= 2^25 here: the symbol counters are 32-bit, which keeps the tile registers free)
  const u32 nn = (u32)ch.n;
  // symbols before the first 64-B aligned tile (the stream is 2-B aligned)
  u32 head = ((64 - ((u32)(uintptr_t)sp & 63)) & 63) >> 1;
  if (head > nn) head = nn;
  const u32 ntile = (nn - head) >> 5;  // 64-B tiles of 32 symbols
  // head: symbol-wise, all lanes in step (flush rounds are wave-wide)
  for (u32 i = 0; __any((int)(i < head)); ++i) {
    wide16_enc_one<DIV>(e, a, sp, i, i < head, lane, wring, wout, wrank);
    if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }
  // body, part 1: the tiles every live lane of the wave has, with every lane active; dead lanes
  // run along on a dummy tile and a slot with no writable bytes
  const u32 tmin = cuwg_tmin(live, ntile);
  const uint8_t* tp = live ? reinterpret_cast<const uint8_t*>(sp + head)
                           : reinterpret_cast<const uint8_t*>(g_w16sink);
  // 32-symbol tiles, 4 x 16 B per lane, the next tile in flight while the current one is coded
  // (explicit registers, as in k_encode_wide); the entries of the next 8-symbol block in flight
  // while the current block is coded (the last tile's look-ahead loads its own first block again)
  const u32 tstep = live ? 64 : 0;  // bytes per tile
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
  W16Ent8 E, F;
  if (tmin) {
    const uint4* q = reinterpret_cast<const uint4*>(tp);
    c0 = q[0];
    c1 = q[1];
    c2 = q[2];
    c3 = q[3];
#if RC_W16_ENC_AHEAD
    wide16_load8(E, a, c0);
#endif
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
#if RC_W16_ENC_AHEAD
    wide16_load8(F, a, c1);
    wide16_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16_load8(E, a, c2);
    wide16_enc8<DIV>(e, m, F, true, lane, wring, wout, wrank);
    wide16_load8(F, a, c3);
    wide16_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16_load8(E, a, n0);
    wide16_enc8<DIV>(e, m, F, true, lane, wring, wout, wrank);
#else
    wide16_load8(E, a, c0);
    wide16_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16_load8(F, a, c1);
    wide16_enc8<DIV>(e, m, F, true, lane, wring, wout, wrank);
    wide16_load8(E, a, c2);
    wide16_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16_load8(F, a, c3);
    wide16_enc8<DIV>(e, m, F, true, lane, wring, wout, wrank);
#endif
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
  }
  // body, part 2 (ragged waves): the remaining 8-symbol blocks of the tiles, lanes masked (an
  // idle lane loads the entries of symbol 0)
  const u32 nblk = ntile * 4;
  for (u32 b = tmin * 4; __any((int)(b < nblk)); ++b) {
    const bool act = b < nblk;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (act) v = reinterpret_cast<const uint4*>(tp)[b];
    wide16_load8(E, a, v);
    wide16_enc8<DIV>(e, m, E, act, lane, wring, wout, wrank);
  }
  const u32 tail0 = head + (ntile << 5);
  for (u32 j = 0; __any((int)(tail0 + j < nn)); ++j) {  // j is wave-uniform
    wide16_enc_one<DIV>(e, a, sp, tail0 + j, tail0 + j < nn, lane, wring, wout, wrank);
    if ((j & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }

  const u32 len = cuwg_enc_finish(e, &l.out[tid], ch.al, lane, wring, wout, wrank);
  if (live)
    cuwg_enc_report(ch, k, len, (e.err >> 24) ? wide16_first_error(a.row, m.n, sp, ch.n) : 0u,
                    out_len, flags);
}

// ------------------------------------------------------------------------------------------
// Decoder
// ------------------------------------------------------------------------------------------
#ifdef RC_WIDE16_STATS
// Scratch builds only (-DRC_WIDE16_STATS, tools/kbench_wide16.py; not part of the C ABI): how
// often the decoder's wave takes the fix-up branch.  g_wide16_stats[0] counts lane-symbols, [1]
// the lane-symbols on which the lane's wave took the branch.
__device__ unsigned long long g_wide16_stats[2];
extern "C" int rc_wide16_stats_read_(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide16_stats), sizeof g_wide16_stats) != hipSuccess)
    return -1;
  const unsigned long long zero[2] = {0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_wide16_stats), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
struct Wide16Dec : Dec<DEC_LD, 0> {
  u32 st_steps, st_fix;
};
#else
typedef Dec<DEC_LD, 0> Wide16Dec;
#endif

// The q-to-symbol table is staged in LDS at address 0 in front of the rings (RC_W16_SYMOF_LDS,
// rc_wide16.h): one of the step's two dependent L2 reads becomes an LDS read, at the price of
// lanes (rc_wide16_plan).  -DRC_W16_SYMOF_LDS=0 is the form that reads it from device memory with
// 1,024 lanes per workgroup, measured against this one in DESIGN.md §9.21.
static __device__ __forceinline__ u32 wide16_symof(const Wide16Args& a, u32 q) {
#if RC_W16_SYMOF_LDS
  typedef __attribute__((address_space(3))) uint16_t l_u16;
  return *(const l_u16*)(uintptr_t)(q << 1);
#else
  return a.symof[q];
#endif
}

// (cum, c) of symbol s from the cum-only row in device memory: c = cum[s + 1] - cum[s] (the row
// holds the total from its alphabet's end on)
static __device__ __forceinline__ uint2 wide16_cum_entry(const u32* row, u32 s) {
  const u32 c0 = row[s], c1 = row[s + 1];
  return make_uint2(c0, c1 - c0);
}

// The exact index after a candidate that failed the verification: FreqTable::find_index's
// s = #{ j in [1, n-1] : r * cum[j] <= x }, the result of cuwg_dec_fix's walk, reached through
// the q-to-symbol table so that a step goes from one symbol with c > 0 to the next one and never
// reads the zero-frequency symbols between them: down to symof[cum[s] - 1] (A > x means
// cum[s] > 0), up to symof[cum[s] + c[s]], or to n - 1 once that reaches the total, where the
// walk ends whatever it finds (c = 0 there only on corrupt input: the caller flags it).
static __device__ __forceinline__ void wide16_dec_fix(u32& s, uint2& t, u64& A, u64& B, u64 x,
                                                      u64 r, const Wide16Args& a) {
  if (A > x) {
    do {
      s = wide16_symof(a, t.x - 1u);
      t = wide16_cum_entry(a.row, s);
      A = r * (u64)t.x;
    } while (A > x);
    B = r * (u64)t.y;
  } else {
    while (x - A >= B) {
      const u32 q = t.x + t.y;
      const bool end = q >= a.m.total;
      s = a.m.n - 1u;
      if (!end) s = wide16_symof(a, q);
      t = wide16_cum_entry(a.row, s);
      A = r * (u64)t.x;
      B = r * (u64)t.y;
      if (end) break;
    }
  }
}

// Decoder::decode(&table) with FreqTable::find_index: the hint q from the carried scale G, the
// q-to-symbol halfword (masked index: the table is padded to a power of two), the candidate's
// (cum, c) from the cum row, the exact u64 verification r cum <= x < r (cum + c), and the walk in
// q space (wide16_dec_fix) when a lane's candidate fails it.
template <int DIV>
static __device__ __forceinline__ u32 wide16_dec_sym(Wide16Dec& d, const Wide16Args& a) {
  const ModelArgs& m = a.m;
  u32 roff, raddr;
  asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
  asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(raddr) : "v"(roff), "v"((u32)(uintptr_t)d.ring));
  const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
  const u32 D0 = rp[0], D1 = rp[Wide16Dec::kS];
  const u64 r = range_par_total<DIV, 1>(d.range, m);
  const float X = (float)(d.dhi() - hi32(d.low));
  const u32 qh = hint_floor(X, d.G);
  u32 s = wide16_symof(a, qh & a.qmask);
  uint2 t = wide16_cum_entry(a.row, s);
  float tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));  // (hint only)
  u64 B = mul_rv<1>(r, t.y);
  u64 A = mul_rv<1>(r, t.x);
  const u64 dx = sub64((u32)d.dat, d.dhi(), d.low + A);  // x - r cum
#ifdef RC_WIDE16_STATS
  d.st_steps += 1;
#endif
  if (__builtin_expect(__any((int)(dx >= B)), 0)) {
#ifdef RC_WIDE16_STATS
    d.st_fix += 1;
#endif
    if (dx >= B) {
      wide16_dec_fix(s, t, A, B, d.x(), r, a);
      tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));
      // the table only names symbols with c > 0, so c == 0 can only come from the walk's end at
      // n - 1: corrupt input (the reference loops forever); an over-read, if any, came first
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
static __device__ __forceinline__ uint4 wide16_block8(Wide16Dec& d, const Wide16Args& a) {
  u32 w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32 s0 = wide16_dec_sym<DIV>(d, a);
    const u32 s1 = wide16_dec_sym<DIV>(d, a);
    w[q] = s0 | (s1 << 16);
    if (q == 1 && DEC_CHECK_SPAN == 4) dec_check4<1, DEC_NEED_SPAN>(d);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DIV>
__global__ __launch_bounds__(1024) void k_decode_wide16(
    Wide16Args a, const uint8_t* __restrict__ code, const u64* __restrict__ code_off,
    const u64* __restrict__ code_len, uint16_t* __restrict__ syms_out,
    const u64* __restrict__ sym_off, u32 n_chunks, u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS: the q-to-symbol table at address 0 (a read of it needs no base add), then the
  // code rings
  const u32 tid = threadIdx.x, lanes = blockDim.x;
  const ModelArgs& m = a.m;
#if RC_W16_SYMOF_LDS
  extern __shared__ u32 s_dyn[];
  const u32 ring0 = 2u * (a.qmask + 1u);  // (a multiple of 512 B: total >= 256)
  for (u32 j = tid; j < ring0 / 4u; j += lanes)
    s_dyn[j] = reinterpret_cast<const u32*>(a.symof)[j];
  __syncthreads();
#else
  const u32 ring0 = 0u;
#endif
  const u32 k = blockIdx.x * lanes + tid;
  if (k >= n_chunks) return;
  // f32 rounding toward zero from here on (MODE.FP_ROUND f32 bits = 3), for hint_floor
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3");
  RC_VGPR_FLOOR_128();
  const u32 lane = tid & 63, wave = tid >> 6;

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

  Wide16Dec d;
#ifdef RC_WIDE16_STATS
  d.st_steps = d.st_fix = 0;
#endif
  d.low = 0;
  d.range = ~0ull;
  d.err = 0;
  d.fillb = 0;
  d.pend_ok = 0;
  d.ring = (l_u32*)(uintptr_t)ring0 + wave * DEC_RING_ALLOC * 64 + lane;
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
    op[i] = (uint16_t)wide16_dec_sym<DIV>(d, a);
    dec_check4<1>(d);
  }
  dec_check4<1, DEC_NEED_SPAN>(d);
  // body: 16-symbol phases of two 16-B blocks, written in 64-B bursts of two phases
  uint4* ob = reinterpret_cast<uint4*>(op + i);
  const u32 nfull = (n - i) >> 4;  // whole phases (bursts of two, then a single one)
#define RC_WIDE16_PHASE(oa, ob_)                  \
  dec_gexact<1, 4>(d, m);                         \
  const uint4 oa = wide16_block8<DIV>(d, a);      \
  dec_check4<1, DEC_NEED_SPAN>(d);                \
  const uint4 ob_ = wide16_block8<DIV>(d, a);     \
  dec_phase(d);                                   \
  dec_check4<1, DEC_NEED_SPAN>(d);
  for (u32 b = 0; b < nfull / 2; ++b) {
    rc_prio_rotate(m.prio_rot);
    RC_WIDE16_PHASE(o0, o1) RC_WIDE16_PHASE(o2, o3)
    uint4* ob_b = ob + 4 * b;
    ob_b[0] = o0;
    ob_b[1] = o1;
    ob_b[2] = o2;
    ob_b[3] = o3;
  }
  if (nfull & 1) {
    RC_WIDE16_PHASE(o0, o1)
    uint4* ob_b = ob + 2 * (nfull - 1);
    ob_b[0] = o0;
    ob_b[1] = o1;
  }
#undef RC_WIDE16_PHASE
  i += nfull << 4;
  for (; i < n; ++i) {
    op[i] = (uint16_t)wide16_dec_sym<DIV>(d, a);
    dec_check4<1>(d);
  }
#ifdef RC_WIDE16_STATS
  atomicAdd(&g_wide16_stats[0], (unsigned long long)d.st_steps);
  atomicAdd(&g_wide16_stats[1], (unsigned long long)d.st_fix);
#endif
  flags[k] = cuwg_dec_flag(d);
}

// ------------------------------------------------------------------------------------------
// Host: the plan and the launchers
// ------------------------------------------------------------------------------------------
void rc_wide16_plan(u32 n, u32 total, Wide16Plan* p) {
  memset(p, 0, sizeof *p);
  if (n < 1 || n > RC_MAX_WIDE16_SYMBOLS || total < 256 || total > 65536) return;
  // encoder: no table in LDS, the rings of all the lanes a CU holds at 128 VGPRs, whatever the
  // alphabet
  p->enc_lanes = 1024;
  p->enc_lds = 1024 * SET_ENC_LANE_BYTES;
  p->enc_layout = 0;
  p->enc_tab = 8u * (n + (n < 65536u ? 1u : 0u));
  p->dec_bits = bitlen(total - 1);
  p->dec_shift = 0;
#if RC_W16_SYMOF_LDS
  // decoder: the 2-B q-to-symbol entries beside the rings, whole pairs of waves per SIMD: 1,024
  // lanes up to a total of 2^15 (64 KiB of table), 384 beside the 128 KiB above it
  const u32 symof = 2u << p->dec_bits;
  const u32 fit = (SET_LDS_BYTES - symof) / SET_DEC_LANE_BYTES & ~127u;
  p->dec_lanes = fit < 1024u ? fit : 1024u;
  p->dec_lds = symof + p->dec_lanes * SET_DEC_LANE_BYTES;
#else
  p->dec_lanes = 1024;
  p->dec_lds = 1024 * SET_DEC_LANE_BYTES;
#endif
}

static u32 g_w16_last_lanes[2];
extern "C" void rc_wide16_last_lanes_(uint32_t* out2) {
  out2[0] = g_w16_last_lanes[0];
  out2[1] = g_w16_last_lanes[1];
}

hipError_t rc_wide16_encode_launch(hipStream_t stream, const RcKnobs& k, const Wide16Args& a_in,
                                   int div, const Wide16Plan& p, const uint16_t* syms,
                                   const u64* sym_off, u32 n_chunks, uint8_t* out,
                                   const u64* out_off, u64* out_len, u32* flags) {
  Wide16Args a = a_in;
  g_w16_last_lanes[0] = set_launch_lanes(p.enc_lanes, n_chunks);
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioEncoder, p.enc_lanes, SET_ENC_LANE_BYTES,
                       p.enc_lds, n_chunks, syms, sym_off, n_chunks, out, out_off, out_len, flags);
  };
  return div == DIV_POW2 ? go(k_encode_wide16<DIV_POW2>) : go(k_encode_wide16<DIV_MAGIC>);
}

hipError_t rc_wide16_decode_launch(hipStream_t stream, const RcKnobs& k, const Wide16Args& a_in,
                                   int div, const Wide16Plan& p, const uint8_t* code,
                                   const u64* code_off, const u64* code_len, uint16_t* syms_out,
                                   const u64* sym_off, u32 n_chunks, u32* flags) {
  Wide16Args a = a_in;
  const u32 plan_lanes = p.dec_lanes, plan_lds = p.dec_lds;
  g_w16_last_lanes[1] = set_launch_lanes(plan_lanes, n_chunks);
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioDecoder512, plan_lanes, SET_DEC_LANE_BYTES,
                       plan_lds, n_chunks, code, code_off, code_len, syms_out, sym_off, n_chunks,
                       flags);
  };
  return div == DIV_POW2 ? go(k_decode_wide16<DIV_POW2>) : go(k_decode_wide16<DIV_MAGIC>);
}
