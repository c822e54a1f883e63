// rc_wide16_fine.hip — k_encode_wide16_fine / k_decode_wide16_fine: the wide16 batch coders for a
// wide16 fine model (rc_wide16_fine.h): one table of up to 2^16 16-bit symbols whose total lies
// in (2^16, 2^24].  Symbol i of a chunk is coded exactly as encoder.encode(&table, sym[i]) /
// decoder.decode(&table).  The arithmetic is the SM = 0 regime of the single-table coders
// (rc_encode.inc, rc_decode.inc: enc_core's (cum, c) entries, the 64-bit ffbh, three ring words
// per decoder step, DEC_NEED_WIDE), the loops around it are those of k_encode_wide16 /
// k_decode_wide16.  The loops are restated here, not shared through a header: the wide16 kernels
// interleave their SM = 1 ring checks and the carried hint scale with the loop bodies, and a
// shared scaffold taking those as parameters would have to leave their code unchanged to the
// instruction (tools/kernel_diff.py), which two files do by construction.
// What is new: the decoder finds a symbol through a bucket table over the top bits of q (in LDS),
// a short search over the occupied symbols' cum row (in the L2) where the bucket names more than
// one rank, and a fix-up that steps in rank space.
#define RC_DEC_SHARED_ONLY
#include "rc_wide16_fine.h"

#include "rc_encode.inc"
#include "rc_decode.inc"
#include "rc_cuwg.inc"

// dummy symbol tile of dead lanes (zeros: symbol 0 is in every alphabet)
__device__ uint4 g_w16fsink[4];

// Bytes one symbol can settle at a total of at most 2^24: the range is at least
// 2^48 when a symbol starts, so range / total >= 2^24 and the symbol's range r c >= 2^24;
// no_carry_expansion settles k bytes only while r c < 2^(64 - 8k), so k <= 4, and
// range_reduction_expansion at most 7 more.
#define W16F_NOCARRY_BYTES 4u
#define W16F_REDUCE_BYTES 7u
// Encoder ring: a flush check comes after every rare path (enc_sym) and after at most 8 symbols:
// inside the head and the tail at every eighth symbol, after the head loop (a head of up to 31
// symbols ends up to 7 symbols past its last check, and the body's first check comes 8 symbols
// later: without this one 15 symbols of 3 bytes would pass between two checks, 45 bytes, which
// the 16-bit symbols of k_encode_wide16 never reach and these do), and after every 8-symbol block
// of the body.  A symbol off the rare path settles at most 3 bytes (enc_core: z <= 31), so
// between two checks a lane adds at most 8 x 3 bytes, or 7 x 3 and one rare symbol's 4 + 7; the
// tail leaves at most 7 x 3 bytes unchecked in front of Encoder::finish's 8.
static_assert(FLUSH_AT - 1 + 7 * 3 + (W16F_NOCARRY_BYTES + W16F_REDUCE_BYTES) <= 4 * ENC_RING - 1 &&
                  FLUSH_AT - 1 + 8 * 3 <= 4 * ENC_RING - 1 &&
                  FLUSH_AT - 1 + 7 * 3 + 8 <= 4 * ENC_RING - 1,
              "fine encoder may overrun its output ring");
// Decoder ring: DEC_NEED_WIDE bytes are staged before every symbol (the rare test after each
// symbol), which covers the 4 bytes of dec_apply; a reduction of m <= 7 bytes stages m +
// DEC_NEED_WIDE before it reads its own.
static_assert(DEC_NEED_WIDE >= W16F_NOCARRY_BYTES && DEC_NEED_HEAD >= DEC_NEED_WIDE,
              "fine decoder's symbol may read past the staged bytes");
static_assert(W16F_REDUCE_BYTES + DEC_NEED_WIDE <= 4u * DEC_RING - 32u + 1u,
              "rare-path ring need exceeds what a refill may stage");
static_assert(DEC_MIRROR >= 2, "three ring words are read from any ring position");

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// the 8 (cum, c) entries of the 8 symbols of one 16-B block, all loads issued together.  A symbol
// >= n reads the poison entry n (a.enc_clamp; at n = 2^16 there is none and no 16-bit value needs
// one).
struct W16FEnt8 {
  uint2 t[8];
};
static __device__ __forceinline__ void wide16f_load8(W16FEnt8& E, const Wide16FineArgs& a,
                                                     uint4 v) {
  const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    E.t[2 * p] = a.enc[min(w[p] & 0xFFFFu, a.enc_clamp)];
    E.t[2 * p + 1] = a.enc[min(w[p] >> 16, a.enc_clamp)];
  }
}

// 8 symbols from their entries, one rare test per symbol (enc_sym2's pairing is the small
// models'), a flush check after the 8 symbols
template <int DIV>
static __device__ __forceinline__ void wide16f_enc8(Enc& e, const ModelArgs& m, const W16FEnt8& E,
                                                    bool act, u32 lane, const u32* wring,
                                                    const EncOut* wout, u32* wrank) {
#pragma unroll
  for (int p = 0; p < 8; ++p) enc_sym<DIV, 0>(e, m, E.t[p], act, lane, wring, wout, wrank);
  enc_flush(e, lane, wring, wout, wrank);
}

// one symbol fetched on its own (unaligned head / tail of a chunk)
template <int DIV>
static __device__ __forceinline__ void wide16f_enc_one(Enc& e, const Wide16FineArgs& a,
                                                       const uint16_t* sp, u32 i, bool act,
                                                       u32 lane, const u32* wring,
                                                       const EncOut* wout, u32* wrank) {
  const u32 sym = act ? (u32)sp[i] : 0u;
  enc_sym<DIV, 0>(e, a.m, a.enc[min(sym, a.enc_clamp)], act, lane, wring, wout, wrank);
}

// the first symbol of a chunk the reference cannot encode (rare: flagged chunks only)
static __device__ u32 wide16f_first_error(const uint2* enc, u32 n_symbols, const uint16_t* sp,
                                          u64 n) {
  for (u64 i = 0; i < n; ++i) {
    const u32 s = sp[i];
    if (s >= n_symbols) return RC_F_BAD_SYMBOL;
    if (enc[s].y == 0) return RC_F_ZERO_FREQ;
  }
  return 0;
}

template <int DIV>
__global__ __launch_bounds__(1024) void k_encode_wide16_fine(
    Wide16FineArgs a, const uint16_t* __restrict__ syms, const u64* __restrict__ sym_off,
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
    wide16f_enc_one<DIV>(e, a, sp, i, i < head, lane, wring, wout, wrank);
    if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }
  // (the head's last symbols: the next check is 8 symbols away, see the ring's margin above)
  enc_flush(e, lane, wring, wout, wrank);
  // body, part 1: the tiles every live lane of the wave has, with every lane active; dead lanes
  // run along on a dummy tile and a slot with no writable bytes
  const u32 tmin = cuwg_tmin(live, ntile);
  const uint8_t* tp = live ? reinterpret_cast<const uint8_t*>(sp + head)
                           : reinterpret_cast<const uint8_t*>(g_w16fsink);
  // 32-symbol tiles, 4 x 16 B per lane, the next tile in flight while the current one is coded.
  // A block's 8 entry loads are issued together and the block is coded behind them: the wide16
  // encoder's second entry block, loaded a block ahead, does not fit beside the 64-bit products
  // of this regime (80 B of scratch per lane at 128 VGPRs; half a block ahead, two sets of 4
  // entries in the same 16 registers, still 96 and 32 B), and a step here is long enough to cover
  // more of the L2's latency within a block.
  const u32 tstep = live ? 64 : 0;  // bytes per tile
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
  W16FEnt8 E;
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
    wide16f_load8(E, a, c0);
    wide16f_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16f_load8(E, a, c1);
    wide16f_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16f_load8(E, a, c2);
    wide16f_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
    wide16f_load8(E, a, c3);
    wide16f_enc8<DIV>(e, m, E, true, lane, wring, wout, wrank);
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
    wide16f_load8(E, a, v);
    wide16f_enc8<DIV>(e, m, E, act, lane, wring, wout, wrank);
  }
  const u32 tail0 = head + (ntile << 5);
  for (u32 j = 0; __any((int)(tail0 + j < nn)); ++j) {  // j is wave-uniform
    wide16f_enc_one<DIV>(e, a, sp, tail0 + j, tail0 + j < nn, lane, wring, wout, wrank);
    if ((j & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }

  const u32 len = cuwg_enc_finish(e, &l.out[tid], ch.al, lane, wring, wout, wrank);
  if (live)
    cuwg_enc_report(ch, k, len, e.err ? wide16f_first_error(a.enc, m.n, sp, ch.n) : 0u, out_len,
                    flags);
}

// ------------------------------------------------------------------------------------------
// Decoder
// ------------------------------------------------------------------------------------------
#ifdef RC_WIDE16_FINE_STATS
// Scratch builds only (-DRC_WIDE16_FINE_STATS, tools/kbench_wide16.py; not part of the C ABI):
// how often the decoder's wave takes the search and the fix-up branch.  [0] counts lane-symbols,
// [1] the lane-symbols on which the lane's wave ran the search, [2] those on which it took the
// fix-up branch.
__device__ unsigned long long g_wide16_fine_stats[3];
extern "C" int rc_wide16_fine_stats_read_(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide16_fine_stats), sizeof g_wide16_fine_stats) !=
      hipSuccess)
    return -1;
  const unsigned long long zero[3] = {0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_wide16_fine_stats), zero, sizeof zero) == hipSuccess ? 0
                                                                                            : -1;
}
struct Wide16FineDec : Dec<DEC_LD, 0> {
  u32 st_steps, st_search, st_fix;
};
#else
typedef Dec<DEC_LD, 0> Wide16FineDec;
#endif

// The exact rank after a candidate that failed the verification: FreqTable::find_index's
// s = #{ i in [1, n-1] : r * cum[i] <= x }, reached in rank space, so that a step goes from one
// occupied symbol to the next whatever lies between them: down while r rcum[j] > x (that ends at
// rank 0 at the latest: rcum[0] = 0), up while x - r rcum[j] >= r c[j].  Once rcum[j + 1] reaches
// the total the walk ends at symbol n - 1 whatever it finds: the last rank when that symbol is
// occupied, else (total, 0) (c = 0 there only on corrupt input: the caller flags it).
static __device__ __forceinline__ void wide16f_dec_fix(u32& j, u32& s, uint2& t, u64& A, u64& B,
                                                       u64 x, u64 r, const Wide16FineArgs& a) {
  bool end = false;
  if (A > x) {
    do --j;
    while (r * (u64)a.rcum[j] > x);
  } else {  // x - A >= B: x >= r rcum[j + 1]
    u32 nx = t.x + t.y;
    while (nx < a.m.total && r * (u64)nx <= x) {
      ++j;
      nx = a.rcum[j + 1];
    }
    end = r * (u64)nx <= x;  // (then nx is the total)
  }
  t.x = a.rcum[j];
  t.y = a.rcum[j + 1] - t.x;
  s = a.occ[j];
  if (end && s != a.m.n - 1u) {
    s = a.m.n - 1u;
    t = make_uint2(a.m.total, 0u);
  }
  A = r * (u64)t.x;
  B = r * (u64)t.y;
}

// Decoder::decode(&table) with FreqTable::find_index: the hint q (the SM = 0 form of dec_sym:
// both high halves shifted by clz(range), one reciprocal), clamped to total - 1 (and set to it
// when x >= range, which only corrupt input reaches: x << clz would drop its top bits); the
// bucket's two ranks from LDS; the last rank of them whose rcum is <= q (no step when the bucket
// names one rank); that rank's (rcum, c) and symbol from the L2; the exact u64 verification
// r cum <= x < r (cum + c); the walk in rank space (wide16f_dec_fix) when a lane fails it.
template <int DIV>
static __device__ __forceinline__ u32 wide16f_dec_sym(Wide16FineDec& d, const Wide16FineArgs& a) {
  const ModelArgs& m = a.m;
  u32 roff, raddr;
  asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
  asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(raddr) : "v"(roff), "v"((u32)(uintptr_t)d.ring));
  const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
  const u32 D0 = rp[0], D1 = rp[Wide16FineDec::kS], D2 = rp[2 * Wide16FineDec::kS];
  const u64 r = range_par_total<DIV, 0>(d.range, m);
  const u64 x = d.x();
  const u32 sh = (u32)__builtin_clz(hi32(d.range));  // (range >= 2^48 between symbols)
  const float X = cvt_f32(hi32(x << sh));
  const float R = cvt_f32(hi32(d.range << sh));
  u32 q = min(cvt_u32_sat(X * (m.ftotal * __builtin_amdgcn_rcpf(R))), a.qmax);
  q = x >= d.range ? a.qmax : q;
  // the bucket table is the kernel's first LDS object: 2 (q >> shift) is its byte address
  typedef __attribute__((address_space(3))) uint16_t l_u16;
  const l_u16* bp = (const l_u16*)(uintptr_t)((q >> a.shift) << 1);
  u32 j = bp[0], j1 = bp[1];
#ifdef RC_WIDE16_FINE_STATS
  d.st_steps += 1;
  if (__any((int)(j < j1))) d.st_search += 1;
#endif
  while (j < j1) {
    const u32 mid = (j + j1 + 1u) >> 1;
    if (a.rcum[mid] <= q) j = mid;
    else j1 = mid - 1u;
  }
  const u32 cum0 = a.rcum[j], cum1 = a.rcum[j + 1];
  u32 s = a.occ[j];
  uint2 t = make_uint2(cum0, cum1 - cum0);
  u64 A = r * (u64)t.x;
  u64 B = r * (u64)t.y;
  if (__builtin_expect(__any((int)(x - A >= B)), 0)) {
#ifdef RC_WIDE16_FINE_STATS
    d.st_fix += 1;
#endif
    if (x - A >= B) {
      wide16f_dec_fix(j, s, t, A, B, x, r, a);
      // the ranks only name symbols with c > 0, so c == 0 can only come from the walk's end at
      // n - 1: corrupt input (the reference loops forever); an over-read, if any, came first
      if (t.y == 0) {
        d.err = d.err ? d.err : (d.bpos > d.limb ? RC_F_TRUNCATED : RC_F_CORRUPT);
        B = r;
      }
    }
  }
  dec_apply<0, 0>(d, d.low + A, B, d.dat, 0.0f, D0, D1, D2);
  // rare: range_reduction_expansion, or the ring runs short for the next symbol
  const bool rare = (hi32(d.range) < 0x10000u) |
                    ((int)(d.fillb - d.bpos) < (int)(8 * DEC_NEED_WIDE));
  if (__builtin_expect(__any((int)rare), 0)) {
    if (rare) dec_rare(d, DEC_NEED_WIDE);
  }
  return s;
}

// 8 symbols into one 16-B block (half j of word q = symbol 2q + j)
template <int DIV>
static __device__ __forceinline__ uint4 wide16f_block8(Wide16FineDec& d, const Wide16FineArgs& a) {
  u32 w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32 s0 = wide16f_dec_sym<DIV>(d, a);
    const u32 s1 = wide16f_dec_sym<DIV>(d, a);
    w[q] = s0 | (s1 << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DIV>
__global__ __launch_bounds__(1024) void k_decode_wide16_fine(
    Wide16FineArgs a, const uint8_t* __restrict__ code, const u64* __restrict__ code_off,
    const u64* __restrict__ code_len, uint16_t* __restrict__ syms_out,
    const u64* __restrict__ sym_off, u32 n_chunks, u32* __restrict__ flags) {
  rc_set_prio(a.m);
  // dynamic LDS: the bucket table at address 0 (a read of it needs no base add), then the code
  // rings
  extern __shared__ u32 s_dyn[];
  const u32 tid = threadIdx.x, lanes = blockDim.x;
  constexpr u32 ring0 = RC_W16F_BUCKET_LDS;
  constexpr u32 bwords = (1u << (RC_W16F_BITS - 1)) + 1u;  // 2^bits + 2 halfwords
  static_assert(4u * bwords <= ring0, "the bucket table overlaps the rings");
  for (u32 j = tid; j < bwords; j += lanes) s_dyn[j] = reinterpret_cast<const u32*>(a.bucket)[j];
  __syncthreads();
  const u32 k = blockIdx.x * lanes + tid;
  if (k >= n_chunks) return;
  // (the default rounding mode stays: the hint is a plain product, and the verification is exact)
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

  Wide16FineDec d;
#ifdef RC_WIDE16_FINE_STATS
  d.st_steps = d.st_search = d.st_fix = 0;
#endif
  d.low = 0;
  d.range = ~0ull;
  d.err = 0;
  d.fillb = 0;
  d.pend_ok = 0;
  d.G = 0.0f;
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

  u32 i = 0;
  // head: single symbols until the output is 64-B aligned (it is 2-B aligned); every symbol
  // leaves DEC_NEED_WIDE bytes staged for the next one, so there is no ring check between them
  u32 head = ((64 - ((u32)(uintptr_t)op & 63)) & 63) >> 1;
  if (head > n) head = n;
  for (; i < head; ++i) op[i] = (uint16_t)wide16f_dec_sym<DIV>(d, a);
  // body: 16-symbol phases of two 16-B blocks, written in 64-B bursts of two phases
  uint4* ob = reinterpret_cast<uint4*>(op + i);
  const u32 nfull = (n - i) >> 4;  // whole phases (bursts of two, then a single one)
#define RC_WIDE16F_PHASE(oa, ob_)               \
  const uint4 oa = wide16f_block8<DIV>(d, a);   \
  const uint4 ob_ = wide16f_block8<DIV>(d, a);  \
  dec_phase(d);
  for (u32 b = 0; b < nfull / 2; ++b) {
    rc_prio_rotate(a.m.prio_rot);
    RC_WIDE16F_PHASE(o0, o1) RC_WIDE16F_PHASE(o2, o3)
    uint4* ob_b = ob + 4 * b;
    ob_b[0] = o0;
    ob_b[1] = o1;
    ob_b[2] = o2;
    ob_b[3] = o3;
  }
  if (nfull & 1) {
    RC_WIDE16F_PHASE(o0, o1)
    uint4* ob_b = ob + 2 * (nfull - 1);
    ob_b[0] = o0;
    ob_b[1] = o1;
  }
#undef RC_WIDE16F_PHASE
  i += nfull << 4;
  for (; i < n; ++i) op[i] = (uint16_t)wide16f_dec_sym<DIV>(d, a);
#ifdef RC_WIDE16_FINE_STATS
  atomicAdd(&g_wide16_fine_stats[0], (unsigned long long)d.st_steps);
  atomicAdd(&g_wide16_fine_stats[1], (unsigned long long)d.st_search);
  atomicAdd(&g_wide16_fine_stats[2], (unsigned long long)d.st_fix);
#endif
  flags[k] = cuwg_dec_flag(d);
}

// ------------------------------------------------------------------------------------------
// Host: the plan and the launchers
// ------------------------------------------------------------------------------------------
void rc_wide16_fine_plan(u32 n, u32 total, Wide16Plan* p) {
  memset(p, 0, sizeof *p);
  if (n < 1 || n > RC_MAX_WIDE16_SYMBOLS || total <= 65536u || total > RC_MAX_WIDE16_FINE_TOTAL)
    return;
  // encoder: no table in LDS, the rings of all the lanes a CU holds at 128 VGPRs
  p->enc_lanes = 1024;
  p->enc_lds = 1024 * SET_ENC_LANE_BYTES;
  p->enc_layout = 0;
  p->enc_tab = 8u * (n + (n < 65536u ? 1u : 0u));
  // decoder: the bucket table beside the rings, whole pairs of waves per SIMD
  p->dec_bits = RC_W16F_BITS;
  p->dec_shift = bitlen(total - 1) - RC_W16F_BITS;  // (>= 1: total > 2^16)
  const u32 fit = (SET_LDS_BYTES - RC_W16F_BUCKET_LDS) / SET_DEC_LANE_BYTES & ~127u;
  p->dec_lanes = fit < 1024u ? fit : 1024u;
  p->dec_lds = RC_W16F_BUCKET_LDS + p->dec_lanes * SET_DEC_LANE_BYTES;
}

static u32 g_w16f_last_lanes[2];
extern "C" void rc_wide16_fine_last_lanes_(uint32_t* out2) {
  out2[0] = g_w16f_last_lanes[0];
  out2[1] = g_w16f_last_lanes[1];
}

hipError_t rc_wide16_fine_encode_launch(hipStream_t stream, const RcKnobs& k,
                                        const Wide16FineArgs& a_in, int div, const Wide16Plan& p,
                                        const uint16_t* syms, const u64* sym_off, u32 n_chunks,
                                        uint8_t* out, const u64* out_off, u64* out_len,
                                        u32* flags) {
  Wide16FineArgs a = a_in;
  g_w16f_last_lanes[0] = set_launch_lanes(p.enc_lanes, n_chunks);
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioEncoder, p.enc_lanes, SET_ENC_LANE_BYTES,
                       p.enc_lds, n_chunks, syms, sym_off, n_chunks, out, out_off, out_len, flags);
  };
  return div == DIV_POW2 ? go(k_encode_wide16_fine<DIV_POW2>)
                         : go(k_encode_wide16_fine<DIV_MAGIC>);
}

hipError_t rc_wide16_fine_decode_launch(hipStream_t stream, const RcKnobs& k,
                                        const Wide16FineArgs& a_in, int div, const Wide16Plan& p,
                                        const uint8_t* code, const u64* code_off,
                                        const u64* code_len, uint16_t* syms_out,
                                        const u64* sym_off, u32 n_chunks, u32* flags) {
  Wide16FineArgs a = a_in;
  const u32 plan_lanes = p.dec_lanes, plan_lds = p.dec_lds;
  g_w16f_last_lanes[1] = set_launch_lanes(plan_lanes, n_chunks);
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.m, kPrioDecoder512, plan_lanes, SET_DEC_LANE_BYTES,
                       plan_lds, n_chunks, code, code_off, code_len, syms_out, sym_off, n_chunks,
                       flags);
  };
  return div == DIV_POW2 ? go(k_decode_wide16_fine<DIV_POW2>)
                         : go(k_decode_wide16_fine<DIV_MAGIC>);
}
