// rc_order1.inc — the device source of the order-1 coders, k_encode_order1 / k_decode_order1,
// written once (DESIGN.md §9.13) and compiled by several translation units: rc_order1.hip
// instantiates the kernels of the lag-1 sets (period 1 and periodic), rc_order1_lag{2,4,8}.hip
// those of one lag each (RC_O1_LAG; DESIGN.md §9.15), so that the lag-1 unit holds the kernels it
// always held and the units build side by side.
#pragma once
#define RC_DEC_SHARED_ONLY
#include "rc_order1.h"

#include "rc_encode.inc"
#include "rc_decode.inc"
#include "rc_cuwg.inc"

// dummy symbol tiles of dead lanes (zeros); one per translation unit
#ifdef RC_O1_LAG
static __device__ uint4 g_o1sink[4];
#else
__device__ uint4 g_o1sink[4];
#endif

// ------------------------------------------------------------------------------------------
// Map policies: where in LDS the map of a symbol lies.  The kernels below are written once and
// instantiated with either (DESIGN.md §9.13); a map read is the same read with another base.
//   at(i):   the map that gives the row of the symbol at index i of the chunk (heads and tails)
//   align(h): called once behind a head of h symbols, before the 16-symbol blocks
//   blk(j):  the map that gives the row of in-block position j (a compile-time j)
// ------------------------------------------------------------------------------------------

// period 1 (row_i = map[sym[i-1]]): one map
struct O1Map1 {
  static constexpr bool kPeriodic = false;
  static constexpr int kLag = 1;
  u32 off;
  __device__ __forceinline__ void init(u32 map_off, u32) { off = map_off; }
  static __device__ __forceinline__ u32 period(const O1Args&) { return 1u; }
  __device__ __forceinline__ u32 pm() const { return 0u; }
  __device__ __forceinline__ u32 at(u32) const { return off; }
  __device__ __forceinline__ void align(u32) {}
  __device__ __forceinline__ u32 blk(int) const { return off; }
};

// periodic sets (rc_order1.h, DESIGN.md §9.12): row_i = map[i mod P][sym[i-1]], P in {2, 4, 8},
// the P maps staged slice behind slice.  The phase of a symbol is a property of the LANE: the
// byte-wise head of a chunk depends on its alignment, so the lanes of a wave sit at different
// symbol indices in the same 16-symbol block.  Behind a head of h symbols in-block position j of
// every block is symbol h + 16 b + j, whose phase (h + j) mod P does not depend on b (P divides
// 16): each lane holds the LDS addresses of the maps of in-block positions 0 .. 7 (mb[t]: slice
// (h + t) mod P, and position j uses mb[j & 7]) in 8 registers chosen by the compile-time j.
// Heads and tails take the slice from the symbol index.
struct O1MapP {
  static constexpr bool kPeriodic = true;
  static constexpr int kLag = 1;
  u32 off, mask, mb[8];
  __device__ __forceinline__ void init(u32 map_off, u32 period) {
    off = map_off;
    mask = period - 1;
  }
  static __device__ __forceinline__ u32 period(const O1Args& oa) { return oa.period; }
  __device__ __forceinline__ u32 pm() const { return mask; }
  __device__ __forceinline__ u32 at(u32 i) const { return off + ((i & mask) << 10); }
  __device__ __forceinline__ void align(u32 head) {
#pragma unroll
    for (u32 t = 0; t < 8; ++t) mb[t] = at(head + t);
  }
  __device__ __forceinline__ u32 blk(int j) const { return mb[j & 7]; }
};

// lagged sets (rc_order1.h, DESIGN.md §9.15): row_i = map[i mod P][sym[i-LAG]], LAG in {2, 4, 8},
// first_row for i < LAG.  The maps are the periodic policy's (P = 1: mask = 0, every mb[t] is the
// one map); the lag is the policy's compile-time constant, so the lag-1 instantiations of the
// kernels below keep their names and their code.  at(i) and blk(j) still name the map that gives
// the row OF symbol i / in-block position j; which symbol indexes it is the kernels' business.
template <int LAG>
struct O1MapLag : O1MapP {
  static_assert(LAG == 2 || LAG == 4 || LAG == 8, "lags of 2, 4 and 8 symbols");
  static constexpr int kLag = LAG;
};

// ------------------------------------------------------------------------------------------
// Encoder
// ------------------------------------------------------------------------------------------

// bytes of one staged row: 256 8-B (cum, c) entries (layout 0) or cum[0 .. 256] (layout 1)
template <int LAYOUT>
static __device__ __forceinline__ u32 o1_row_bytes() {
  return LAYOUT == 0 ? 2048u : 4u * SET_ROW_WORDS;
}

// the row offset the map gives for previous symbol p (a byte: every one of the 256 staged
// entries is a row of the set, so a symbol past the alphabet reads a harmless row too)
static __device__ __forceinline__ u32 o1_map(u32 map_off, u32 p) {
  return *(const l_u32*)(uintptr_t)(map_off + (p << 2));
}

// 16 symbols (one 16-B load), as set_enc16: the table entry is read two symbols ahead, pairs
// share one rare test, a flush check after every 8 symbols.  ro: the row of the tile's first
// symbol, carried from the symbol before the tile; the other 15 rows come from the tile itself
// (the row of symbol j is map[symbol j - 1]).  Leaves the row of the next tile's first symbol in
// ro.
template <int DIV, int LAYOUT, class MAP>
static __device__ __forceinline__ void o1_enc16(Enc& e, const ModelArgs& m, const MAP& mp, uint4 v,
                                                u32& ro, bool act, u32 lane, const u32* wring,
                                                const EncOut* wout, u32* wrank) {
  const u32 ws[4] = {v.x, v.y, v.z, v.w};
#define O1_SYM(j) ((ws[(j) >> 2] >> (8 * ((j) & 3))) & 255u)
  // the rows of all 16 symbols (and of the next block's first) are read before the block is
  // coded: they depend on the tile alone, and issued here they are not held back behind the
  // coder's ring stores, which the compiler must assume to alias the map
  u32 r[17];
  r[0] = ro;
#pragma unroll
  for (int j = 1; j <= 16; ++j) r[j] = o1_map(mp.blk(j), O1_SYM(j - 1));
  uint2 t = cuwg_enc_entry<LAYOUT>(r[0], O1_SYM(0));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      const int j = 4 * q + i;
      const uint2 t1 = cuwg_enc_entry<LAYOUT>(r[j + 1], O1_SYM(j + 1));
      // (past the tile's end: a harmless read of the last symbol in the next row)
      const uint2 tn = cuwg_enc_entry<LAYOUT>(r[j + 2], O1_SYM(j + 2 < 16 ? j + 2 : 15));
      enc_sym2<DIV, 1>(e, m, t, t1, act, lane, wring, wout, wrank);
      t = tn;
    }
    if (q & 1) enc_flush(e, lane, wring, wout, wrank);
  }
#undef O1_SYM
  if (act) ro = r[16];
}

// o1_enc16 at a lag of LAG symbols: the rows of in-block positions j >= LAG come from the tile
// itself (symbol j - LAG), those of positions j < LAG from the last LAG symbols before the block,
// carried as the previous block's last word pw (LAG = 8: its last two, pz then pw) and not as LAG
// rows, which would not fit the registers.  All 16 row reads issue before the block is coded, as
// above.  Leaves the block's own last words in (pz, pw); a masked lane keeps its own.
// FIRST (the blocks right behind a head shorter than the lag, outside the tile loop): the first
// nfirst in-block positions lie at less than LAG symbols from the chunk's start and take first_ro,
// one select per position below LAG.  Without FIRST every position has its context, and nfirst
// and first_ro are not read.
template <int DIV, int LAYOUT, int LAG, bool FIRST, class MAP>
static __device__ __forceinline__ void o1_enc16_lag(Enc& e, const ModelArgs& m, const MAP& mp,
                                                    uint4 v, u32& pz, u32& pw, u32 nfirst,
                                                    u32 first_ro, bool act, u32 lane,
                                                    const u32* wring, const EncOut* wout,
                                                    u32* wrank) {
  const u32 ws[4] = {v.x, v.y, v.z, v.w};
  const u32 pv[2] = {pz, pw};
#define O1_SYM(j) ((ws[(j) >> 2] >> (8 * ((j) & 3))) & 255u)
  // (symbol t of the block before, t in 8 .. 15)
#define O1_PREV(t) ((pv[((t) >> 2) - 2] >> (8 * ((t) & 3))) & 255u)
  u32 r[17];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    r[j] = o1_map(mp.blk(j), j >= LAG ? O1_SYM(j >= LAG ? j - LAG : 0)
                                      : O1_PREV(j < LAG ? 16 - LAG + j : 8));
    if (FIRST && j < LAG) r[j] = (u32)j < nfirst ? first_ro : r[j];
  }
  r[16] = r[15];  // (read ahead past the block only)
  uint2 t = cuwg_enc_entry<LAYOUT>(r[0], O1_SYM(0));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      const int j = 4 * q + i;
      const uint2 t1 = cuwg_enc_entry<LAYOUT>(r[j + 1], O1_SYM(j + 1));
      // (past the tile's end: a harmless read of the last symbol once more)
      const uint2 tn = cuwg_enc_entry<LAYOUT>(r[j + 2], O1_SYM(j + 2 < 16 ? j + 2 : 15));
      enc_sym2<DIV, 1>(e, m, t, t1, act, lane, wring, wout, wrank);
      t = tn;
    }
    if (q & 1) enc_flush(e, lane, wring, wout, wrank);
  }
#undef O1_PREV
#undef O1_SYM
  if (act) {
    pz = v.z;
    pw = v.w;
  }
}

// one symbol fetched byte-wise (unaligned head / tail of a chunk)
template <int DIV, int LAYOUT>
static __device__ __forceinline__ void o1_enc_byte(Enc& e, const ModelArgs& m, u32 map_off,
                                                   const uint8_t* sp, u64 i, u32& ro, bool act,
                                                   u32 lane, const u32* wring, const EncOut* wout,
                                                   u32* wrank) {
  const u32 sym = act ? (u32)sp[i] : 0u;
  enc_sym<DIV, 1>(e, m, cuwg_enc_entry<LAYOUT>(ro, sym), act, lane, wring, wout, wrank);
  const u32 rn = o1_map(map_off, sym);
  if (act) ro = rn;
}

// the same at a lag: the context of symbol i is read beside it (symbol i - LAG of the chunk; heads
// and tails are short), map_off is the map OF symbol i, and the first LAG symbols of a chunk
// take first_ro, the row of first_row
template <int DIV, int LAYOUT, int LAG>
static __device__ __forceinline__ void o1_enc_byte_lag(Enc& e, const ModelArgs& m, u32 map_off,
                                                       const uint8_t* sp, u32 i, u32 first_ro,
                                                       bool act, u32 lane, const u32* wring,
                                                       const EncOut* wout, u32* wrank) {
  const u32 sym = act ? (u32)sp[i] : 0u;
  const u32 p = act && i >= (u32)LAG ? (u32)sp[i - (u32)LAG] : 0u;
  const u32 rm = o1_map(map_off, p);
  enc_sym<DIV, 1>(e, m, cuwg_enc_entry<LAYOUT>(i >= (u32)LAG ? rm : first_ro, sym), act, lane,
                  wring, wout, wrank);
}

// the first symbol of a chunk the reference cannot encode (rare: flagged chunks only), walked
// with the context as the reference's caller would (periodic: with the phase, the row of symbol
// i + 1 is map[(i + 1) mod P][sym[i]], pm = P - 1)
template <bool PERIODIC>
static __device__ u32 o1_first_error(const u32* rows, const uint8_t* map, u32 first_row, u32 pm,
                                     u32 n_symbols, const uint8_t* sp, u64 n) {
  u32 j = first_row;
  for (u64 i = 0; i < n; ++i) {
    const u32 s = sp[i];
    if (s >= n_symbols) return RC_F_BAD_SYMBOL;
    const u32* row = rows + j * SET_ROW_WORDS;
    if (row[s + 1] == row[s]) return RC_F_ZERO_FREQ;
    j = PERIODIC ? map[((((u32)i + 1u) & pm) << 8) + s] : map[s];
  }
  return 0;
}

// the same walk with the lag: the row of symbol i >= LAG is map[i mod P][sym[i-LAG]], and every
// symbol before i has passed the alphabet test when it is read as a context
template <int LAG>
static __device__ u32 o1_first_error_lag(const u32* rows, const uint8_t* map, u32 first_row,
                                         u32 pm, u32 n_symbols, const uint8_t* sp, u64 n) {
  for (u64 i = 0; i < n; ++i) {
    const u32 s = sp[i];
    if (s >= n_symbols) return RC_F_BAD_SYMBOL;
    const u32 j = i >= (u64)LAG ? map[(((u32)i & pm) << 8) + sp[i - LAG]] : first_row;
    const u32* row = rows + j * SET_ROW_WORDS;
    if (row[s + 1] == row[s]) return RC_F_ZERO_FREQ;
  }
  return 0;
}

template <int DIV, int LAYOUT, class MAP>
__global__ __launch_bounds__(1024) void k_encode_order1(
    O1Args oa, const uint8_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_chunks,
    uint8_t* __restrict__ out, const u64* __restrict__ out_off, u64* __restrict__ out_len,
    u32* __restrict__ flags) {
  const SetArgs& a = oa.s;
  rc_set_prio(a.m);
  // dynamic LDS, sized by the plan: the K rows at address 0, the maps behind them (period 1: the
  // one map in the place of the indexed encoder's row K; else P KiB), then (1-KiB aligned) 8 KiB
  // of rings per wave, the lanes' output geometry and the waves' rank tables
  extern __shared__ __attribute__((aligned(1024))) u32 s_enc[];
  const u32 tid = threadIdx.x, lanes = blockDim.x, K = a.k;
  const ModelArgs& m = a.m;
  const u32 map_off = K * o1_row_bytes<LAYOUT>();
  MAP mp;
  mp.init(map_off, oa.period);
  if (LAYOUT == 0) {
    for (u32 en = tid; en < K * 256u; en += lanes) {
      const u32 row = en >> 8, s = en & 255u;
      const u32 c0 = a.rows[row * SET_ROW_WORDS + s], c1 = a.rows[row * SET_ROW_WORDS + s + 1];
      const uint2 t = s >= m.n ? make_uint2(RC_F_BAD_SYMBOL << 24, 1u)
                      : c1 == c0 ? make_uint2(RC_F_ZERO_FREQ << 24, 1u) : make_uint2(c0, c1 - c0);
      s_enc[2 * en] = t.x;
      s_enc[2 * en + 1] = t.y;
    }
  } else {
    for (u32 en = tid; en < K * SET_ROW_WORDS; en += lanes) s_enc[en] = a.rows[en];
  }
  for (u32 p = tid; p < MAP::period(oa) * 256u; p += lanes)
    s_enc[map_off / 4 + p] = (u32)oa.map[p] * o1_row_bytes<LAYOUT>();
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
  // the row of the lane's next symbol (at a lag: the row of first_row, for a chunk's first symbols)
  u32 ro = oa.first_row * o1_row_bytes<LAYOUT>();
  constexpr int LAG = MAP::kLag;
  u32 pz = 0, pw = 0;  // at a lag: the last words of the block before the lane's next one
  // (n <= 2^25 here: the symbol counters are 32-bit, which keeps the tile registers free)
  const u32 nn = (u32)ch.n;
  u32 head = (64 - ((u32)(uintptr_t)sp & 63)) & 63;  // symbols before the first 64-B aligned tile
  if (head > nn) head = nn;
  // at a lag, a head shorter than the lag leaves symbols that take first_row to the first block.
  // The tile loop has no place for them, so such a lane codes the 64 symbols behind its head as
  // four blocks of their own (`pre`, below) and its tiles start one tile later, still 64-B
  // aligned; with fewer than 64 symbols left it has no tile and codes them all byte-wise.
  [[maybe_unused]] u32 bhead = head;  // the symbols coded byte-wise in front of the blocks
  [[maybe_unused]] bool pre = false;
  if constexpr (LAG > 1) {
    if (head < (u32)LAG) {
      pre = nn - head >= 64;
      if (pre)
        head += 64;
      else
        bhead = head = nn;
    }
  }
  const u32 ntile = (nn - head) >> 6;
  // head: byte-wise, all lanes in step (flush rounds are wave-wide); symbol i leaves the row of
  // symbol i + 1
  if constexpr (LAG == 1) {
    for (u32 i = 0; __any((int)(i < head)); ++i) {
      o1_enc_byte<DIV, LAYOUT>(e, m, mp.at(i + 1), sp, i, ro, i < head, lane, wring, wout, wrank);
      if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
    }
  } else {
    for (u32 i = 0; __any((int)(i < bhead)); ++i) {
      o1_enc_byte_lag<DIV, LAYOUT, LAG>(e, m, mp.at(i), sp, i, ro, i < bhead, lane, wring, wout,
                                        wrank);
      if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
    }
    // the LAG symbols before the first block, where the blocks before it would have left them
    // (behind a short head the chunk has fewer: those positions take first_row)
    if (pre || ntile) {
#pragma unroll
      for (int t = 0; t < LAG; ++t) {
        if (bhead + (u32)t >= (u32)LAG) {
          const u32 b = (u32)sp[bhead + (u32)t - (u32)LAG] << (8 * ((16 - LAG + t) & 3));
          if (((16 - LAG + t) >> 2) == 3)
            pw |= b;
          else
            pz |= b;
        }
      }
    }
  }
  mp.align(head);  // the lane's maps of the in-block positions, for every block behind its head
  if constexpr (LAG > 1) {
    // the four blocks behind a short head, lanes masked as in the ragged loop below: block b
    // starts at symbol bhead + 16 b, and the first LAG - bhead positions of block 0 take first_row
    if (__any((int)pre)) {
      const uint4* q = reinterpret_cast<const uint4*>(pre ? sp + bhead
                                                          : reinterpret_cast<const uint8_t*>(g_o1sink));
      u32 nfirst = pre ? (u32)LAG - bhead : 0u;
      for (u32 b = 0; b < 4; ++b) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pre) v = q[b];
        o1_enc16_lag<DIV, LAYOUT, LAG, true>(e, m, mp, v, pz, pw, nfirst, ro, pre, lane, wring,
                                             wout, wrank);
        nfirst = 0;
      }
    }
  }
  // body, part 1: the tiles every live lane of the wave has, with every lane active; dead lanes
  // run along on a dummy tile and a slot with no writable bytes
  const u32 tmin = cuwg_tmin(live, ntile);
  const uint8_t* tp = live ? sp + head : reinterpret_cast<const uint8_t*>(g_o1sink);
  // 64-symbol tiles, 4 x 16 B per lane, the next tile in flight while the current one is coded
  // (explicit registers, as in k_encode_static)
  const u32 tstep = live ? 64 : 0;  // bytes per tile
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
  // one 16-symbol block: the carried row at lag 1, the carried words at a lag
#define O1_ENC16(v, act)                                                                   \
  if constexpr (LAG == 1)                                                                  \
    o1_enc16<DIV, LAYOUT>(e, m, mp, v, ro, act, lane, wring, wout, wrank);                 \
  else                                                                                     \
    o1_enc16_lag<DIV, LAYOUT, LAG, false>(e, m, mp, v, pz, pw, 0u, 0u, act, lane, wring,   \
                                          wout, wrank);
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
    O1_ENC16(c0, true)
    O1_ENC16(c1, true)
    O1_ENC16(c2, true)
    O1_ENC16(c3, true)
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
  }
  // body, part 2 (ragged waves): the remaining 16-symbol blocks of the tiles, lanes masked (a
  // masked lane keeps its carried row); block b starts at symbol head + 16 b like the full
  // tiles' blocks
  const u32 nblk = ntile * 4;
  for (u32 b = tmin * 4; __any((int)(b < nblk)); ++b) {
    const bool act = b < nblk;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (act) v = reinterpret_cast<const uint4*>(tp)[b];
    O1_ENC16(v, act)
  }
#undef O1_ENC16
  const u32 tail0 = head + (ntile << 6);
  for (u32 j = 0; __any((int)(tail0 + j < nn)); ++j) {  // j is wave-uniform
    if constexpr (LAG == 1)
      o1_enc_byte<DIV, LAYOUT>(e, m, mp.at(tail0 + j + 1), sp, tail0 + j, ro, tail0 + j < nn, lane,
                               wring, wout, wrank);
    else
      o1_enc_byte_lag<DIV, LAYOUT, LAG>(e, m, mp.at(tail0 + j), sp, tail0 + j, ro,
                                        tail0 + j < nn, lane, wring, wout, wrank);
    if ((j & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }

  const u32 len = cuwg_enc_finish(e, &l.out[tid], ch.al, lane, wring, wout, wrank);
  if constexpr (LAG == 1) {
    if (live)
      cuwg_enc_report(ch, k, len,
                      (e.err >> 24) ? o1_first_error<MAP::kPeriodic>(a.rows, oa.map, oa.first_row,
                                                                     mp.pm(), m.n, sp, ch.n)
                                    : 0u,
                      out_len, flags);
  } else {
    if (live)
      cuwg_enc_report(ch, k, len,
                      (e.err >> 24) ? o1_first_error_lag<LAG>(a.rows, oa.map, oa.first_row,
                                                              mp.pm(), m.n, sp, ch.n)
                                    : 0u,
                      out_len, flags);
  }
}

// ------------------------------------------------------------------------------------------
// Decoder
// ------------------------------------------------------------------------------------------
typedef Dec<DEC_LD, 0> O1Dec;

// the decoder's map word of row j: (LDS byte address of the cum row >> 2) | (the row's first
// bucket, in words) << 16; both are below 40,960 (160 KiB of 4-B words)
static __device__ __forceinline__ u32 o1_ctx_word(u32 j, u32 rows_off, u32 lut_bits) {
  return ((rows_off + j * (4u * SET_ROW_WORDS)) >> 2) | ((j << lut_bits) << 16);
}

// Decoder::decode(&models[row]) with FreqTable::find_index over that row, as set_dec_sym
// (rc_indexed.hip).  cw is the carried context: the map word of the row of THIS symbol.  The word
// of the next symbol's row, map[s], is read beside the candidate's (cum, c) and read again after
// a fix-up moved s, so cw is replaced only once the exact verification has fixed the symbol, and
// the next symbol's bucket read waits for one LDS read, not for a row number to be scaled.
template <int DIV>
static __device__ __forceinline__ u32 o1_dec_sym(O1Dec& d, const ModelArgs& m, u32 map_off,
                                                 u32& cw) {
  u32 roff, raddr;
  asm("v_and_b32 %0, %1, %2" : "=v"(roff) : "i"((DEC_RING - 1) << 5), "v"(d.bpos));
  asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(raddr) : "v"(roff), "v"((u32)(uintptr_t)d.ring));
  const l_u32* rp = (const l_u32*)(uintptr_t)raddr;
  const u32 D0 = rp[0], D1 = rp[O1Dec::kS];
  const u64 r = range_par_total<DIV, 1>(d.range, m);
  const float X = (float)(d.dhi() - hi32(d.low));
  const u32 qh = hint_floor(X, d.G);
  // the row's bucket (buckets at LDS address 0, 2^lut_bits 4-B entries per row)
  const u32 la = ((cw >> 16) + __builtin_amdgcn_ubfe(qh, m.lut_shift, m.lut_bits)) << 2;
  const u32 ent = *(const l_u32*)(uintptr_t)la;
  const u32 below = smask((qh & 0xFFFFu) - (ent >> 16));
  u32 s = __builtin_amdgcn_ubfe(ent, mselc(below, 0u, 8u), 8);
  const u32 rowa = (cw & 0xFFFFu) << 2;
  uint2 t = cuwg_cum_entry(rowa, s);
  u32 nw = *(const l_u32*)(uintptr_t)(map_off + (s << 2));  // (s < 256: inside the staged map)
  float tc = m.ftotal * __builtin_amdgcn_rcpf(cvt_f32(t.y));  // (hint only)
  u64 B = mul_rv<1>(r, t.y);
  u64 A = mul_rv<1>(r, t.x);
  const u64 dx = sub64((u32)d.dat, d.dhi(), d.low + A);  // x - r cum
  if (__builtin_expect(__any((int)(dx >= B)), 0)) {
    if (dx >= B) {
      cuwg_dec_fix<true>(s, t, A, B, d.x(), r, rowa, m.n);
      nw = *(const l_u32*)(uintptr_t)(map_off + (s << 2));
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
  cw = nw;
  return s;
}

// 16 symbols into one 16-B block, with the ring checks.  In-block position j reads the map of
// the symbol behind it, blk(j + 1); o1_dec_sym's second read after a fix-up takes the same base.
template <int DIV, class MAP>
static __device__ __forceinline__ uint4 o1_phase16(O1Dec& d, const ModelArgs& m, const MAP& mp,
                                                   u32& cw) {
  dec_gexact<1, 4>(d, m);  // bounds the drift of the carried scale to 16 symbols
  u32 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
      w[q] = put_byte(w[q], o1_dec_sym<DIV>(d, m, mp.blk(4 * q + jj + 1), cw), jj);
    if (q < 3 && ((q + 1) * 4) % DEC_CHECK_SPAN == 0) dec_check4<1, DEC_NEED_SPAN>(d);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// At a lag of LAG symbols the carried context is a queue of LAG map words in registers, cq[0] the
// word of the row of the next symbol: symbol i reads, through the map OF symbol i + LAG, the word
// that symbol will take.  o1_dec_sym is used as it is: it consumes a word and leaves the one read
// at the decoded symbol in its place (after a fix-up: read again with the same base).

// one symbol of a head or a tail (run-time index: the queue shifts); map_off: at(i + LAG)
template <int DIV, int LAG>
static __device__ __forceinline__ u32 o1_dec_sym_lag(O1Dec& d, const ModelArgs& m, u32 map_off,
                                                     u32 (&cq)[LAG]) {
  u32 w = cq[0];
  const u32 s = o1_dec_sym<DIV>(d, m, map_off, w);
#pragma unroll
  for (int t = 0; t + 1 < LAG; ++t) cq[t] = cq[t + 1];
  cq[LAG - 1] = w;
  return s;
}

// o1_phase16 at a lag: in-block position j consumes slot j mod LAG and refills it through
// blk(j + LAG), a compile-time choice of register; LAG divides 16, so the next symbol's word is
// in slot 0 again behind the phase
template <int DIV, class MAP, int LAG>
static __device__ __forceinline__ uint4 o1_phase16_lag(O1Dec& d, const ModelArgs& m, const MAP& mp,
                                                       u32 (&cq)[LAG]) {
  dec_gexact<1, 4>(d, m);  // bounds the drift of the carried scale to 16 symbols
  u32 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
      w[q] = put_byte(w[q],
                      o1_dec_sym<DIV>(d, m, mp.blk(4 * q + jj + LAG), cq[(4 * q + jj) % LAG]), jj);
    if (q < 3 && ((q + 1) * 4) % DEC_CHECK_SPAN == 0) dec_check4<1, DEC_NEED_SPAN>(d);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DIV, class MAP>
__global__ __launch_bounds__(1024) void k_decode_order1(
    O1Args oa, const uint8_t* __restrict__ code, const u64* __restrict__ code_off,
    const u64* __restrict__ code_len, uint8_t* __restrict__ syms_out,
    const u64* __restrict__ sym_off, u32 n_chunks, u32* __restrict__ flags) {
  const SetArgs& a = oa.s;
  rc_set_prio(a.m);
  // dynamic LDS, sized by the plan: the K rows' buckets at address 0 (a bucket read needs no
  // base add), the K cum-only rows, the maps (1 KiB each), then the code rings
  extern __shared__ u32 s_dyn[];
  const u32 tid = threadIdx.x, lanes = blockDim.x, K = a.k;
  const ModelArgs& m = a.m;
  const u32 lut_words = K << m.lut_bits;
  const u32 rows_off = 4u * lut_words;
  const u32 map_off = rows_off + 4u * K * SET_ROW_WORDS;
  MAP mp;
  mp.init(map_off, oa.period);
  for (u32 j = tid; j < lut_words; j += lanes) s_dyn[j] = a.lut[j];
  for (u32 j = tid; j < K * SET_ROW_WORDS; j += lanes) s_dyn[lut_words + j] = a.rows[j];
  for (u32 p = tid; p < MAP::period(oa) * 256u; p += lanes)
    s_dyn[map_off / 4 + p] = o1_ctx_word(oa.map[p], rows_off, m.lut_bits);
  __syncthreads();
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
  uint8_t* op = syms_out + s0;
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

  O1Dec d;
  d.low = 0;
  d.range = ~0ull;
  d.err = 0;
  d.fillb = 0;
  d.pend_ok = 0;
  d.ring = (l_u32*)(uintptr_t)(map_off + MAP::period(oa) * O1_MAP_BYTES) +
           wave * DEC_RING_ALLOC * 64 + lane;
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

  u32 cw = o1_ctx_word(oa.first_row, rows_off, m.lut_bits);  // the row of the next symbol
  constexpr int LAG = MAP::kLag;
  // at a lag: the words of the next LAG symbols, first_row's for a chunk's first
  [[maybe_unused]] u32 cq[LAG];
  if constexpr (LAG > 1) {
#pragma unroll
    for (int t = 0; t < LAG; ++t) cq[t] = cw;
  }
  u32 i = 0;
  // head: single symbols until the output is 64-B aligned; symbol i reads the map of symbol i + 1
  constexpr u32 OUT_ALIGN = 16 * DEC_OUT_BURST;
  static_assert(DEC_OUT_BURST == 4, "bursts of four phases");
  u32 head = (OUT_ALIGN - ((u32)(uintptr_t)op & (OUT_ALIGN - 1))) & (OUT_ALIGN - 1);
  if (head > n) head = n;
  dec_check4<1>(d);
  for (; i < head; ++i) {
    if constexpr (LAG == 1)
      op[i] = (uint8_t)o1_dec_sym<DIV>(d, m, mp.at(i + 1), cw);
    else
      op[i] = (uint8_t)o1_dec_sym_lag<DIV, LAG>(d, m, mp.at(i + LAG), cq);
    dec_check4<1>(d);
  }
  dec_check4<1, DEC_NEED_SPAN>(d);
  mp.align(head);
  // body: 16-symbol phases, bursts of four, then single ones
  uint4* ob = reinterpret_cast<uint4*>(op + i);
  const u32 nfull = (n - i) >> 4;
  const u32 nbu = nfull / DEC_OUT_BURST;
  u32 g = 0;  // phase
  // (one phase with the policy's carried context: the word at lag 1, the queue at a lag)
#define RC_O1_PHASE(o)                                     \
  uint4 o;                                                 \
  if constexpr (LAG == 1)                                  \
    o = o1_phase16<DIV, MAP>(d, m, mp, cw);                \
  else                                                     \
    o = o1_phase16_lag<DIV, MAP, LAG>(d, m, mp, cq);       \
  ++g;                                                     \
  dec_phase(d);                                            \
  dec_check4<1, DEC_NEED_SPAN>(d);
  for (u32 b = 0; b < nbu; ++b) {
    rc_prio_rotate(m.prio_rot);
    RC_O1_PHASE(o0) RC_O1_PHASE(o1) RC_O1_PHASE(o2) RC_O1_PHASE(o3)
    uint4* ob_b = ob + DEC_OUT_BURST * b;
    ob_b[0] = o0;
    ob_b[1] = o1;
    ob_b[2] = o2;
    ob_b[3] = o3;
  }
  while (g < nfull) {
    const u32 gb = g;
    RC_O1_PHASE(o)
    ob[gb] = o;
  }
#undef RC_O1_PHASE
  i += nfull << 4;
  for (; i < n; ++i) {
    if constexpr (LAG == 1)
      op[i] = (uint8_t)o1_dec_sym<DIV>(d, m, mp.at(i + 1), cw);
    else
      op[i] = (uint8_t)o1_dec_sym_lag<DIV, LAG>(d, m, mp.at(i + LAG), cq);
    dec_check4<1>(d);
  }
  flags[k] = cuwg_dec_flag(d);
}

