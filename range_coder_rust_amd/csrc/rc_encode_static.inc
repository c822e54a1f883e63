// rc_encode_static.inc — k_encode_static (rc_encode.hip), and with RC_ENC_GROUPED its grouped twin
// k_encode_static_grouped (rc_chunk_set.hip; static chunk sets, rc_chunk_set.h): the lane's
// chunk comes from g.order, a dead lane being ~0u there, and the workgroup stages row
// g.wg_row[blockIdx.x] of the set.  The preprocessor makes the difference, so that k_encode_static
// compiles from the tokens it had before there were chunk sets.  The including unit defines
// g_sink and RC_ENC_TU (its stamp buffer in scratch -DRC_STAMP builds).
#ifdef RC_ENC_GROUPED
#define RC_ENC_KERNEL k_encode_static_grouped
#define RC_ENC_GRP_PARAM GroupArgs g,
#else
#define RC_ENC_KERNEL k_encode_static
#define RC_ENC_GRP_PARAM
#endif
template <int DIV, int SM>
__global__ __launch_bounds__(WG, ENC_WAVES) void RC_ENC_KERNEL(ModelArgs m, RC_ENC_GRP_PARAM const uint8_t* __restrict__ syms,
                                                        const u64* __restrict__ sym_off,
                                                        u32 n_chunks, uint8_t* __restrict__ out,
                                                        const u64* __restrict__ out_off,
                                                        u64* __restrict__ out_len,
                                                        u32* __restrict__ flags) {
  RC_STAMP_BEGIN();
  rc_set_prio(m);
#ifdef RC_ENC_GROUPED
  {  // a workgroup with no class leaves before staging
    const u32 row = g.wg_row[blockIdx.x];
    if (row == ~0u) return;
    m.tab += (size_t)row * 256;
  }
#endif
  __shared__ uint2 s_tab[256];
  // (1-KiB aligned: a column base has no bits in the row field, ENC_ROWS)
  __shared__ __attribute__((aligned(1024))) u32 s_ring[WAVES * ENC_RING * 64];
  __shared__ EncOut s_out[WG];
  __shared__ u32 s_rank[WG];  // per wave: the lanes holding a unit, by rank (flush rounds)
  const u32 tid = threadIdx.x;
  {
    // SM (cum < 2^16): a symbol the reference cannot encode (c == 0: endless loop; outside the
    // alphabet: panic) is staged as (flag << 24, c = 1), so the common path only ORs entries
    // together; a chunk whose OR shows a flag is re-scanned for its first error at the end
    uint2 t = m.tab[tid];
    if (SM == 1 && t.y == 0)
      t = make_uint2((t.x == 0xFFFFFFFFu ? RC_F_BAD_SYMBOL : RC_F_ZERO_FREQ) << 24, 1u);
    s_tab[tid] = t;
  }
  const u32 lane = tid & 63, wave = tid >> 6;
#ifdef RC_ENC_GROUPED
  const u32 k = g.order[blockIdx.x * WG + tid];
  const bool live = k != ~0u;  // dead lanes still take part in the wave's flush rounds
#else
  const u32 k = blockIdx.x * WG + tid;
  const bool live = k < n_chunks;  // dead lanes still take part in the wave's flush rounds
#endif
#if ENC_WAVES == 4
  RC_VGPR_FLOOR_128();
#endif

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
  const u32 a = (u32)(((uintptr_t)out + o0) & (ENC_UNIT - 1));
  u64 cap = o1 - o0;
  if (cap > 0xFFFFFF00ull - a) cap = 0xFFFFFF00ull - a;
  s_out[tid].gbase = out + o0 - a;
  s_out[tid].lo_ok = a;
  s_out[tid].hi_ok = a + (u32)cap;
  __syncthreads();
  const u32* wring = s_ring + wave * ENC_RING * 64;
  const EncOut* wout = s_out + wave * 64;
  u32* const wrank = s_rank + wave * 64;

  Enc e;
#ifdef RC_FILL
  e.fill = 0;
#endif
  e.low = 0;  // RangeCoder::default (range_coder.rs:13-20)
  e.range = ~0ull;
  e.acc = 0;
  e.B = 8 * a;  // pad bytes in front of the slot (never stored)
  e.fthr = 8u * FLUSH_AT;  // fpos = 0
  e.err = 0;
  e.ring = (u32)(uintptr_t)(__attribute__((address_space(3))) u32*)(s_ring + wave * ENC_RING * 64 +
                                                                     ring_col(lane));

  const uint8_t* sp = syms + s0;
  u64 head = (64 - ((uintptr_t)sp & 63)) & 63;  // symbols before the first 64-B aligned tile
  if (head > n) head = n;
  const u64 ntile = (n - head) >> 6;
  // head: byte-wise, all lanes in step (flush rounds are wave-wide)
  for (u64 i = 0; __any((int)(i < head)); ++i) {
    enc_byte_sym<DIV, SM>(e, m, s_tab, sp, i, i < head, lane, wring, wout, wrank);
    if ((i & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }
  // body, part 1: the tiles every live lane of the wave has, with every lane active (no
  // per-symbol exec masking).  Dead lanes run along on a dummy tile (g_sink, zeros) and a slot
  // with no writable bytes; their results are dropped.
  u64 tm = live ? ntile : ~0ull;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const u64 v = ((u64)(u32)__shfl_xor((int)hi32(tm), o) << 32) | (u32)__shfl_xor((int)(u32)tm, o);
    tm = v < tm ? v : tm;
  }
  if (tm == ~0ull) tm = 0;  // no live lane in this wave
  const u64 tmin = ((u64)__builtin_amdgcn_readfirstlane(hi32(tm)) << 32) |
                   __builtin_amdgcn_readfirstlane((u32)tm);  // wave-uniform (scalar) trip count
  const uint4* tp = live ? reinterpret_cast<const uint4*>(sp + head)
                         : reinterpret_cast<const uint4*>(g_sink);
  // 64-symbol tiles, 4 x 16 B per lane, the next tile in flight while the current one is coded
  // (explicit registers: as arrays the compiler put the tiles in scratch memory, round 5).
  // ENC_TILE_Q 2 (scratch builds): 32-symbol half tiles, 16 registers fewer.
  const u64 tstep = live ? ENC_TILE_Q : 0;  // uint4s per load
  const u64 trips = tmin * (4 / ENC_TILE_Q);
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
  if (trips) {
    c0 = tp[0];
    c1 = tp[1];
    if (ENC_TILE_Q == 4) {
      c2 = tp[2];
      c3 = tp[3];
    }
  }
  for (u64 t = 0; t < trips; ++t) {
    rc_prio_rotate(m.prio_rot);
    uint4 n0 = c0, n1 = c1, n2 = c2, n3 = c3;
    if (t + 1 < trips) {
      const uint4* q = tp + (t + 1) * tstep;
      n0 = q[0];
      n1 = q[1];
      if (ENC_TILE_Q == 4) {
        n2 = q[2];
        n3 = q[3];
      }
    }
    enc16<DIV, SM>(e, m, s_tab, c0, true, lane, wring, wout, wrank);
    enc16<DIV, SM>(e, m, s_tab, c1, true, lane, wring, wout, wrank);
    if (ENC_TILE_Q == 4) {
      enc16<DIV, SM>(e, m, s_tab, c2, true, lane, wring, wout, wrank);
      enc16<DIV, SM>(e, m, s_tab, c3, true, lane, wring, wout, wrank);
    }
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
  }
  // body, part 2 (ragged waves): the remaining 16-symbol blocks of the tiles, lanes masked
  const u64 nblk = ntile * 4;
  for (u64 b = tmin * 4; __any((int)(b < nblk)); ++b) {
    const bool act = b < nblk;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (act) v = tp[b];
    enc16<DIV, SM>(e, m, s_tab, v, act, lane, wring, wout, wrank);
  }
  const u64 tail0 = head + (ntile << 6);
  for (u64 j = 0; __any((int)(tail0 + j < n)); ++j) {  // j is wave-uniform
    enc_byte_sym<DIV, SM>(e, m, s_tab, sp, tail0 + j, tail0 + j < n, lane, wring, wout,
                          wrank);
    if ((j & 7) == 7) enc_flush(e, lane, wring, wout, wrank);
  }

  // Encoder::finish (encoder.rs:40-46): 8 x left_shift
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    enc_emit_byte(e, (u32)(e.low >> 56));
    e.low <<= 8;
  }
  const u32 len = (e.B >> 3) - a;
  u32 wend = enc_wpos(e);
  if (e.B & 31) {  // the last, incomplete dword
    ring_put(e.ring, (e.B >> 5) & (ENC_RING - 1), (u32)(e.acc << (32 - (e.B & 31))));
    wend += 4;
  }
  // final rounds: the last (partial) units, clipped to the stream end
  const u32 end = a + len;
  if (end < s_out[tid].hi_ok) s_out[tid].hi_ok = end;
  while (__any((int)(enc_fpos(e) < wend)))
    enc_round(e, enc_fpos(e) < wend, lane, wring, wout, wrank);
  RC_STAMP_END(RC_ENC_TU, blockIdx.x * WAVES + wave, lane, n);
  if (live) {
    if (SM == 1) e.err = (e.err >> 24) ? enc_first_error(m, sp, n) : 0u;
    if (!e.err && (u64)len > cap) e.err = RC_F_CAPACITY;
    out_len[k] = too_long ? 0u : len;
    flags[k] = too_long ? RC_F_TOO_LONG : e.err;
  }
}
