// rc_rows.hip — resumable streams against per-symbol tables held in device memory
// (include/range_coder.h, rc_stream_decode_rows / rc_stream_encode_rows).
//
// rc_stream_decode (rc_resume.hip) takes one table for every symbol of a call, so a stream whose
// model changes from symbol to symbol cannot be decoded in one launch.  Here the tables are the
// rows of an n_rows x n_symbols array in device memory and row_of names one row per symbol.  The
// rows are known before any symbol is decoded, so nothing of the model depends on the coder.
//
// Decode: one wave per stream.  The coder's state is wave-uniform.  The row of a symbol is read
// once, coalesced (lane l holds cum[r][l + 64 h] and c[r][l + 64 h], h < G groups); every
// comparison the reference's bisection can make (cum[j] <= rfreq) goes into G ballot masks, and
// the search walks the masks step for step (FreqTable::find_index, sample_impl.rs:27-45: the same
// comparisons on the same path, so a non-monotone cum gives the reference's symbol).  c[left] and
// cum[left] come out of the held registers by readlane.  The loads of symbol i + RC_ROWS_D are
// issued while symbol i is coded (a register ring with static indices: the loop is unrolled by
// RC_ROWS_D).  Code bytes are read as a wave-wide window of two 256-B halves, the second loaded
// while the first is consumed; decoded symbols are collected per 64 and stored coalesced.
//
// Decode, many streams (k_stream_decode_rows_lane): one lane per stream, the
// row walked in device memory by the lane itself; rows_decode_plan picks between the two.
//
// Encode: one lane per stream, the shared encoder body with the triple gathered from the rows.
//
// The coder step (narrow_r and its sticky flags), the byte count of the renormalisation loops and
// the encoder body are rc_stream_dev.h's, shared with rc_resume.hip: the arithmetic of every
// stream kernel is the reference's, branch for branch, and is written once.
#include "rc_stream_dev.h"

#ifndef RC_ROWS_D
#define RC_ROWS_D 4  // prefetch depth in symbols: 1, 2, 4 or 8 (the sweep)
#endif
static_assert(RC_ROWS_D == 1 || RC_ROWS_D == 2 || RC_ROWS_D == 4 || RC_ROWS_D == 8,
              "the ring's slot of symbol i is i % RC_ROWS_D in every 64-symbol block");

namespace {

static __device__ __forceinline__ u32 rfl(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
static __device__ __forceinline__ u64 rfl64(u64 v) {
  return ((u64)rfl((u32)(v >> 32)) << 32) | rfl((u32)v);
}
static __device__ __forceinline__ u32 rdl(u32 v, u32 l) { return __builtin_amdgcn_readlane(v, l); }

// The stream's code bytes as the wave sees them: two 256-B halves, lane l of half h holding the
// aligned dword at address base + 256 h + 4 l.  A dword is loaded only if it lies inside the
// 64-B segments that hold a byte of the stream ([lo64, lo64 + span64)); any other reads as 0 and
// is never consumed (the caller checks pos + nb <= code_len first).
struct Window {
  u64 base;    // address of byte 0 of half 0 (a multiple of 4)
  u64 pos0;    // stream position of that byte (mod 2^64)
  u32 w0, w1;  // this lane's dword of each half
};
static __device__ __forceinline__ u32 win_load(u64 a, u64 lo64, u64 span64) {
  return a - lo64 < span64 ? gload((const u32*)a) : 0u;
}
// the halves that cover stream position pos (at address a0 + pos)
static __device__ __forceinline__ void win_fill(Window& w, u64 a0, u64 pos, u64 lo64, u64 span64,
                                                u32 lane) {
  const u64 a = a0 + pos;
  w.base = a & ~3ull;
  w.pos0 = pos - (a & 3ull);
  w.w0 = win_load(w.base + 4 * lane, lo64, span64);
  w.w1 = win_load(w.base + 256 + 4 * lane, lo64, span64);
}
// once pos has entered half 1: half 1 becomes half 0, and the next 256 B are requested
static __device__ __forceinline__ void win_advance(Window& w, u64 pos, u64 lo64, u64 span64,
                                                   u32 lane) {
  if (pos - w.pos0 >= 256) {
    w.base += 256;
    w.pos0 += 256;
    w.w0 = w.w1;
    w.w1 = win_load(w.base + 256 + 4 * lane, lo64, span64);
  }
}
// the byte at stream position pos (pos - pos0 < 512)
static __device__ __forceinline__ u32 win_byte(const Window& w, u64 pos) {
  const u32 off = (u32)(pos - w.pos0);
  const u32 d = off < 256 ? rdl(w.w0, (off >> 2) & 63) : rdl(w.w1, (off >> 2) & 63);
  return (d >> (8 * (off & 3))) & 255u;
}

// one symbol's row as the wave holds it: lane l, group h: entry l + 64 h of c and of cum
template <int G>
struct RowRegs {
  u32 c[G], cum[G];
};
template <int G>
static __device__ __forceinline__ void row_load(RowRegs<G>& o, const u32* __restrict__ c_tab,
                                                const u32* __restrict__ cum_tab, u32 row, bool ok,
                                                u32 n_alpha, u32 lane) {
#pragma unroll
  for (int h = 0; h < G; ++h) {
    const u32 j = lane + 64 * h;
    const bool in = ok && j < n_alpha;
    const u64 e = (u64)row * n_alpha + j;
    o.c[h] = in ? gload(c_tab + e) : 0u;
    o.cum[h] = in ? gload(cum_tab + e) : 0u;
  }
}
// entry j of a row out of its groups' registers (by value: handed over as an array, the groups of
// the 4-group kernel were kept in LDS by the compiler)
template <int G>
static __device__ __forceinline__ u32 pick(u32 v0, u32 v1, u32 v2, u32 v3, u32 j) {
  const u32 h = j >> 6;
  u32 x = v0;
  if constexpr (G > 1) x = h == 1 ? v1 : x;
  if constexpr (G > 2) x = h == 2 ? v2 : x;
  if constexpr (G > 2) x = h == 3 ? v3 : x;
  return rdl(x, j & 63);
}
template <int G>
static __device__ __forceinline__ u32 pick(const u32 (&v)[G], u32 j) {
  return pick<G>(v[0], v[G > 1], v[G > 2 ? 2 : 0], v[G > 2 ? 3 : 0], j);
}

// row index and total of the 64 symbols from stream symbol b0 on, one per lane; ok: the lanes
// whose symbol exists and names a row of the table
struct BlockRows {
  u32 row, total;
  u64 ok;
};
static __device__ __forceinline__ BlockRows block_rows(const u32* __restrict__ row_of,
                                                       const u32* __restrict__ total_tab,
                                                       u32 n_rows, u64 s0, u64 n, u64 b0,
                                                       u32 lane) {
  BlockRows o;
  const bool have = b0 < n && lane < n - b0;
  o.row = have ? gload(row_of + s0 + b0 + lane) : 0xFFFFFFFFu;
  const bool ok = have && o.row < n_rows;
  o.total = ok ? gload(total_tab + o.row) : 0u;
  o.ok = __ballot(ok);
  return o;
}

// Decoder::decode x n for stream blockIdx.x, G = ceil(n_alpha / 64) groups of table entries
template <int G>
__global__ __launch_bounds__(RWG) void k_stream_decode_rows(
    const u32* __restrict__ c_tab, const u32* __restrict__ cum_tab,
    const u32* __restrict__ total_tab, u32 n_rows, u32 n_alpha, const u32* __restrict__ row_of,
    rc_stream_state* __restrict__ st, const uint8_t* __restrict__ code,
    const u64* __restrict__ code_off, const u64* __restrict__ code_len,
    uint8_t* __restrict__ syms, const u64* __restrict__ sym_off, u32* __restrict__ flags) {
  constexpr int D = RC_ROWS_D;
  const u32 k = blockIdx.x, lane = threadIdx.x;
  const rc_stream_state S0 = st[k];  // (every lane reads the same 48 bytes)
  u32 sflags = rfl(S0.flags), stage = rfl(S0.stage);
  if (sflags) {  // the reference panicked at an earlier call
    if (lane == 0) flags[k] = sflags;
    return;
  }
  const u64 a0 = rfl64((u64)(code + gload64(code_off + k)));  // address of the stream's byte 0
  const u64 clen = rfl64(gload64(code_len + k));
  const u64 s0 = rfl64(gload64(sym_off + k)), n = rfl64(gload64(sym_off + k + 1)) - s0;
  const u64 lo64 = a0 & ~63ull;
  const u64 span64 = clen ? ((a0 + clen + 63) & ~63ull) - lo64 : 0;
  u64 low = rfl64(S0.lower_bound), range = rfl64(S0.range), data = rfl64(S0.data);
  u64 pos = rfl64(S0.pos), done = rfl64(S0.n);
  if (stage == 0 && clen < 8) {  // Decoder::new on fewer than 8 bytes (decoder.rs:14-23)
    if (lane == 0) {
      st[k].flags = RC_F_TRUNCATED;
      flags[k] = RC_F_TRUNCATED;
    }
    return;
  }
  // the rows of the first two blocks, and the tables of the first D symbols, before anything waits
  BlockRows A = block_rows(row_of, total_tab, n_rows, s0, n, 0, lane);
  BlockRows B = block_rows(row_of, total_tab, n_rows, s0, n, 64, lane);
  RowRegs<G> ring[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    row_load<G>(ring[d], c_tab, cum_tab, rdl(A.row, d), (A.ok >> d) & 1, n_alpha, lane);
  Window W;
  if (stage == 0) {  // Decoder::new: the first 8 bytes
    win_fill(W, a0, 0, lo64, span64, lane);
    data = 0;
    for (pos = 0; pos < 8; ++pos) data = (data << 8) | win_byte(W, pos);
    stage = 1;
  } else {
    win_fill(W, a0, pos, lo64, span64, lane);
  }
  for (u64 b0 = 0; b0 < n && !sflags; b0 += 64) {
    const u32 cnt = n - b0 < 64 ? (u32)(n - b0) : 64u;
    const BlockRows C = block_rows(row_of, total_tab, n_rows, s0, n, b0 + 128, lane);
    u32 symv = 0, got = 0;
    for (u32 i0 = 0; i0 < cnt && !sflags; i0 += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const u32 i = i0 + d;
        if (i >= cnt || sflags) break;
        const RowRegs<G> T = ring[d];
        {  // the ring's slot takes the table of symbol i + D (this block's or the next one's)
          const u32 t = i + D;
          const u32 tr = t < 64 ? rdl(A.row, t & 63) : rdl(B.row, t & 63);
          const bool tok = ((t < 64 ? A.ok : B.ok) >> (t & 63)) & 1;
          row_load<G>(ring[d], c_tab, cum_tab, tr, tok, n_alpha, lane);
        }
        const u32 total = rdl(A.total, i);
        // a row index >= n_rows; then find_index's range_par_total dividing by zero
        if (!((A.ok >> i) & 1) || total == 0) {
          sflags = RC_F_BAD_MODEL;
          break;
        }
        win_advance(W, pos, lo64, span64, lane);
        // FreqTable::find_index (sample_impl.rs:27-45)
        const u64 r = rfl64(rc_udiv64(range, total));
        const u64 rfreq = r ? rfl64(rc_udiv64(data - low, r)) : 0;
        u64 m[G];
#pragma unroll
        for (int h = 0; h < G; ++h)
          m[h] = __ballot(lane + 64 * h < n_alpha && (u64)T.cum[h] <= rfreq);
        u32 left = 0, right = n_alpha - 1;
        while (left < right) {
          const u32 mid = (left + right) >> 1, j = mid + 1;  // the reference reads cum[mid + 1]
          u64 w = m[0];
#pragma unroll
          for (int h = 1; h < G; ++h) w = (j >> 6) == (u32)h ? m[h] : w;
          if ((w >> (j & 63)) & 1) left = mid + 1;
          else right = mid;
        }
        const Narrow q = narrow_r(low, range, r, pick<G>(T.c, left), pick<G>(T.cum, left),
                                  RC_F_CORRUPT);
        if (q.err) {
          sflags = q.err;
          break;
        }
        // (counted inline: one count-and-apply helper for the decoders changed this kernel's code)
        u64 nl = q.low, nr = q.range;
        u32 nb = 0;
        while (((nl ^ (nl + nr)) >> 56) == 0) {  // no_carry_expansion (:110-116)
          nl <<= 8;
          nr <<= 8;
          ++nb;
        }
        while (nr < TOP16) {  // range_reduction_expansion (:126-135)
          nr = ~nl & (TOP16 - 1);
          nl <<= 8;
          nr <<= 8;
          ++nb;
        }
        if (pos + nb > clen) {  // shift_left_buffer pops past the end (decoder.rs:31-35)
          sflags = RC_F_TRUNCATED;
          break;
        }
        low = nl;
        range = nr;
        for (u32 j = 0; j < nb; ++j) data = (data << 8) | win_byte(W, pos++);
        symv = lane == i ? left : symv;
        got = i + 1;
      }
    }
    if (lane < got) gstore8(syms + s0 + b0 + lane, symv);  // the block's symbols, coalesced
    done += got;
    A = B;
    B = C;
  }
  if (lane == 0) {
    rc_stream_state S;
    S.lower_bound = low;
    S.range = range;
    S.data = data;
    S.pos = pos;
    S.n = done;
    S.flags = sflags;
    S.stage = stage;
    st[k] = S;
    flags[k] = sflags;
  }
}

// A lane's code bytes (k_stream_decode_rows_lane): the aligned 8 bytes at address wa, of which
// `off` are consumed, and the 8 behind them, requested when the window moved on.  A window is
// loaded only if it holds a byte of the stream ([lo8, lo8 + span8), the stream's own aligned
// 8-byte windows: all inside the 64-B segments that hold a byte of the stream); any other reads
// as 0 and is never consumed (the caller checks pos + nb <= code_len first).
struct LaneWin {
  u64 wa, cur, nxt;
  u32 off;
};
static __device__ __forceinline__ u64 lwin_load(u64 a, u64 lo8, u64 span8) {
  return a - lo8 < span8 ? gload64((const u64*)a) : 0ull;
}
static __device__ __forceinline__ void lwin_fill(LaneWin& w, u64 a, u64 lo8, u64 span8) {
  w.wa = a & ~7ull;
  w.off = (u32)a & 7u;
  w.cur = lwin_load(w.wa, lo8, span8);
  w.nxt = lwin_load(w.wa + 8, lo8, span8);
}
static __device__ __forceinline__ u32 lwin_byte(LaneWin& w, u64 lo8, u64 span8) {
  if (w.off == 8) {
    w.wa += 8;
    w.cur = w.nxt;
    w.nxt = lwin_load(w.wa + 8, lo8, span8);
    w.off = 0;
  }
  const u32 half = w.off < 4 ? (u32)w.cur : (u32)(w.cur >> 32);
  return (half >> (8 * (w.off++ & 3))) & 255u;
}

#ifndef RC_ROWS_LANE_L2
#define RC_ROWS_LANE_L2 0  // 1: the search resolves two levels per round trip (scratch builds)
#endif

// FreqTable::find_index's bisection over row cr (sample_impl.rs:33-44), every comparison read
// from the row in device memory: one dependent load per step.  With -DRC_ROWS_LANE_L2=1 a node's
// two possible children are requested with the node (each only if the bisection can reach it from
// here, which also keeps it inside the row): the same comparisons on the same path in half the
// round trips, and measured slower (three loads and their address arithmetic
// per round cost a lone wave more issue slots than the round trips they save).
static __device__ __forceinline__ u32 lane_find_index(const u32* __restrict__ cr, u32 n_alpha,
                                                      u64 rfreq) {
  u32 left = 0, right = n_alpha - 1;
#if RC_ROWS_LANE_L2
  while (left < right) {
    const u32 mid = (left + right) >> 1;
    const bool has_r = mid + 1 < right, has_l = left < mid;
    const u32 mid_r = (mid + 1 + right) >> 1, mid_l = (left + mid) >> 1;
    const u32 v = gload(cr + mid + 1);  // (mid + 1 <= right < n_alpha)
    const u32 vr = has_r ? gload(cr + mid_r + 1) : 0u;  // (mid_r + 1 <= right)
    const u32 vl = has_l ? gload(cr + mid_l + 1) : 0u;  // (mid_l + 1 <= mid)
    if ((u64)v <= rfreq) {
      left = mid + 1;
      if (has_r) {
        if ((u64)vr <= rfreq) left = mid_r + 1;
        else right = mid_r;
      }
    } else {
      right = mid;
      if (has_l) {
        if ((u64)vl <= rfreq) left = mid_l + 1;
        else right = mid_l;
      }
    }
  }
#else
  while (left < right) {
    const u32 mid = (left + right) >> 1;
    if ((u64)gload(cr + mid + 1) <= rfreq) left = mid + 1;
    else right = mid;
  }
#endif
  return left;
}

// Decoder::decode x n, one lane per stream: k_stream_decode_rows's results for
// launches of many streams, where 64 lanes doing one stream's scalar work leave the device idle.
// Every lane walks its own row in device memory; the row index of symbol i + 2 and the total of
// symbol i + 1 are requested while symbol i is coded.  A lane whose stream is done or flagged
// touches no memory but its one write-back while the wave's longest stream runs on.
__global__ __launch_bounds__(RWG) void k_stream_decode_rows_lane(
    const u32* __restrict__ c_tab, const u32* __restrict__ cum_tab,
    const u32* __restrict__ total_tab, u32 n_rows, u32 n_alpha, const u32* __restrict__ row_of,
    rc_stream_state* __restrict__ st, const uint8_t* __restrict__ code,
    const u64* __restrict__ code_off, const u64* __restrict__ code_len,
    uint8_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_streams,
    u32* __restrict__ flags) {
  const u32 k = blockIdx.x * RWG + threadIdx.x;
  if (k >= n_streams) return;
  RC_VGPR_FLOOR_80();
  rc_stream_state S = st[k];
  if (S.flags) {  // the reference panicked at an earlier call
    flags[k] = S.flags;
    return;
  }
  const u64 a0 = (u64)(code + gload64(code_off + k));  // address of the stream's byte 0
  const u64 clen = gload64(code_len + k);
  const u64 s0 = gload64(sym_off + k), n = gload64(sym_off + k + 1) - s0;
  if (S.stage == 0 && clen < 8) {  // Decoder::new on fewer than 8 bytes (decoder.rs:14-23)
    st[k].flags = RC_F_TRUNCATED;
    flags[k] = RC_F_TRUNCATED;
    return;
  }
  const u64 lo8 = a0 & ~7ull;
  const u64 span8 = clen ? ((a0 + clen + 7) & ~7ull) - lo8 : 0;
  // the rows of the first two symbols and the total of the first, before anything waits
  const u32* const rp = row_of + s0;
  u32 row_a = n > 0 ? gload(rp) : 0xFFFFFFFFu;
  u32 row_b = n > 1 ? gload(rp + 1) : 0xFFFFFFFFu;
  bool ok_a = row_a < n_rows;
  u32 total_a = ok_a ? gload(total_tab + row_a) : 0u;
  u64 low = S.lower_bound, range = S.range, data = S.data, pos = S.pos, done = S.n;
  u32 sflags = 0;
  LaneWin W;
  if (S.stage == 0) {  // Decoder::new: the first 8 bytes
    lwin_fill(W, a0, lo8, span8);
    data = 0;
    for (pos = 0; pos < 8; ++pos) data = (data << 8) | lwin_byte(W, lo8, span8);
    S.stage = 1;
  } else {
    lwin_fill(W, a0 + pos, lo8, span8);
  }
  uint8_t* const op = syms + s0;
  for (u64 i = 0; i < n; ++i) {
    const u32 row_c = i + 2 < n ? gload(rp + i + 2) : 0xFFFFFFFFu;
    const bool ok_b = row_b < n_rows;  // (no symbol i + 1: 2^32 - 1 names no row)
    const u32 total_b = ok_b ? gload(total_tab + row_b) : 0u;
    // a row index >= n_rows; then find_index's range_par_total dividing by zero
    if (!ok_a || total_a == 0) {
      sflags = RC_F_BAD_MODEL;
      break;
    }
    // FreqTable::find_index (sample_impl.rs:27-45)
    const u64 r = rc_udiv64(range, total_a);
    const u64 rfreq = r ? rc_udiv64(data - low, r) : 0;
    const u64 e = (u64)row_a * n_alpha;
    const u32 left = lane_find_index(cum_tab + e, n_alpha, rfreq);
    const Narrow q = narrow_r(low, range, r, gload(c_tab + e + left), gload(cum_tab + e + left),
                              RC_F_CORRUPT);
    if (q.err) {
      sflags = q.err;
      break;
    }
    // (counted inline: one count-and-apply helper for the decoders changed this kernel's code)
    u64 nl = q.low, nr = q.range;
    u32 nb = 0;
    while (((nl ^ (nl + nr)) >> 56) == 0) {  // no_carry_expansion (:110-116)
      nl <<= 8;
      nr <<= 8;
      ++nb;
    }
    while (nr < TOP16) {  // range_reduction_expansion (:126-135)
      nr = ~nl & (TOP16 - 1);
      nl <<= 8;
      nr <<= 8;
      ++nb;
    }
    if (pos + nb > clen) {  // shift_left_buffer pops past the end (decoder.rs:31-35)
      sflags = RC_F_TRUNCATED;
      break;
    }
    low = nl;
    range = nr;
    pos += nb;
    for (u32 j = 0; j < nb; ++j) data = (data << 8) | lwin_byte(W, lo8, span8);
    gstore8(op + i, left);
    ++done;
    row_a = row_b;
    ok_a = ok_b;
    total_a = total_b;
    row_b = row_c;
  }
  S.lower_bound = low;
  S.range = range;
  S.data = data;
  S.pos = pos;
  S.n = done;
  S.flags = sflags;
  st[k] = S;
  flags[k] = sflags;
}

// Encoder::encode x n (+ finish) for stream k: the shared body with the triple gathered from the
// rows.  The step's checks keep this order: the row, the symbol, the row's total.
__global__ __launch_bounds__(RWG) void k_stream_encode_rows(
    const u32* __restrict__ c_tab, const u32* __restrict__ cum_tab,
    const u32* __restrict__ total_tab, u32 n_rows, u32 n_alpha, const u32* __restrict__ row_of,
    const uint8_t* __restrict__ syms, rc_stream_state* __restrict__ st,
    const u64* __restrict__ sym_off, u32 n_streams, uint8_t* __restrict__ out,
    const u64* __restrict__ out_off, u64* __restrict__ out_len, uint8_t* __restrict__ nbytes,
    u32 finish, u32* __restrict__ flags) {
  const u32 k = blockIdx.x * RWG + threadIdx.x;
  if (k >= n_streams) return;
  RC_VGPR_FLOOR_48();
  stream_encode_body<false>(
      k, st, sym_off, out, out_off, out_len, nbytes, finish, flags,
      [=](u64 low, u64 range, u64 s0, u64 i) {
        const u32 row = gload(row_of + s0 + i);
        if (row >= n_rows) return Narrow{low, range, RC_F_BAD_MODEL};
        const u32 sym = syms[s0 + i];
        // c_freq(index) panics (sample_impl.rs:19)
        if (sym >= n_alpha) return Narrow{low, range, RC_F_BAD_SYMBOL};
        const u64 e = (u64)row * n_alpha + sym;
        const u32 total = gload(total_tab + row);
        if (total == 0) return Narrow{low, range, RC_F_BAD_MODEL};  // range_par_total divides by 0
        return narrow_r(low, range, rc_udiv64(range, total), gload(c_tab + e), gload(cum_tab + e),
                        RC_F_ZERO_FREQ);
      });
}

// Which decoder a launch takes: 0 the wave-per-stream kernel, 1 the lane-per-stream kernel
// (the sweep).  The wave kernel's rate stops growing once every SIMD holds a few
// of its waves; the lane kernel's grows with the stream count until the device is full of
// lanes.  The two curves cross at kRowsLaneStreamsPerCu streams per CU in both alphabets
// measured, so the rule does not look at n_symbols.  64 streams or fewer are one wave of the lane
// kernel: always the wave kernel.  Monotone in n_streams.
constexpr u32 kRowsLaneStreamsPerCu = 16;
int rows_decode_plan(u32 n_streams, u32 n_symbols, u32 n_cus) {
  (void)n_symbols;
  if (n_streams <= 64) return 0;
  return (u64)n_streams >= (u64)kRowsLaneStreamsPerCu * (n_cus ? n_cus : 1u) ? 1 : 0;
}

}  // namespace

extern "C" {

// Host-only hooks (tests/test_rows_plan.py, tools/kbench_rows.py; not in include/range_coder.h).
// The rule above, callable without a device.
int rc_rows_decode_plan_(uint32_t n_streams, uint32_t n_symbols, uint32_t n_cus) {
  return rows_decode_plan(n_streams, n_symbols, n_cus);
}

// rc_stream_decode_rows of this context: 0 by the rule, 1 always the wave kernel, 2 always the
// lane kernel.  Nothing else reads the value.
rc_status rc_rows_decoder_(rc_ctx* ctx, uint32_t which) {
  if (!ctx || which > 2) return RC_E_ARG;
  ctx->rows_decoder = which;
  return RC_OK;
}

rc_status rc_stream_decode_rows(rc_ctx* ctx, const uint32_t* c, const uint32_t* cum,
                                const uint32_t* total, uint32_t n_rows, uint32_t n_symbols,
                                const uint32_t* row_of, rc_stream_state* states,
                                const uint8_t* code, const uint64_t* code_off,
                                const uint64_t* code_len, uint8_t* syms, const uint64_t* sym_off,
                                uint32_t n_streams, uint32_t* flags) {
  if (!ctx || n_streams > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_symbols < 1 || n_symbols > 256) return RC_E_BAD_MODEL;
  if (n_streams == 0) return RC_OK;
  if (!c || !cum || !total || !row_of || !states || !code || !code_off || !code_len || !syms ||
      !sym_off || !flags || n_rows == 0)
    return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  bool lane = ctx->rows_decoder == 2;
  if (ctx->rows_decoder == 0 && n_streams > 64) {  // the rule (the device's CU count, asked once)
    if (!ctx->n_cus) {
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
          cus < 1)
        return RC_E_DEVICE;
      ctx->n_cus = (u32)cus;
    }
    lane = rows_decode_plan(n_streams, n_symbols, ctx->n_cus) == 1;
  }
  if (lane) {
    hipLaunchKernelGGL(k_stream_decode_rows_lane, dim3((n_streams + RWG - 1) / RWG), dim3(RWG), 0,
                       s, c, cum, total, n_rows, n_symbols, row_of, states, code, code_off,
                       code_len, syms, sym_off, n_streams, flags);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
  }
  auto kern = n_symbols <= 64 ? k_stream_decode_rows<1>
              : n_symbols <= 128 ? k_stream_decode_rows<2> : k_stream_decode_rows<4>;
  hipLaunchKernelGGL(kern, dim3(n_streams), dim3(RWG), 0, s, c, cum, total, n_rows, n_symbols,
                     row_of, states, code, code_off, code_len, syms, sym_off, flags);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}

rc_status rc_stream_encode_rows(rc_ctx* ctx, const uint32_t* c, const uint32_t* cum,
                                const uint32_t* total, uint32_t n_rows, uint32_t n_symbols,
                                const uint32_t* row_of, const uint8_t* syms,
                                rc_stream_state* states, const uint64_t* sym_off,
                                uint32_t n_streams, uint8_t* out, const uint64_t* out_off,
                                uint64_t* out_len, uint8_t* nbytes, uint32_t finish,
                                uint32_t* flags) {
  if (!ctx || n_streams > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_symbols < 1 || n_symbols > 256) return RC_E_BAD_MODEL;
  if (n_streams == 0) return RC_OK;
  if (!c || !cum || !total || !row_of || !syms || !states || !sym_off || !out || !out_off ||
      !out_len || !flags || n_rows == 0)
    return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  hipLaunchKernelGGL(k_stream_encode_rows, dim3((n_streams + RWG - 1) / RWG), dim3(RWG), 0, s, c,
                     cum, total, n_rows, n_symbols, row_of, syms, states, sym_off, n_streams, out,
                     out_off, out_len, nbytes, finish, flags);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}

}  // extern "C"
