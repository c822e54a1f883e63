// rc_model_build.hip — the step before encode: building the frequency table from the data, on
// the GPU.
//
// The reference builds its model on the CPU, one symbol at a time: FreqTable::new, then
// add_alphabet_freq per symbol (examples/sample_impl.rs:49-60), then calc_cum's exclusive scan
// (:61-69).  Here:
//   * k_histogram counts symbols of many chunks at once (per-chunk and/or batch histograms):
//     16-B loads, eight u16 LDS sub-histograms per wave;
//   * rc_quantize_counts turns counts into a (c, cum, total) table: exactly calc_cum's table
//     when no target is given, or a table scaled to a target total (e.g. 2^16, so the coder
//     takes its fast power-of-two path), deterministic and restated by the oracle;
//   * k_ideal_bits is the batched PModel::ideal_code_length (pmodel.rs:14-40): per chunk,
//     sum over its histogram of count * log2(total / c), in f64;
//   * k_histogram_wide and k_ideal_bits_wide do both for the 16-bit symbols of wide static
//     models (up to 4096 bins; the ideal bits straight from the symbols, without a histogram);
//   * k_histogram_order1 counts by context class under a given map; k_histogram_pairs counts the
//     full 256 x 256 pair histogram, rc_cluster_contexts (host) fits a context map to it, and
//     k_ideal_bits_order1 prices a batch under an order-1 set (rc_order1.h);
//   * the k_cj_* kernels are that clustering on the device, jointly over the (phase, context)
//     items of periodic pair counts (rc_cluster_contexts_dev).
#include "rc_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define HWG 256  // k_ideal_bits

// k_histogram: chunk-stride workgroups of 4 waves; 16-B loads; LDS sub-histograms counted with
// ds_add_u32.  Measured (profiles/r03/ab/hist/): the LDS atomics' latency per
// wave binds, so the rate follows the resident waves per CU, and lanes of one instruction that
// hit one address serialise (a skewed model's hot symbols).  Hence small sub-histograms (4 KiB
// per wave: 32 waves per CU) with many copies: u16 counters, eight copies.
typedef __attribute__((address_space(3))) u32 hl_u32;

static __device__ __forceinline__ void hl_add(hl_u32* p, u32 v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Eight u16 sub-histograms per wave in the LDS of four u32 ones (4 KiB per wave, so 32 waves
// per CU as with four): lane L counts into copy L & 7; dword 8 (b & 127) + copy holds bins b
// (low half) and b + 128 (high half), so the hot low symbols of a skewed model never share a
// dword.  A u16 takes at most 8 lanes x HSEG_LANE symbols before the segment's readout.
#define HSEG_LANE 8176u  // symbols per lane per segment (16 x 511): 8 x (8176 + 2) < 2^16

// blocks [i0, i1) of the chunk (stride 256 from this thread's first) into the sub-histograms.
// HOT: symbol H (wave-uniform) is not added to LDS but counted by ballot into hc (an SGPR):
// the lanes of a skewed model's hottest symbol no longer serialise on its counters.
template <bool HOT>
static __device__ __forceinline__ void h8_blocks(const u32x4* v, u64 i0, u64 i1, u32 colb, u32 one,
                                                 u32 H, u32& hc) {
#pragma unroll 4
  for (u64 i = i0; i < i1; i += 256) {
    const u32x4 w = gload16(v + i);
    const u32 ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // per symbol: the dword's address as one bfe + one v_lshl_add_u32, the increment as
      // one SDWA shift reading byte j of x = 16 (b_j >> 7) per byte (asm: from C the
      // compiler re-derived each shift from the word with a shift, an and and an add)
      const u32 x = (ws[q] >> 3) & 0x10101010u;
      u32 a[4], y[4];
#define H8_SYM(j)                                                                               \
  asm("v_lshl_add_u32 %0, %1, 5, %2" : "=v"(a[j]) : "v"(__builtin_amdgcn_ubfe(ws[q], 8 * j, 7)), \
      "v"(colb));                                                                               \
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_" #j    \
      " src1_sel:DWORD"                                                                         \
      : "=v"(y[j]) : "v"(x), "v"(one));                                                        \
  if (HOT) {                                                                                    \
    const bool h = __builtin_amdgcn_ubfe(ws[q], 8 * j, 8) == H;                                 \
    hc += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(h));                            \
    if (!h) hl_add((hl_u32*)(uintptr_t)a[j], y[j]);                                             \
  } else {                                                                                      \
    hl_add((hl_u32*)(uintptr_t)a[j], y[j]);                                                     \
  }
      H8_SYM(0) H8_SYM(1) H8_SYM(2) H8_SYM(3)
#undef H8_SYM
    }
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_histogram(
    const uint8_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_chunks,
    u32* __restrict__ chunk_hist, u64* __restrict__ hist, u32 hot_ok) {
  __shared__ u32 sh[4 * 1024];
  __shared__ u32 s_hot[4];  // per wave: the segment's ballot count of the hot symbol
  __shared__ u32 s_key[4];  // per wave: max of (count << 8 | bin) of the last chunk
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // LDS byte address of this lane's copy; a VGPR holding 1 (the SDWA shift's operand)
  const u32 colb = (u32)(uintptr_t)(hl_u32*)(sh + wave * 1024 + (lane & 7));
  u32 one = 1;
  asm volatile("" : "+v"(one));
  RC_VGPR_FLOOR_64();
  u64 acc = 0;  // bin tid over this WG's chunks
  for (u32 j = tid; j < 4 * 1024; j += 256) sh[j] = 0;
  bool have_key = false;
  for (u32 k = blockIdx.x; k < n_chunks; k += gridDim.x) {
    const u64 s0 = sym_off[k], n = sym_off[k + 1] - s0;
    const uint8_t* p = syms + s0;
    u64 head = (16 - ((uintptr_t)p & 15)) & 15;
    if (head > n) head = n;
    const u64 nv = (n - head) >> 4;
    const u32x4* v = reinterpret_cast<const u32x4*>(p + head);
    u32 cnt = 0;
    // segments of 256 * HSEG_LANE / 16 blocks: every lane adds <= HSEG_LANE symbols per segment
    const u64 seg = 256ull * HSEG_LANE / 16;
    u32 H = 256, key = 0;
    for (u64 b0 = 0; b0 == 0 || b0 < nv; b0 += seg) {
      __syncthreads();
      if (b0 == 0) {
        // the hot symbol: the previous chunk's most frequent one, if it held >= 1/8 of it
        if (have_key && hot_ok) {
          key = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
          key = __builtin_amdgcn_readfirstlane(key);
        }
        H = key >> 8 ? (key & 255u) : 256u;
        if (tid < head) {
          const u32 b = p[tid];
          atomicAdd(&sh[wave * 1024 + (b & 127) * 8 + (lane & 7)], 1u << (16 * (b >> 7)));
        }
        const u64 t0 = head + (nv << 4);
        if (t0 + tid < n) {  // < 16 tail symbols
          const u32 b = p[t0 + tid];
          atomicAdd(&sh[wave * 1024 + (b & 127) * 8 + (lane & 7)], 1u << (16 * (b >> 7)));
        }
      }
      const u64 b1 = b0 + seg < nv ? b0 + seg : nv;
      u32 hc = 0;
      if (H < 256) h8_blocks<true>(v, b0 + tid, b1, colb, one, H, hc);
      else h8_blocks<false>(v, b0 + tid, b1, colb, one, H, hc);
      if (lane == 0) s_hot[wave] = hc;
      __syncthreads();
      // bin tid: the half (tid >> 7) of dwords 8 (tid & 127) + c of the four waves
#pragma unroll
      for (u32 w = 0; w < 4; ++w) {
        u32x4* r = reinterpret_cast<u32x4*>(sh + w * 1024 + (tid & 127) * 8);
#pragma unroll
        for (u32 h = 0; h < 2; ++h) {
          const u32x4 x = r[h];
          const u32 sft = 16 * (tid >> 7);
          cnt += ((x.x >> sft) & 0xFFFFu) + ((x.y >> sft) & 0xFFFFu) + ((x.z >> sft) & 0xFFFFu) +
                 ((x.w >> sft) & 0xFFFFu);
        }
      }
      if (tid == H) cnt += s_hot[0] + s_hot[1] + s_hot[2] + s_hot[3];
      __syncthreads();
      for (u32 j = tid; j < 4 * 1024; j += 256) sh[j] = 0;
    }
    if (chunk_hist) chunk_hist[(u64)k * 256 + tid] = cnt;
    acc += cnt;
    // this chunk's most frequent symbol, for the next one (read after the next barrier); a
    // bin below 1/8 of the chunk gives key 0 (no hot symbol)
    u32 kv = (u64)cnt * 8 >= n && n >= 4096 ? (min(cnt, 0xFFFFFFu) << 8) | tid : 0u;
#pragma unroll
    for (int o = 32; o; o >>= 1) kv = max(kv, (u32)__shfl_xor((int)kv, o));
    if (lane == 0) s_key[wave] = kv;
    have_key = true;
  }
  if (hist && acc) atomicAdd(reinterpret_cast<unsigned long long*>(hist + tid), (unsigned long long)acc);
}

// k_histogram_order1: pair counts by context class, the counts an order-1 set's rows are
// quantised from (rc_order1.h).  Row j of the result counts the symbols whose context row is j:
// first_row for a chunk's first symbol, map[previous symbol] for every other one.  Chunk-stride
// workgroups; a thread takes 16 consecutive symbols and the one before them; K x 256 u32 counters
// in LDS (dynamic, at most 64 KiB) and the 256-B map behind them, flushed into the u64 result
// before a counter can wrap: at most 2^32 - 1 symbols are counted between two flushes, so no
// counter exceeds that whatever the data.
struct O1HistMap {
  u32 w[64];  // the 256 map bytes
};
typedef u32x4 u32x4_h1 __attribute__((aligned(1)));
#define O1H_SEG (1ull << 30)  // symbols of a chunk counted between two looks at the budget

__global__ __launch_bounds__(256) void k_histogram_order1(
    O1HistMap map, u32 first_row, u32 K, const uint8_t* __restrict__ syms,
    const u64* __restrict__ sym_off, u32 n_chunks, u64* __restrict__ hist) {
  extern __shared__ u32 s_h1[];
  const u32 tid = threadIdx.x;
  const uint8_t* const s_map = reinterpret_cast<const uint8_t*>(s_h1 + K * 256u);
  for (u32 j = tid; j < K * 256u; j += 256) s_h1[j] = 0;
  if (tid < 64) s_h1[K * 256u + tid] = map.w[tid];
  __syncthreads();
  auto flush = [&]() {
    __syncthreads();
    for (u32 j = 0; j < K; ++j) {
      const u32 v = s_h1[j * 256u + tid];
      if (v) {
        atomicAdd(reinterpret_cast<unsigned long long*>(hist + j * 256u + tid),
                  (unsigned long long)v);
        s_h1[j * 256u + tid] = 0;
      }
    }
    __syncthreads();
  };
  u64 pending = 0;  // symbols counted since the last flush (workgroup-uniform)
  for (u32 k = blockIdx.x; k < n_chunks; k += gridDim.x) {
    const u64 s0 = sym_off[k], n = sym_off[k + 1] - s0;
    const uint8_t* p = syms + s0;
    for (u64 b0 = 0; b0 < n; b0 += O1H_SEG) {
      const u64 b1 = n - b0 < O1H_SEG ? n : b0 + O1H_SEG;
      if (pending + (b1 - b0) > 0xFFFFFFFFull) {
        flush();
        pending = 0;
      }
      pending += b1 - b0;
      for (u64 i = b0 + 16ull * tid; i < b1; i += 16ull * 256) {
        u32 row = i ? (u32)s_map[p[i - 1]] : first_row;  // chunk boundaries reset the context
        if (i + 16 <= b1) {
          const u32x4 v = *(const __attribute__((address_space(1))) u32x4_h1*)(p + i);
          const u32 ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32 s = (ws[q] >> (8 * j)) & 255u;
              atomicAdd(&s_h1[row * 256u + s], 1u);
              row = s_map[s];
            }
          }
        } else {
          for (u64 j = i; j < b1; ++j) {
            const u32 s = p[j];
            atomicAdd(&s_h1[row * 256u + s], 1u);
            row = s_map[s];
          }
        }
      }
    }
  }
  flush();
}

// k_histogram_pairs: the full 256 x 256 pair histogram of a batch (pair[p][s]: positions i >= 1
// of a chunk with sym[i-1] = p, sym[i] = s) and the histogram of the chunks' first symbols: the
// counts a context map is fitted from (rc_cluster_contexts).  65,536 u32 counters are 256 KiB,
// more than a CU's LDS, so the workgroups are split into O1P_SLICES groups by context: workgroup
// b belongs to group g = b % O1P_SLICES, reads every symbol of its chunks (chunk-stride within
// the group, so the groups' workgroups that read one chunk run side by side and share it in
// L2) and counts only the pairs whose previous symbol lies in [g R, (g + 1) R), R = 256 /
// O1P_SLICES, into R x 256 u32 counters in LDS; group 0 also counts the first symbols, into 256
// more.  Lane layout as k_histogram_order1: 16 consecutive symbols and the byte before them,
// O1P_SUB lanes to a chunk, so a workgroup walks O1P_WG / O1P_SUB chunks at a time (with all its
// lanes on one chunk, three in four idle on 4-KiB chunks).  Measured (profiles/order1_fit/,
// DESIGN.md §9.10): two slices of 1024-lane workgroups (129 KiB of LDS, one workgroup and 16
// waves per CU) beat four and eight slices with up to 32 waves per CU, because every slice
// reads and unpacks every symbol; u64 atomics straight into the result in L2 were 200 times
// slower.
// No counter can wrap: every symbol counted adds one to at most one counter of its workgroup,
// and the counters are flushed into the u64 results before the workgroup has counted 2^32
// symbols since the last flush, so none exceeds 2^32 - 1 whatever the data.
//
// PER (rc_histogram_pairs_periodic; periodic order-1 sets, rc_order1.h): the position in a record
// is a third index, pair[ph][p][s] counts the positions i >= 1 of a chunk with i mod P = ph,
// sym[i-1] = p and sym[i] = s.  The same structure with O1P_SLICES * P slices, (phase, part of
// the contexts): workgroup b belongs to slice g = b % (O1P_SLICES * P), phase g / O1P_SLICES and
// contexts [(g % O1P_SLICES) R, (g % O1P_SLICES + 1) R).  A lane's 16 consecutive symbols start
// at a multiple of 16 from the chunk's start (the segments are multiples of 16 too), so its j-th
// symbol has phase j mod P whatever the lane: the phase test is a compare of two wave-uniform
// values per unrolled j.  Every slice reads and unpacks every symbol, and the budget counts every
// symbol read, more than the slice counts.  Without PER, `period` is not read (P = 1: the phase
// test is always true and compiles away).
#ifndef O1P_SLICES       // (scratch builds: -DO1P_SLICES=n -DO1P_WG=lanes)
#define O1P_SLICES 2u
#endif
#ifndef O1P_WG
#define O1P_WG 1024u
#endif
#ifndef O1P_SUB
#define O1P_SUB 256u     // lanes that share a chunk
#endif
#define O1P_Q (O1P_WG / O1P_SUB)                  // chunks a workgroup walks at a time
#define O1P_SEG ((1ull << 31) / O1P_Q)            // symbols of a chunk between two looks at the budget
#define O1P_ROWS (256u / O1P_SLICES)              // contexts per slice
#define O1P_WORDS (O1P_ROWS * 256u + 256u)        // the slice's counters, then the first symbols'
#define O1P_LDS (4u * O1P_WORDS)

// (the source: rc_hist_pairs.inc, once for lag 1 and once for the lagged kernels)
#include "rc_hist_pairs.inc"
#define O1C_LAGGED
#include "rc_hist_pairs.inc"
#undef O1C_LAGGED

// k_ideal_bits_order1: per chunk the sum of icl[row_i][sym_i] over its symbols, row_0 =
// first_row and row_i = map[sym[i-1]], straight from the symbols: no histogram and no atomics.
// icl: K x 256 ideal code lengths in f64, +inf where c == 0 and from n_symbols on; it is staged
// in dynamic LDS once per workgroup (2 K KiB, 128 KiB at K = 64) with the 256-B map behind it
// (entries from n_symbols on are 0, as the coders stage them).  The table bounds the workgroups
// per CU, one at K = 64, so the host picks the workgroup size from K to keep 16 waves or more
// on the CU.  One wave per chunk, waves striding over the chunks (one workgroup per chunk was
// slower at every K, 2.8 times at K = 64 on 4-KiB chunks: DESIGN.md §9.10); a lane takes 16
// consecutive symbols and the byte before them (as k_histogram_order1) at a stride of 1024
// symbols, into a private f64 sum, and a butterfly adds the 64 sums.  Every term is >= 0 or +inf (there is no
// 0 * inf), so a chunk is +inf or finite, never NaN.  Accuracy: a lane adds at most
// 16 ceil(n_k / 1024) <= n_k / 64 + 16 non-negative terms one by one and the butterfly adds
// log2 64 = 6 more steps, so the relative error of a finite chunk of n_k symbols is at most
// about (n_k / 64 + 22) * 2^-53: below 1e-12 up to n_k = 5.7e5.
//
// PER (a periodic set, rc_order1.h): row_i = map[i mod P][sym[i-1]].  The lanes start at multiples
// of 16 from the chunk's start, so the symbol after a lane's j-th has phase (j + 1) mod P and the
// byte before its first pairs with phase 0: only the staged map (P x 256 B) and its index change;
// the sums, their order and so the accuracy bound are the same.  Without PER, `period` is not
// read (P = 1: every map index is the symbol).
// (the source: rc_ideal_bits_order1.inc, once for lag 1 and once for the lagged kernels)
#include "rc_ideal_bits_order1.inc"
#define O1C_LAGGED
#include "rc_ideal_bits_order1.inc"
#undef O1C_LAGGED

// per chunk: bits = sum_i hist[i] * icl[i] in f64 (icl[i] = +inf for c_i == 0: the reference's
// ideal_code_length returns Err there, pmodel.rs:16-18).  One wave per chunk: lane L reads bins
// 4L .. 4L+3 of the row as one 16-B load (the wave reads the whole 1-KiB row at once) and holds
// their icl in registers for every chunk; the 64 partial sums are added by a butterfly.  Empty
// bins are skipped (0 * inf would be NaN).
__global__ __launch_bounds__(HWG) void k_ideal_bits(const double* __restrict__ icl,
                                                    const u32* __restrict__ chunk_hist,
                                                    u32 n_chunks, double* __restrict__ bits) {
  const u32 lane = threadIdx.x & 63;
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  RC_VGPR_FLOOR_48();
  const double i0 = icl[4 * lane], i1 = icl[4 * lane + 1], i2 = icl[4 * lane + 2],
               i3 = icl[4 * lane + 3];
  const u32 nw = gridDim.x * (HWG / 64);
  for (u32 k = blockIdx.x * (HWG / 64) + wave; k < n_chunks; k += nw) {
    const u32x4 h = gload16(reinterpret_cast<const u32x4*>(chunk_hist + (u64)k * 256) + lane);
    double acc = 0.0;
    if (h.x) acc = fma((double)h.x, i0, acc);
    if (h.y) acc = fma((double)h.y, i1, acc);
    if (h.z) acc = fma((double)h.z, i2, acc);
    if (h.w) acc = fma((double)h.w, i3, acc);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const u64 v = (u64)__double_as_longlong(acc);
      const u64 y = ((u64)(u32)__shfl_xor((int)hi32(v), o) << 32) | (u32)__shfl_xor((int)(u32)v, o);
      acc += __longlong_as_double((long long)y);
    }
    if (lane == 0) bits[k] = acc;
  }
}

// ---- wide (16-bit) symbols: the counts and the ideal bits of a wide static model (rc_wide.h) ----

// k_histogram_wide: counts of 16-bit symbols below n_bins <= 4096.  Chunk-stride workgroups of 4
// waves like k_histogram; 16-B loads of 8 symbols with a symbol-wise head (0..7 symbols up to the
// first 16-B boundary: a chunk starts at any symbol) and tail around them.  One 16-KiB array of
// plain u32 LDS counters per workgroup (8 workgroups, 32 waves, per CU: §9.2's finding is that
// the rate follows the resident waves), shared by its four waves and split into 2^cshift copies
// of every bin: counter word = (bin << cshift) + (lane & (copies - 1)), so the copies of one bin
// lie in neighbouring banks and the lanes of one ds_add that hit one bin spread over them.  The
// host picks the copies from n_bins (hw_copy_shift): as many as fit, at most 32 (an LDS atomic is
// served in two groups of 32 lanes, and only the lanes of one group conflict), one at 4096 bins.
// A symbol >= n_bins touches no counter: it is counted by ballot into a count per wave.
//
// ROWS = false (batch only): the counters persist across the workgroup's chunks and are read out
// only at a flush, so no chunk pays a readout of n_bins counters.  ROWS = true: read out and
// cleared per chunk; at n_bins = 4096 that readout (16 bins per thread and two barriers) is the
// same order of work as counting a 16-Ki-symbol chunk (64 symbols per thread), which is inherent
// to asking for rows.  Either way at most 2^32 - 1 symbols are counted between two flushes into
// the u64 results, so no u32 counter wraps whatever the data (as k_histogram_order1).
#ifndef HW_WORDS             // (scratch builds: -DHW_WORDS=8192u)
#define HW_WORDS 4096u       // counter words per workgroup (16 KiB)
#endif
#define HW_SEG (1ull << 27)  // 16-B blocks (2^30 symbols) of a chunk between two looks at the budget

static inline u32 hw_copy_shift(u32 n_bins) {  // log2 of the copies: the most that fit, <= 32
  u32 s = 0;
  while (s < 5 && ((u64)n_bins << (s + 1)) <= HW_WORDS) ++s;
  return s;
}

template <bool ROWS>
__global__ __launch_bounds__(256) void k_histogram_wide(
    const uint16_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_chunks, u32 n_bins,
    u32 cshift, u32* __restrict__ chunk_hist, u64* __restrict__ hist, u64* __restrict__ oob) {
  __shared__ u32 sh[HW_WORDS];
  const u32 tid = threadIdx.x, lane = tid & 63;
  const u32 cmask = (1u << cshift) - 1u, copy = lane & cmask;
  RC_VGPR_FLOOR_64();
  for (u32 j = tid; j < HW_WORDS; j += 256) sh[j] = 0;
  // symbols >= n_bins seen by this wave since the last flush.  Added to from ballots inside
  // divergent code, so only a lane that took part in every ballot holds the wave's count: lane 0
  // does (the head, the tail and the block loop give the work to the lowest threads first).
  u32 oobc = 0;
  u32 acc[16];  // ROWS: bins tid + 256 j over this workgroup's chunks since the last flush
#pragma unroll
  for (u32 j = 0; j < 16; ++j) acc[j] = 0;
  auto count = [&](u32 s) {
    const bool in = s < n_bins;
    oobc += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(!in));
    if (in) hl_add((hl_u32*)(sh + (s << cshift) + copy), 1u);
  };
  // the sum of bin's copies, cleared (a thread reads out bins tid + 256 j only; the rotation
  // spreads the 32 lanes of a read over the banks)
  auto take = [&](u32 bin) {
    u32 v = 0;
#pragma unroll 1
    for (u32 c = 0; c <= cmask; ++c) {
      u32* w = sh + (bin << cshift) + ((c + tid) & cmask);
      v += *w;
      *w = 0;
    }
    return v;
  };
  // into the u64 results: acc (rows) or the counters (batch only), and the out-of-range count
  auto flush = [&]() {
    if (ROWS) {
      u32 t = tid;  // (opaque, as at the readout below)
      asm volatile("" : "+v"(t));
#pragma unroll
      for (u32 j = 0; j < 16; ++j) {
        if (hist && acc[j])
          atomicAdd(reinterpret_cast<unsigned long long*>(hist + t + 256 * j),
                    (unsigned long long)acc[j]);
        acc[j] = 0;
      }
    } else {
      __syncthreads();
#pragma unroll 1
      for (u32 bin = tid; bin < n_bins; bin += 256) {
        const u32 v = take(bin);
        if (hist && v)
          atomicAdd(reinterpret_cast<unsigned long long*>(hist + bin), (unsigned long long)v);
      }
    }
    if (oob && lane == 0 && oobc)
      atomicAdd(reinterpret_cast<unsigned long long*>(oob), (unsigned long long)oobc);
    oobc = 0;
    if (!ROWS) __syncthreads();
  };
  u64 pending = 0;  // symbols counted since the last flush (workgroup-uniform)
  __syncthreads();
  for (u32 k = blockIdx.x; k < n_chunks; k += gridDim.x) {
    const u64 s0 = sym_off[k], n = sym_off[k + 1] - s0;
    const uint16_t* p = syms + s0;
    u64 head = ((16 - ((uintptr_t)p & 15)) & 15) >> 1;
    if (head > n) head = n;
    const u64 nv = (n - head) >> 3, t0 = head + (nv << 3);
    const u32x4* v = reinterpret_cast<const u32x4*>(p + head);
    for (u64 b0 = 0; b0 == 0 || b0 < nv; b0 += HW_SEG) {
      const u64 b1 = nv - b0 < HW_SEG ? nv : b0 + HW_SEG;
      const u64 ns = ((b1 - b0) << 3) + (b0 == 0 ? n - (nv << 3) : 0);
      if (pending + ns > 0xFFFFFFFFull) {
        flush();
        pending = 0;
      }
      pending += ns;
      if (b0 == 0) {
        if (tid < head) count(p[tid]);
        if (t0 + tid < n) count(p[t0 + tid]);  // < 8 tail symbols
      }
#pragma unroll 2
      for (u64 i = b0 + tid; i < b1; i += 256) {
        const u32x4 w = gload16(v + i);
        const u32 ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          count(ws[q] & 0xFFFFu);
          count(ws[q] >> 16);
        }
      }
      if (ROWS) {  // this segment's counts into the chunk's row (u32) and into acc
        __syncthreads();
        u32* row = chunk_hist + (u64)k * n_bins;
        // (opaque: from tid itself the compiler keeps sixteen bins' worth of addresses in
        // registers across the chunk loop, 144 VGPRs in all)
        u32 t = tid;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (u32 j = 0; j < 16; ++j) {
          const u32 bin = t + 256 * j;
          if (bin < n_bins) {
            const u32 c = take(bin);
            row[bin] = b0 == 0 ? c : row[bin] + c;
            acc[j] += c;
          }
          // one bin at a time: sixteen readouts in flight at once cost the registers of two
          // resident waves
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
      }
    }
  }
  flush();
}

// k_ideal_bits_wide: per chunk the sum of icl[s] over its symbols, straight from the symbols: no
// histogram and no atomics.  icl[0 .. n]: the table's ideal code lengths in f64, +inf where
// c == 0, and entry n = +inf, which every symbol >= n is clamped to; it is staged in LDS once per
// workgroup (8 (n + 1) bytes, at most 32 KiB + 8 B).  One wave per chunk, waves striding over the
// chunks; a lane gathers the icl of its symbols (16-B loads of 8, head and tail as above) into a
// private f64 sum and a butterfly adds the 64 sums.  Every term is >= 0 or +inf (there is no
// 0 * inf), so a chunk is +inf or finite, never NaN.  Accuracy: with P = 64 partial sums of at
// most ceil(n_k / P) + 1 terms each and log2 P butterfly steps, the relative error of a finite
// chunk of n_k symbols is at most about (n_k / P + log2 P + 1) * 2^-53.
__global__ __launch_bounds__(HWG) void k_ideal_bits_wide(
    const double* __restrict__ icl, u32 n_symbols, const uint16_t* __restrict__ syms,
    const u64* __restrict__ sym_off, u32 n_chunks, double* __restrict__ bits) {
  extern __shared__ double s_icl[];
  const u32 lane = threadIdx.x & 63;
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  RC_VGPR_FLOOR_64();
  for (u32 j = threadIdx.x; j <= n_symbols; j += HWG) s_icl[j] = icl[j];
  __syncthreads();
  const u32 nw = gridDim.x * (HWG / 64);
  for (u32 k = blockIdx.x * (HWG / 64) + wave; k < n_chunks; k += nw) {
    const u64 s0 = sym_off[k], n = sym_off[k + 1] - s0;
    const uint16_t* p = syms + s0;
    u64 head = ((16 - ((uintptr_t)p & 15)) & 15) >> 1;
    if (head > n) head = n;
    const u64 nv = (n - head) >> 3, t0 = head + (nv << 3);
    const u32x4* v = reinterpret_cast<const u32x4*>(p + head);
    double acc = 0.0;
    if (lane < head) acc += s_icl[min((u32)p[lane], n_symbols)];
    if (t0 + lane < n) acc += s_icl[min((u32)p[t0 + lane], n_symbols)];
#pragma unroll 2
    for (u64 i = lane; i < nv; i += 64) {
      const u32x4 w = gload16(v + i);
      const u32 ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc += s_icl[min(ws[q] & 0xFFFFu, n_symbols)];
        acc += s_icl[min(ws[q] >> 16, n_symbols)];
      }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const u64 x = (u64)__double_as_longlong(acc);
      const u64 y = ((u64)(u32)__shfl_xor((int)hi32(x), o) << 32) | (u32)__shfl_xor((int)(u32)x, o);
      acc += __longlong_as_double((long long)y);
    }
    if (lane == 0) bits[k] = acc;
  }
}

// ---- rc_cluster_contexts_dev: the greedy clustering of rc_cluster_contexts on the device, over
// the I = 256 P + 1 items (phase, context) and "start of chunk"  ----
//
// Buffers (one hipMallocAsync): V, a private copy of the count rows (I x 256 u64; merges add row
// b into row a here); per slot cost (f64), tot (u64), live (u32); the delta table D (I x I f64,
// entries [a][b] with a < b; a dead column holds +inf, a dead row is never read); per row the
// smallest entry and its column (rmin, rarg: the lexicographically smallest (delta, b)); the
// merge log.  A stream-ordered chain of kernels, none of which waits for another workgroup:
//   k_cj_init     one wave per item: the copy, the total (exact, as total >> 32 and its low 32
//                 bits), the cost, live, and the bad-symbol flag.  The host reads the totals back,
//                 validates and fixes the number of merges: live items - max_models.
//   k_cj_pairs    the delta of every live pair: a wave holds row a in registers and walks 64 b.
//   k_cj_rowmin   one wave per row: rmin, rarg.
//   k_cj_merge    (one workgroup, per merge) rescans the row of the slot merged last, takes the
//                 arg-min of (rmin, a) over the live rows, merges b into a (row, total, the merged
//                 row's cost as cj_cost sums it, live[b] = 0, the log entry).
//   k_cj_refresh  (one wave per live slot x, per merge) delta(x, a) into D, +inf into column b,
//                 and row x's minimum: compared with the new entry, or rescanned when its arg-min
//                 was a or b.  Row a's own minimum is left to the next k_cj_merge, because its
//                 entries are written by many workgroups.
// The delta: cost(a + b) - (cost(a) + cost(b)), cost(v) = sum over t = v_s > 0 of
// t * log2(n / t), n the integer sum.  A lane adds the terms of symbols 4 L .. 4 L + 3 in that
// order and a butterfly adds the 64 sums, the same in every kernel, without contraction: a delta
// is a pure function of the two rows and the two costs, symmetric in a and b, and the cost of a
// merged row equals the cost(a + b) its delta was computed from.  Every term is >= 0.
#define CJ_NONE 0xFFFFFFFFu

static __device__ __forceinline__ double cj_cost(const u64 t[4], u64 n) {
#pragma clang fp contract(off)
  const double dn = (double)n;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (t[j]) acc += (double)t[j] * log2(dn / (double)t[j]);
#pragma unroll
  for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// the lexicographically smaller of (d, i) and the same of lane ^ o, over the wave
static __device__ __forceinline__ void cj_wave_min(double& d, u32& i) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double d2 = __shfl_xor(d, o);
    const u32 i2 = (u32)__shfl_xor((int)i, o);
    if (d2 < d || (d2 == d && i2 < i)) {
      d = d2;
      i = i2;
    }
  }
}

static __device__ __forceinline__ void cj_load4(const u64* row, u32 lane, u64 v[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = row[4 * lane + j];
}

__global__ __launch_bounds__(256) void k_cj_init(
    const u64* __restrict__ pair, const u64* __restrict__ first, u32 I, u32 n_symbols,
    u64* __restrict__ V, u64* __restrict__ tot, u64* __restrict__ tot_hi,
    double* __restrict__ cost, u32* __restrict__ live, u32* __restrict__ hdr) {
  const u32 lane = threadIdx.x & 63;
  const u32 item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= I) return;
  const bool ctx_item = item + 1 < I;
  u64 v[4];
  cj_load4(ctx_item ? pair + (size_t)item * 256 : first, lane, v);
  bool bad = false;
  u64 hs = 0, ls = 0;  // sums of the high and the low halves: each below 2^40 over the row
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bad |= v[j] && (4 * lane + j >= n_symbols || (ctx_item && (item & 255u) >= n_symbols));
    hs += v[j] >> 32;
    ls += v[j] & 0xFFFFFFFFull;
    V[(size_t)item * 256 + 4 * lane + j] = v[j];
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    hs += __shfl_xor((unsigned long long)hs, o);
    ls += __shfl_xor((unsigned long long)ls, o);
  }
  const u64 hi = hs + (ls >> 32);  // total >> 32, exact
  const u64 t = (hi << 32) | (ls & 0xFFFFFFFFull);
  const double c = t ? cj_cost(v, t) : 0.0;  // (wave-uniform)
  const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
  if (lane == 0) {
    tot[item] = t;
    tot_hi[item] = hi;
    cost[item] = c;
    live[item] = t != 0;
    if (anybad) atomicOr(hdr, 1u);
  }
}

__global__ __launch_bounds__(256) void k_cj_pairs(
    u32 I, const u64* __restrict__ V, const u64* __restrict__ tot,
    const double* __restrict__ cost, const u32* __restrict__ live, double* __restrict__ D) {
  const u32 lane = threadIdx.x & 63;
  const u32 a = blockIdx.x;
  const u32 base = blockIdx.y * 256 + (threadIdx.x >> 6) * 64;  // this wave's b: base .. base + 63
  if (a >= I || base + 63 <= a) return;
  double mine = INFINITY;
  if (live[a]) {
    u64 va[4];
    cj_load4(V + (size_t)a * 256, lane, va);
    const double ca = cost[a];
    const u64 ta = tot[a];
    for (u32 j = 0; j < 64; ++j) {
      const u32 b = base + j;
      if (b <= a || b >= I || !live[b]) continue;  // (wave-uniform)
      u64 t[4];
      cj_load4(V + (size_t)b * 256, lane, t);
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] += va[q];
      const double d = cj_cost(t, ta + tot[b]) - (ca + cost[b]);
      if (lane == j) mine = d;
    }
  }
  const u32 b = base + lane;
  if (b > a && b < I) D[(size_t)a * I + b] = mine;
}

// row x's smallest entry over the columns b > x, (delta, b) lexicographically; column oa reads as
// da and column ob as +inf whatever D holds (the entries this wave has just written)
static __device__ __forceinline__ void cj_scan_row(const double* __restrict__ D, u32 I, u32 x,
                                                   u32 lane, u32 oa, double da, u32 ob, double& d,
                                                   u32& i) {
  d = INFINITY;
  i = CJ_NONE;
  for (u32 b = x + 1 + lane; b < I; b += 64) {
    const double v = b == oa ? da : b == ob ? INFINITY : D[(size_t)x * I + b];
    if (v < d) {
      d = v;
      i = b;
    }
  }
  cj_wave_min(d, i);
}

__global__ __launch_bounds__(256) void k_cj_rowmin(u32 I, const double* __restrict__ D,
                                                   const u32* __restrict__ live,
                                                   double* __restrict__ rmin,
                                                   u32* __restrict__ rarg) {
  const u32 lane = threadIdx.x & 63;
  const u32 x = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (x >= I) return;
  double d = INFINITY;
  u32 i = CJ_NONE;
  if (live[x]) cj_scan_row(D, I, x, lane, CJ_NONE, 0.0, CJ_NONE, d, i);
  if (lane == 0) {
    rmin[x] = d;
    rarg[x] = i;
  }
}

// hdr[2], hdr[3]: a + 1 and b + 1 of the last merge (0: none yet, or none found)
__global__ __launch_bounds__(1024) void k_cj_merge(
    u32 I, u32 m, double* __restrict__ D, u64* __restrict__ V, u64* __restrict__ tot,
    double* __restrict__ cost, u32* __restrict__ live, double* __restrict__ rmin,
    u32* __restrict__ rarg, u32* __restrict__ hdr, u32* __restrict__ log) {
  __shared__ double s_d[16];
  __shared__ u32 s_i[16];
  __shared__ double s_rd;
  __shared__ u32 s_ri;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's lexicographically smallest (d, i), into s_rd, s_ri
  auto reduce = [&](double d, u32 i) {
    cj_wave_min(d, i);
    __syncthreads();
    if (lane == 0) {
      s_d[wave] = d;
      s_i[wave] = i;
    }
    __syncthreads();
    if (wave == 0) {
      d = lane < 16 ? s_d[lane] : INFINITY;
      i = lane < 16 ? s_i[lane] : CJ_NONE;
      cj_wave_min(d, i);
      if (lane == 0) {
        s_rd = d;
        s_ri = i;
      }
    }
    __syncthreads();
  };
  const u32 prev = hdr[2] - 1u;  // the slot merged last: its row of D is new
  double pd = INFINITY;
  u32 pb = CJ_NONE;
  if (prev < I) {
    double d = INFINITY;
    u32 i = CJ_NONE;
    for (u32 b = prev + 1 + tid; b < I; b += 1024) {
      const double v = D[(size_t)prev * I + b];
      if (v < d) {
        d = v;
        i = b;
      }
    }
    reduce(d, i);
    pd = s_rd;
    pb = s_ri;
    if (tid == 0) {
      rmin[prev] = pd;
      rarg[prev] = pb;
    }
  }
  double d = INFINITY;
  u32 i = CJ_NONE;
  for (u32 r = tid; r < I; r += 1024) {
    if (!live[r]) continue;
    const double v = r == prev ? pd : rmin[r];
    if (v < d) {
      d = v;
      i = r;
    }
  }
  reduce(d, i);
  const u32 a = s_ri;
  const u32 b = a < I ? (a == prev ? pb : rarg[a]) : CJ_NONE;
  if (wave != 0) return;
  if (a >= I || b >= I || b <= a) {  // no live pair: nothing is merged (the host sees the log)
    if (lane == 0) {
      log[2 * m] = CJ_NONE;
      log[2 * m + 1] = CJ_NONE;
      hdr[2] = 0;
      hdr[3] = 0;
    }
    return;
  }
  u64 t[4], vb[4];
  cj_load4(V + (size_t)a * 256, lane, t);
  cj_load4(V + (size_t)b * 256, lane, vb);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    t[q] += vb[q];
    V[(size_t)a * 256 + 4 * lane + q] = t[q];
  }
  const u64 n = tot[a] + tot[b];
  const double c = cj_cost(t, n);
  if (lane == 0) {
    tot[a] = n;
    cost[a] = c;
    live[b] = 0;
    log[2 * m] = a;
    log[2 * m + 1] = b;
    hdr[2] = a + 1;
    hdr[3] = b + 1;
    D[(size_t)a * I + b] = INFINITY;  // column b is dead in row a too (no wave refreshes x = b)
  }
}

__global__ __launch_bounds__(256) void k_cj_refresh(
    u32 I, const u64* __restrict__ V, const u64* __restrict__ tot,
    const double* __restrict__ cost, const u32* __restrict__ live, double* __restrict__ D,
    double* __restrict__ rmin, u32* __restrict__ rarg, const u32* __restrict__ hdr) {
  const u32 lane = threadIdx.x & 63;
  const u32 x = blockIdx.x * 4 + (threadIdx.x >> 6);
  const u32 a = hdr[2] - 1u, b = hdr[3] - 1u;
  if (a >= I || b >= I || x >= I || x == a || !live[x]) return;  // (b is no longer live)
  u64 t[4], vx[4];
  cj_load4(V + (size_t)a * 256, lane, t);
  cj_load4(V + (size_t)x * 256, lane, vx);
#pragma unroll
  for (int q = 0; q < 4; ++q) t[q] += vx[q];
  const double d = cj_cost(t, tot[a] + tot[x]) - (cost[a] + cost[x]);
  const u32 r = rarg[x];
  if (x > a) {
    if (lane == 0) D[(size_t)a * I + x] = d;
    if (x < b) {
      if (lane == 0) D[(size_t)x * I + b] = INFINITY;
      if (r == b) {
        double nd;
        u32 ni;
        cj_scan_row(D, I, x, lane, CJ_NONE, 0.0, b, nd, ni);
        if (lane == 0) {
          rmin[x] = nd;
          rarg[x] = ni;
        }
      }
    }
    return;
  }
  if (lane == 0) {
    D[(size_t)x * I + a] = d;
    D[(size_t)x * I + b] = INFINITY;
  }
  if (r == a || r == b) {
    double nd;
    u32 ni;
    cj_scan_row(D, I, x, lane, a, d, b, nd, ni);
    if (lane == 0) {
      rmin[x] = nd;
      rarg[x] = ni;
    }
  } else if (lane == 0) {
    const double old = rmin[x];
    if (d < old || (d == old && a < r)) {
      rmin[x] = d;
      rarg[x] = a;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
// rc_histogram_pairs (PER = false, period 1), rc_histogram_pairs_periodic (PER = true, period 1
// included) and rc_histogram_pairs_lagged (one kernel per lag): each call keeps its own
// instantiation of the kernel
template <class Kern>
static rc_status histogram_pairs_launch(Kern kern, rc_ctx* ctx, u32 period, const uint8_t* syms,
                                        const uint64_t* sym_off, uint32_t n_chunks,
                                        uint64_t* pair_hist, uint64_t* first_hist) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (period != 1 && period != 2 && period != 4 && period != 8) return RC_E_ARG;
  if (n_chunks == 0 || (!pair_hist && !first_hist)) return RC_OK;
  if (!syms || !sym_off) return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return RC_E_DEVICE;
  if (set_allow_lds(reinterpret_cast<const void*>(kern)) != hipSuccess) return RC_E_DEVICE;
  // as many workgroups as the CUs hold (their LDS and 32 waves each), in O1P_SLICES * P groups
  // that stride over the chunks side by side
  const u32 slices = O1P_SLICES * period;
  const u32 per_cu = std::max(1u, std::min(163840u / O1P_LDS, 2048u / O1P_WG));
  const u32 groups =
      std::max(1u, std::min<u32>((n_chunks + O1P_Q - 1) / O1P_Q, (u32)cus * per_cu / slices));
  hipLaunchKernelGGL(kern, dim3(groups * slices), dim3(O1P_WG), O1P_LDS, s, syms, sym_off,
                     n_chunks, pair_hist, first_hist, period);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}
template <bool PER>
static rc_status histogram_pairs(rc_ctx* ctx, u32 period, const uint8_t* syms,
                                 const uint64_t* sym_off, uint32_t n_chunks, uint64_t* pair_hist,
                                 uint64_t* first_hist) {
  return histogram_pairs_launch(k_histogram_pairs<PER>, ctx, period, syms, sym_off, n_chunks,
                                pair_hist, first_hist);
}

extern "C" {

rc_status rc_histogram(rc_ctx* ctx, const uint8_t* syms, const uint64_t* sym_off,
                       uint32_t n_chunks, uint32_t* chunk_hist, uint64_t* hist) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_chunks == 0 || (!chunk_hist && !hist)) return RC_OK;
  if (!syms || !sym_off) return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return RC_E_DEVICE;
  // 16 KiB LDS per workgroup: 8 workgroups (32 waves) per CU
  const u32 grid = std::min<u32>(n_chunks, (u32)cus * 8);
  // RC_HIST_HOT=0 (in the environment of rc_ctx_create) turns the ballot-counted hot symbol
  // off (measurements)
  hipLaunchKernelGGL(k_histogram, dim3(grid), dim3(256), 0, s, syms, sym_off, n_chunks,
                     chunk_hist, hist, (u32)ctx->knobs.hist_hot);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}

rc_status rc_histogram_order1(rc_ctx* ctx, uint32_t n_models, const uint8_t* ctx_map_host,
                              uint32_t first_row, const uint8_t* syms, const uint64_t* sym_off,
                              uint32_t n_chunks, uint64_t* hist) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS || !ctx_map_host || n_models < 1 ||
      n_models > RC_MAX_SET_MODELS || first_row >= n_models)
    return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  O1HistMap map;
  for (u32 i = 0; i < 256; ++i)
    if (ctx_map_host[i] >= n_models) return RC_E_ARG;
  memcpy(map.w, ctx_map_host, 256);
  if (n_chunks == 0) return RC_OK;
  if (!syms || !sym_off || !hist) return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return RC_E_DEVICE;
  // K KiB of counters and the map per workgroup (just over the default 64-KiB limit of dynamic
  // LDS at K = 64); up to 8 workgroups (32 waves) per CU
  const u32 lds = n_models * 1024u + 256u;
  if (set_allow_lds(reinterpret_cast<const void*>(k_histogram_order1)) != hipSuccess)
    return RC_E_DEVICE;
  const u32 per_cu = std::max(1u, std::min(8u, 163840u / lds));
  const u32 grid = std::min<u32>(n_chunks, (u32)cus * per_cu);
  hipLaunchKernelGGL(k_histogram_order1, dim3(grid), dim3(256), lds, s, map, first_row, n_models,
                     syms, sym_off, n_chunks, hist);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}

rc_status rc_histogram_pairs(rc_ctx* ctx, const uint8_t* syms, const uint64_t* sym_off,
                             uint32_t n_chunks, uint64_t* pair_hist, uint64_t* first_hist) {
  return histogram_pairs<false>(ctx, 1, syms, sym_off, n_chunks, pair_hist, first_hist);
}

rc_status rc_histogram_pairs_periodic(rc_ctx* ctx, uint32_t period, const uint8_t* syms,
                                      const uint64_t* sym_off, uint32_t n_chunks,
                                      uint64_t* pair_hist, uint64_t* first_hist) {
  return histogram_pairs<true>(ctx, period, syms, sym_off, n_chunks, pair_hist, first_hist);
}

rc_status rc_histogram_pairs_lagged(rc_ctx* ctx, uint32_t period, uint32_t lag,
                                    const uint8_t* syms, const uint64_t* sym_off,
                                    uint32_t n_chunks, uint64_t* pair_hist, uint64_t* first_hist) {
  switch (lag) {
    case 1:
      return rc_histogram_pairs_periodic(ctx, period, syms, sym_off, n_chunks, pair_hist,
                                         first_hist);
    case 2:
      return histogram_pairs_launch(k_histogram_pairs_lag<2>, ctx, period, syms, sym_off, n_chunks,
                                    pair_hist, first_hist);
    case 4:
      return histogram_pairs_launch(k_histogram_pairs_lag<4>, ctx, period, syms, sym_off, n_chunks,
                                    pair_hist, first_hist);
    case 8:
      return histogram_pairs_launch(k_histogram_pairs_lag<8>, ctx, period, syms, sym_off, n_chunks,
                                    pair_hist, first_hist);
  }
  return RC_E_ARG;
}

rc_status rc_ideal_bits_order1(rc_ctx* ctx, const rc_model* o1, const uint8_t* syms,
                               const uint64_t* sym_off, uint32_t n_chunks, double* bits) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (!rc_model_kind_ok(o1, 1u << RC_KIND_ORDER1)) return RC_E_ARG;  // kinds do not mix
  if (o1->device != dev) return RC_E_ARG;
  // the set's cum rows ([K][257]) and its staged map (`period` slices of 256), device memory
  const u32* const rows_dev = o1->o1.s.rows;
  const uint8_t* const map_dev = o1->o1.map;
  const u32 first_row = o1->o1.first_row, K = o1->o1.s.k;
  if (n_chunks == 0) return RC_OK;
  if (!syms || !sym_off || !bits) return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  // the set keeps its tables on the device only (K cum rows cum[0 .. 256], the entries from n on
  // holding the total): read them back, then PModel::ideal_code_length (pmodel.rs:14-40) per row
  // and symbol exactly as rc_ideal_bits computes it, +inf for c == 0, which covers the symbols
  // from n on.  Pinned staging: the rows, then the table, 8-B aligned.
  const size_t rows_words = (size_t)K * 257u;
  const size_t rows_bytes = (rows_words * sizeof(u32) + 7) & ~(size_t)7;
  const size_t icl_bytes = (size_t)K * 256u * sizeof(double);
  char* pin = (char*)rc_pinned_scratch_(rows_bytes + icl_bytes);
  if (!pin) return RC_E_DEVICE;
  if (hipMemcpyAsync(pin, rows_dev, rows_words * sizeof(u32), hipMemcpyDeviceToHost, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return RC_E_DEVICE;
  const u32* cum = (const u32*)pin;
  double* icl = (double*)(pin + rows_bytes);
  for (u32 j = 0; j < K; ++j) {
    const u32* r = cum + (size_t)j * 257u;
    const double lt = log((double)r[256]);
    for (u32 i = 0; i < 256; ++i) {
      const u32 c = r[i + 1] - r[i];
      icl[(size_t)j * 256u + i] = c > 0 ? (lt - log((double)c)) / M_LN2 : INFINITY;
    }
  }
  double* d = nullptr;
  if (hipMallocAsync((void**)&d, icl_bytes, s) != hipSuccess) return RC_E_DEVICE;
  const u32 period = o1->o1.period;  // (> 1: map_dev holds `period` slices)
  const u32 lag = o1->o1_lag;  // (> 1: the kernel of that lag, whatever the period)
  const auto kern = lag == 2   ? k_ideal_bits_order1_lag<2>
                    : lag == 4 ? k_ideal_bits_order1_lag<4>
                    : lag == 8 ? k_ideal_bits_order1_lag<8>
                    : period > 1 ? k_ideal_bits_order1<true>
                                 : k_ideal_bits_order1<false>;
  if (hipMemcpyAsync(d, icl, icl_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
      set_allow_lds(reinterpret_cast<const void*>(kern)) != hipSuccess) {
    (void)hipFreeAsync(d, s);
    return RC_E_DEVICE;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  // the table's LDS bounds the workgroups per CU (one at K = 64, 8 at most); the workgroup's
  // size keeps at least 16 waves on the CU: 1024 lanes where one fits, 512 where two or three
  // do, else 256 (16 to 32 waves)
  const u32 lds = (u32)icl_bytes + 256u * period;
  const u32 per_cu = std::max(1u, std::min(8u, 163840u / lds));
  const u32 wg = per_cu == 1 ? 1024u : per_cu < 4 ? 512u : 256u;
  const u32 grid = std::min<u32>((n_chunks + wg / 64 - 1) / (wg / 64), (u32)cus * per_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(wg), lds, s, d, map_dev, first_row, K, syms, sym_off,
                     n_chunks, bits, period);
  const bool ok = hipGetLastError() == hipSuccess;
  // the pinned staging is reused by this thread's next call: wait for the copy
  const bool fr = hipFreeAsync(d, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  return ok && fr ? RC_OK : RC_E_DEVICE;
}

rc_status rc_histogram_wide(rc_ctx* ctx, const void* syms, const uint64_t* sym_off,
                            uint32_t n_chunks, uint32_t n_bins, uint32_t* chunk_hist,
                            uint64_t* hist, uint64_t* oob) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS || n_bins < 1 || n_bins > RC_MAX_WIDE_SYMBOLS ||
      ((uintptr_t)syms & 1u) != 0)
    return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_chunks == 0 || (!chunk_hist && !hist && !oob)) return RC_OK;
  if (!syms || !sym_off) return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return RC_E_DEVICE;
  // 16 KiB LDS per workgroup: 8 workgroups (32 waves) per CU
  const u32 grid = std::min<u32>(n_chunks, (u32)cus * std::min(8u, 163840u / (4u * HW_WORDS)));
  const u32 cshift = hw_copy_shift(n_bins);
  if (chunk_hist)
    hipLaunchKernelGGL(k_histogram_wide<true>, dim3(grid), dim3(256), 0, s,
                       (const uint16_t*)syms, sym_off, n_chunks, n_bins, cshift, chunk_hist, hist,
                       oob);
  else
    hipLaunchKernelGGL(k_histogram_wide<false>, dim3(grid), dim3(256), 0, s,
                       (const uint16_t*)syms, sym_off, n_chunks, n_bins, cshift, chunk_hist, hist,
                       oob);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}

// Internal test hook (not in include/range_coder.h; host only): the copies of every bin that
// k_histogram_wide keeps for n_bins bins (0 for an n_bins rc_histogram_wide refuses).
uint32_t rc_histogram_wide_copies_(uint32_t n_bins) {
  return n_bins < 1 || n_bins > RC_MAX_WIDE_SYMBOLS ? 0u : 1u << hw_copy_shift(n_bins);
}

rc_status rc_ideal_bits_wide(rc_ctx* ctx, const rc_model* wide, const void* syms,
                             const uint64_t* sym_off, uint32_t n_chunks, double* bits) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (!rc_model_kind_ok(wide, 1u << RC_KIND_WIDE)) return RC_E_ARG;  // kinds do not mix
  if (((uintptr_t)syms & 1u) != 0) return RC_E_ARG;  // 16-bit symbols
  if (n_chunks == 0) return RC_OK;
  if (!syms || !sym_off || !bits || wide->device != dev) return RC_E_ARG;
  const u32* const row_dev = wide->wide.row;
  const u32 n = wide->wide.m.n;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  // the model keeps its table on the device only (the cum row cum[0 .. n], cum[n] = total): read
  // it back, then PModel::ideal_code_length (pmodel.rs:14-40) per symbol exactly as
  // rc_ideal_bits computes it, +inf for c == 0 and for the entry symbols >= n are clamped to.
  // Pinned staging: the row, then the table, 8-B aligned.
  const size_t row_bytes = (((size_t)n + 1) * sizeof(u32) + 7) & ~(size_t)7;
  const size_t icl_bytes = ((size_t)n + 1) * sizeof(double);
  char* pin = (char*)rc_pinned_scratch_(row_bytes + icl_bytes);
  if (!pin) return RC_E_DEVICE;
  if (hipMemcpyAsync(pin, row_dev, ((size_t)n + 1) * sizeof(u32), hipMemcpyDeviceToHost, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return RC_E_DEVICE;
  const u32* cum = (const u32*)pin;
  double* icl = (double*)(pin + row_bytes);
  const double lt = log((double)cum[n]);
  for (u32 i = 0; i < n; ++i) {
    const u32 c = cum[i + 1] - cum[i];
    icl[i] = c > 0 ? (lt - log((double)c)) / M_LN2 : INFINITY;
  }
  icl[n] = INFINITY;
  double* d = nullptr;
  if (hipMallocAsync((void**)&d, icl_bytes, s) != hipSuccess) return RC_E_DEVICE;
  if (hipMemcpyAsync(d, icl, icl_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipFreeAsync(d, s);
    return RC_E_DEVICE;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  // one wave per chunk, waves striding over the chunks; the table's LDS bounds the workgroups
  // per CU (4 at 4096 symbols), 8 (32 waves) at most
  const u32 per_cu = std::max(1u, std::min(8u, 163840u / (u32)icl_bytes));
  const u32 grid = std::min<u32>((n_chunks + HWG / 64 - 1) / (HWG / 64), (u32)cus * per_cu);
  hipLaunchKernelGGL(k_ideal_bits_wide, dim3(grid), dim3(HWG), icl_bytes, s, d, n,
                     (const uint16_t*)syms, sym_off, n_chunks, bits);
  const bool ok = hipGetLastError() == hipSuccess;
  // the pinned staging is reused by this thread's next call: wait for the copy
  const bool fr = hipFreeAsync(d, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  return ok && fr ? RC_OK : RC_E_DEVICE;
}

}  // extern "C"

// rc_quantize_counts / rc_quantize_counts_wide / rc_quantize_counts_wide16 /
// rc_quantize_counts_wide16_fine: one rule, alphabets of up to max_symbols
static rc_status quantize_counts(const uint64_t* counts, uint32_t n_symbols, u32 max_symbols,
                                 uint64_t target_total, uint32_t qflags, uint32_t* c_out,
                                 uint32_t* cum_out, uint32_t* total_out) {
  if (!counts || !c_out || !cum_out || !total_out || n_symbols < 1 || n_symbols > max_symbols)
    return RC_E_ARG;
  const bool all = (qflags & RC_Q_ALL_SYMBOLS) != 0;
  std::vector<u64> c(n_symbols);
  unsigned __int128 N = 0;
  for (u32 i = 0; i < n_symbols; ++i) N += counts[i];
  if (target_total == 0) {  // exact FreqTable: c = counts, total = sum (sample_impl.rs:58-69)
    for (u32 i = 0; i < n_symbols; ++i) c[i] = counts[i] + ((all && counts[i] == 0) ? 1u : 0u);
  } else {
    u32 need = 0;
    for (u32 i = 0; i < n_symbols; ++i) need += (all || counts[i] > 0) ? 1u : 0u;
    if (N == 0) {
      if (!all) return RC_E_BAD_MODEL;  // nothing to model
      need = n_symbols;
    }
    if (target_total < need || target_total > 0xFFFFFFFFull) return RC_E_BAD_MODEL;
    // c_i = max(1, round(counts_i * T / N)) for modelled symbols (half rounds up)
    u64 sum = 0;
    for (u32 i = 0; i < n_symbols; ++i) {
      if (N == 0) {
        c[i] = 1;
      } else if (counts[i] == 0 && !all) {
        c[i] = 0;
      } else {
        const unsigned __int128 q = ((unsigned __int128)counts[i] * target_total + N / 2) / N;
        c[i] = q < 1 ? 1 : (u64)q;
      }
      sum += c[i];
    }
    // fold the difference: a deficit goes to the largest entry (lowest index on ties); an
    // excess is taken from the largest entries first, never below 1
    if (sum < target_total) {
      u32 m = 0;
      for (u32 i = 1; i < n_symbols; ++i)
        if (c[i] > c[m]) m = i;
      c[m] += target_total - sum;
    } else if (sum > target_total) {
      u64 excess = sum - target_total;
      std::vector<u32> order(n_symbols);
      for (u32 i = 0; i < n_symbols; ++i) order[i] = i;
      std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return c[a] > c[b]; });
      for (u32 j = 0; j < n_symbols && excess; ++j) {
        const u32 i = order[j];
        if (c[i] <= 1) break;
        const u64 take = std::min<u64>(excess, c[i] - 1);
        c[i] -= take;
        excess -= take;
      }
      if (excess) return RC_E_BAD_MODEL;  // unreachable: target >= number of entries
    }
  }
  u64 acc = 0;
  for (u32 i = 0; i < n_symbols; ++i) {
    cum_out[i] = (u32)acc;
    c_out[i] = (u32)c[i];
    acc += c[i];
    if (acc > 0xFFFFFFFFull) return RC_E_BAD_MODEL;  // calc_cum's u32 total would overflow
  }
  if (acc == 0) return RC_E_BAD_MODEL;
  *total_out = (u32)acc;
  return RC_OK;
}

extern "C" {

rc_status rc_quantize_counts(const uint64_t* counts, uint32_t n_symbols, uint64_t target_total,
                             uint32_t qflags, uint32_t* c_out, uint32_t* cum_out,
                             uint32_t* total_out) {
  return quantize_counts(counts, n_symbols, 256u, target_total, qflags, c_out, cum_out, total_out);
}

rc_status rc_quantize_counts_wide(const uint64_t* counts, uint32_t n_symbols,
                                  uint64_t target_total, uint32_t qflags, uint32_t* c_out,
                                  uint32_t* cum_out, uint32_t* total_out) {
  return quantize_counts(counts, n_symbols, RC_MAX_WIDE_SYMBOLS, target_total, qflags, c_out,
                         cum_out, total_out);
}

rc_status rc_quantize_counts_wide16(const uint64_t* counts, uint32_t n_symbols,
                                    uint64_t target_total, uint32_t qflags, uint32_t* c_out,
                                    uint32_t* cum_out, uint32_t* total_out) {
  // every symbol kept encodable needs a frequency of its own: no target below n can hold them
  if ((qflags & RC_Q_ALL_SYMBOLS) && target_total && n_symbols > target_total) return RC_E_ARG;
  return quantize_counts(counts, n_symbols, RC_MAX_WIDE16_SYMBOLS, target_total, qflags, c_out,
                         cum_out, total_out);
}

rc_status rc_quantize_counts_wide16_fine(const uint64_t* counts, uint32_t n_symbols,
                                         uint64_t target_total, uint32_t qflags, uint32_t* c_out,
                                         uint32_t* cum_out, uint32_t* total_out) {
  // the fine models' totals: above 2^16 (a smaller one is rc_quantize_counts_wide16's), at most 2^24
  if (target_total <= 65536u || target_total > RC_MAX_WIDE16_FINE_TOTAL) return RC_E_ARG;
  return quantize_counts(counts, n_symbols, RC_MAX_WIDE16_SYMBOLS, target_total, qflags, c_out,
                         cum_out, total_out);
}

// rc_cluster_contexts: greedy agglomerative clustering of the 256 contexts and the start-of-chunk
// pseudo-context under the empirical-entropy cost (include/range_coder.h).  A cluster lives in
// the slot of its smallest member, so scanning the slots in ascending order with a strict
// comparison is the tie-break.  The pairwise deltas are kept in a table and only the merged
// cluster's row is recomputed per merge: 256 log2 per pair, about 8 M for the start and 65 k per
// merge.
#define CC_ITEMS 257u

// cost(a + b); b may be null
static double cc_cost(const u64* a, const u64* b) {
  u64 n = 0;
  for (u32 s = 0; s < 256; ++s) n += a[s] + (b ? b[s] : 0);
  const double dn = (double)n;
  double c = 0.0;
  for (u32 s = 0; s < 256; ++s) {
    const u64 t = a[s] + (b ? b[s] : 0);
    if (t) c += (double)t * log2(dn / (double)t);
  }
  return c;
}

rc_status rc_cluster_contexts(const uint64_t* pair_hist, const uint64_t* first_hist,
                              uint32_t n_symbols, uint32_t max_models, uint8_t* ctx_map_out,
                              uint32_t* first_row_out, uint32_t* n_models_out,
                              double* cost_bits_out) {
  if (!pair_hist || !first_hist || !ctx_map_out || !first_row_out || !n_models_out ||
      max_models < 1 || max_models > RC_MAX_SET_MODELS || n_symbols < 1 || n_symbols > 256)
    return RC_E_ARG;
  auto item = [&](u32 a) { return a < 256 ? pair_hist + (size_t)a * 256 : first_hist; };
  unsigned __int128 all = 0;
  std::vector<u64> tot(CC_ITEMS, 0);  // samples per slot
  for (u32 a = 0; a < CC_ITEMS; ++a) {
    const u64* v = item(a);
    unsigned __int128 t = 0;
    for (u32 s = 0; s < 256; ++s) {
      if (v[s] && (s >= n_symbols || (a < 256 && a >= n_symbols))) return RC_E_BAD_SYMBOL;
      t += v[s];
    }
    all += t;
    if (all >> 63) return RC_E_ARG;
    tot[a] = (u64)t;
  }
  if (all == 0) return RC_E_BAD_MODEL;
  std::vector<u64> vec((size_t)CC_ITEMS * 256);
  std::vector<double> cost(CC_ITEMS, 0.0), delta((size_t)CC_ITEMS * CC_ITEMS, 0.0);
  std::vector<u32> slot(CC_ITEMS), live;  // slot: an item's cluster (CC_ITEMS: not clustered)
  for (u32 a = 0; a < CC_ITEMS; ++a) {
    memcpy(&vec[(size_t)a * 256], item(a), 256 * sizeof(u64));
    slot[a] = tot[a] ? a : CC_ITEMS;
    if (tot[a]) {
      live.push_back(a);
      cost[a] = cc_cost(&vec[(size_t)a * 256], nullptr);
    }
  }
  auto refresh = [&](u32 a, u32 b) {  // a < b, both live
    delta[(size_t)a * CC_ITEMS + b] =
        cc_cost(&vec[(size_t)a * 256], &vec[(size_t)b * 256]) - cost[a] - cost[b];
  };
  if (live.size() > max_models)
    for (size_t i = 0; i < live.size(); ++i)
      for (size_t j = i + 1; j < live.size(); ++j) refresh(live[i], live[j]);
  while (live.size() > max_models) {
    size_t bi = 0, bj = 1;
    double best = INFINITY;
    for (size_t i = 0; i < live.size(); ++i)
      for (size_t j = i + 1; j < live.size(); ++j) {
        const double d = delta[(size_t)live[i] * CC_ITEMS + live[j]];
        if (d < best) {
          best = d;
          bi = i;
          bj = j;
        }
      }
    const u32 a = live[bi], b = live[bj];
    // the merged cluster's cost, as cc_cost sums it
    cost[a] = cc_cost(&vec[(size_t)a * 256], &vec[(size_t)b * 256]);
    for (u32 s = 0; s < 256; ++s) vec[(size_t)a * 256 + s] += vec[(size_t)b * 256 + s];
    tot[a] += tot[b];
    for (u32 x = 0; x < CC_ITEMS; ++x)
      if (slot[x] == b) slot[x] = a;
    live.erase(live.begin() + (ptrdiff_t)bj);
    for (u32 x : live) {
      if (x < a) refresh(x, a);
      else if (x > a) refresh(a, x);
    }
  }
  // rows by ascending smallest member (live is ascending); the largest row, lowest on ties
  std::vector<u32> row(CC_ITEMS + 1, 0);
  u32 big = 0;
  double bits = 0.0;
  for (size_t i = 0; i < live.size(); ++i) {
    row[live[i]] = (u32)i;
    if (tot[live[i]] > tot[live[big]]) big = (u32)i;
    bits += cost[live[i]];
  }
  row[CC_ITEMS] = big;  // items without samples
  for (u32 p = 0; p < 256; ++p) ctx_map_out[p] = p < n_symbols ? (uint8_t)row[slot[p]] : 0;
  *first_row_out = row[slot[256]];
  *n_models_out = (u32)live.size();
  if (cost_bits_out) *cost_bits_out = bits;
  return RC_OK;
}

// rc_cluster_contexts_dev: rc_cluster_contexts' rule over the 256 P + 1 items of periodic pair
// counts, on the device where they lie (the k_cj_* kernels above).  Two waits: after k_cj_init
// (the totals: validation, and the number of merges, which the host fixes before it enqueues the
// loop) and at the end (the log and the costs).  The host replays the log into slots and rows.
rc_status rc_cluster_contexts_dev(rc_ctx* ctx, uint32_t period, const uint64_t* pair_hist,
                                  const uint64_t* first_hist, uint32_t n_symbols,
                                  uint32_t max_models, uint8_t* ctx_map_out,
                                  uint32_t* first_row_out, uint32_t* n_models_out,
                                  double* cost_bits_out) {
  if (!ctx) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (period != 1 && period != 2 && period != 4 && period != 8) return RC_E_ARG;
  if (!pair_hist || !first_hist || !ctx_map_out || !first_row_out || !n_models_out ||
      max_models < 1 || max_models > RC_MAX_SET_MODELS || n_symbols < 1 || n_symbols > 256)
    return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  const u32 I = 256u * period + 1u;
  // one allocation: D, V, cost, rmin, tot, tot_hi (8-byte entries), then live, rarg, log, hdr
  const size_t n8 = (size_t)I * I + (size_t)I * 256 + 5 * (size_t)I;
  const size_t n4 = 4 * (size_t)I + 4;
  // pinned staging: tot, tot_hi, cost (8-byte entries), then hdr and the log
  char* pin = (char*)rc_pinned_scratch_(3 * (size_t)I * 8 + 16 + 2 * (size_t)I * 4);
  if (!pin) return RC_E_DEVICE;
  char* buf = nullptr;
  if (hipMallocAsync((void**)&buf, n8 * 8 + n4 * 4, s) != hipSuccess) return RC_E_DEVICE;
  double* D = (double*)buf;
  u64* V = (u64*)(D + (size_t)I * I);
  double* cost = (double*)(V + (size_t)I * 256);
  double* rmin = cost + I;
  u64* tot = (u64*)(rmin + I);
  u64* tot_hi = tot + I;
  u32* live = (u32*)(tot_hi + I);
  u32* rarg = live + I;
  u32* log = rarg + I;
  u32* hdr = log + 2 * (size_t)I;
  u64* h_tot = (u64*)pin;
  u64* h_hi = h_tot + I;
  double* h_cost = (double*)(h_hi + I);
  u32* h_hdr = (u32*)(h_cost + I);
  u32* h_log = h_hdr + 4;
  auto done = [&](rc_status st) {
    const bool fr = hipFreeAsync(buf, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    return st == RC_OK && !fr ? RC_E_DEVICE : st;
  };
  const u32 waves4 = (I + 3) / 4;  // workgroups of four waves, one wave per item
  if (hipMemsetAsync(hdr, 0, 16, s) != hipSuccess) return done(RC_E_DEVICE);
  hipLaunchKernelGGL(k_cj_init, dim3(waves4), dim3(256), 0, s, pair_hist, first_hist, I, n_symbols,
                     V, tot, tot_hi, cost, live, hdr);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(h_tot, tot, 2 * (size_t)I * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(h_hdr, hdr, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return done(RC_E_DEVICE);
  if (h_hdr[0] & 1u) return done(RC_E_BAD_SYMBOL);
  unsigned __int128 all = 0;
  std::vector<u64> htot(I);
  std::vector<u32> slot(I), live_h;  // slot: an item's cluster (I: not clustered)
  for (u32 a = 0; a < I; ++a) {
    all += ((unsigned __int128)h_hi[a] << 32) | (h_tot[a] & 0xFFFFFFFFull);
    htot[a] = h_tot[a];
    slot[a] = h_tot[a] ? a : I;
    if (h_tot[a]) live_h.push_back(a);
  }
  if (all >> 63) return done(RC_E_ARG);
  if (all == 0) return done(RC_E_BAD_MODEL);
  const u32 merges = live_h.size() > max_models ? (u32)live_h.size() - max_models : 0u;
  if (merges) {
    hipLaunchKernelGGL(k_cj_pairs, dim3(I, (I + 255) / 256), dim3(256), 0, s, I, V, tot, cost,
                       live, D);
    hipLaunchKernelGGL(k_cj_rowmin, dim3(waves4), dim3(256), 0, s, I, D, live, rmin, rarg);
    for (u32 m = 0; m < merges; ++m) {
      hipLaunchKernelGGL(k_cj_merge, dim3(1), dim3(1024), 0, s, I, m, D, V, tot, cost, live, rmin,
                         rarg, hdr, log);
      if (m + 1 < merges)
        hipLaunchKernelGGL(k_cj_refresh, dim3(waves4), dim3(256), 0, s, I, V, tot, cost, live, D,
                           rmin, rarg, hdr);
    }
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h_log, log, 2 * (size_t)merges * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
      return done(RC_E_DEVICE);
  }
  if (hipMemcpyAsync(h_cost, cost, (size_t)I * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return done(RC_E_DEVICE);
  // replay the log: b's members join a's slot
  for (u32 m = 0; m < merges; ++m) {
    const u32 a = h_log[2 * m], b = h_log[2 * m + 1];
    if (a >= b || b >= I || slot[a] != a || slot[b] != b) return done(RC_E_DEVICE);
    htot[a] += htot[b];
    for (u32 x = 0; x < I; ++x)
      if (slot[x] == b) slot[x] = a;
    live_h.erase(std::find(live_h.begin(), live_h.end(), b));
  }
  // rows by ascending smallest member (live_h is ascending); the largest row, lowest on ties
  std::vector<u32> row(I + 1, 0);
  u32 big = 0;
  double bits = 0.0;
  for (size_t i = 0; i < live_h.size(); ++i) {
    row[live_h[i]] = (u32)i;
    if (htot[live_h[i]] > htot[live_h[big]]) big = (u32)i;
    bits += h_cost[live_h[i]];
  }
  row[I] = big;  // items without samples
  for (u32 x = 0; x + 1 < I; ++x)
    ctx_map_out[x] = (x & 255u) < n_symbols ? (uint8_t)row[slot[x]] : 0;
  *first_row_out = row[slot[I - 1]];
  *n_models_out = (u32)live_h.size();
  if (cost_bits_out) *cost_bits_out = bits;
  return done(RC_OK);
}

rc_status rc_ideal_bits(rc_ctx* ctx, const uint32_t* c_host, uint32_t n_symbols,
                        uint32_t total_freq, const uint32_t* chunk_hist, uint32_t n_chunks,
                        double* bits) {
  if (!ctx || !c_host || n_symbols < 1 || n_symbols > 256 || total_freq < 1 ||
      n_chunks > RC_MAX_CHUNKS)
    return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_chunks == 0) return RC_OK;
  if (!chunk_hist || !bits) return RC_E_ARG;
  // PModel::ideal_code_length (pmodel.rs:14-40): (ln total - ln c) / ln 2; symbols outside the
  // alphabet or with c == 0 have no code length (+inf here)
  double icl[256];
  const double lt = log((double)total_freq);
  for (u32 i = 0; i < 256; ++i)
    icl[i] = (i < n_symbols && c_host[i] > 0) ? (lt - log((double)c_host[i])) / M_LN2 : INFINITY;
  DeviceGuard g(dev);
  double* d = nullptr;
  if (hipMallocAsync((void**)&d, sizeof icl, s) != hipSuccess) return RC_E_DEVICE;
  void* pin = rc_pinned_scratch_(sizeof icl);
  if (!pin) {
    (void)hipFreeAsync(d, s);
    return RC_E_DEVICE;
  }
  memcpy(pin, icl, sizeof icl);
  if (hipMemcpyAsync(d, pin, sizeof icl, hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipFreeAsync(d, s);
    return RC_E_DEVICE;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  // one wave per chunk, waves striding over the chunks: 8 workgroups (32 waves) per CU
  const u32 grid = std::min<u32>((n_chunks + HWG / 64 - 1) / (HWG / 64), (u32)cus * 8);
  hipLaunchKernelGGL(k_ideal_bits, dim3(grid), dim3(HWG), 0, s, d, chunk_hist, n_chunks, bits);
  const bool ok = hipGetLastError() == hipSuccess;
  // the pinned staging is reused by this thread's next call: wait for the copy
  const bool fr = hipFreeAsync(d, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  return ok && fr ? RC_OK : RC_E_DEVICE;
}

}  // extern "C"
