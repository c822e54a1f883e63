// rc_chunk_set.hip — static chunk sets (rc_chunk_set.h): the grouping of a launch
// by chunk class, the grouped encoder k_encode_static_grouped (the grouped decoders:
// rc_decode_grouped_{pow2,magic}.hip), and the kernels that fit the classes (a chunk's cost under
// every row, histograms summed by class).
#include "rc_host.h"

#include <math.h>

#include <algorithm>
#include <vector>

#include "rc_encode.inc"

// ------------------------------------------------------------------------------------------
// Grouping.  order[]: the chunk ids grouped by class, stable by chunk id inside a class, each
// class padded to whole workgroups of W lanes (~0u: a dead lane); wg_row[]: the class of every
// workgroup of the grid rc_group_grid(n, K, W) (~0u: unused).  Counts per tile, one scan, a
// scatter: no kernel waits for another workgroup.
//
// A tile is GROUP_TILE consecutive chunks and belongs to one wave, which walks it in rounds of 64.
// Lane c of the wave keeps class c's running count (K <= 64), and a round ranks its lanes class
// by class: one ballot per class present in the round.
// ------------------------------------------------------------------------------------------
static_assert(RC_MAX_SET_MODELS <= 64, "a lane per class");

template <int SCATTER>
__global__ __launch_bounds__(64) void k_group_tile(const uint8_t* __restrict__ class_of, u32 n,
                                                  u32 K, u32 nb, u32* __restrict__ blk,
                                                  const u32* __restrict__ base,
                                                  u32* __restrict__ order, u32* __restrict__ flags,
                                                  u64* __restrict__ out_len) {
  RC_VGPR_FLOOR_32();
  const u32 b = blockIdx.x, lane = threadIdx.x;
  // SCATTER: class `lane`'s next slot, its padded base plus the members in the tiles before
  u32 run = 0;
  if (SCATTER && lane < K) run = base[lane] + blk[(size_t)lane * nb + b];
  for (u32 r = 0; r < GROUP_TILE / 64; ++r) {
    const u32 k0 = b * GROUP_TILE + r * 64;  // (wave-uniform)
    if (k0 >= n) break;
    const u32 k = k0 + lane;
    const u32 cls = k < n ? (u32)class_of[k] : ~0u;
    const bool valid = cls < K;
    if (SCATTER && k < n && !valid) {
      flags[k] = RC_F_BAD_MODEL;
      if (out_len) out_len[k] = 0;
    }
    u64 rem = __builtin_amdgcn_ballot_w64(valid);
    while (rem) {  // (wave-uniform: every lane is in the loop)
      const u32 c0 = (u32)__shfl((int)cls, (int)__builtin_ctzll(rem));
      const u64 m = __builtin_amdgcn_ballot_w64(cls == c0);
      if (SCATTER) {
        const u32 start = (u32)__shfl((int)run, (int)c0);
        if (cls == c0)
          order[start + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((u32)m, 0u))] = k;
      }
      if (lane == c0) run += (u32)__builtin_popcountll(m);
      rem &= ~m;
    }
  }
  if (!SCATTER && lane < K) blk[(size_t)lane * nb + b] = run;
}

// One workgroup: blk[c][b] (class c's members in tile b) becomes the members in the tiles before
// b; base[c]: the class's first slot, the padded sizes of the classes before it; wg_row[].
__global__ __launch_bounds__(1024) void k_group_scan(u32* __restrict__ blk, u32 nb, u32 K, u32 W,
                                                    u32 grid, u32* __restrict__ base,
                                                    u32* __restrict__ wg_row) {
  RC_VGPR_FLOOR_32();
  __shared__ u32 s_tot[64];
  __shared__ u32 s_base[65];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (u32 c = wave; c < K; c += 16) {  // (wave-uniform)
    u32 carry = 0;
    u32* row = blk + (size_t)c * nb;
    for (u32 b0 = 0; b0 < nb; b0 += 64) {
      const u32 b = b0 + lane;
      const u32 v = b < nb ? row[b] : 0u;
      u32 x = v;  // inclusive scan over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u32 y = (u32)__shfl_up((int)x, o);
        if (lane >= (u32)o) x += y;
      }
      if (b < nb) row[b] = carry + x - v;
      carry += (u32)__shfl((int)x, 63);
    }
    if (lane == 0) s_tot[c] = carry;
  }
  __syncthreads();
  if (tid == 0) {
    u32 acc = 0;
    for (u32 c = 0; c < K; ++c) {
      s_base[c] = acc;
      acc += (s_tot[c] + W - 1) / W * W;
    }
    s_base[K] = acc;
  }
  __syncthreads();
  if (tid < K) base[tid] = s_base[tid];
  for (u32 g = tid; g < grid; g += 1024) {
    const u32 slot = g * W;
    u32 row = ~0u;
    for (u32 c = 0; c < K; ++c)
      if (slot >= s_base[c] && slot < s_base[c + 1]) row = c;
    wg_row[g] = row;
  }
}

// the launch's scratch: order [grid * W], wg_row [grid], base [64], blk [K * nb]
static size_t group_words(u32 n, u32 K, u32 W, u32 nb) {
  const size_t grid = rc_group_grid(n, K, W);
  return grid * W + grid + 64 + (size_t)K * nb;
}

static hipError_t group_into(hipStream_t stream, const uint8_t* class_of, u32 n, u32 K, u32 W,
                             u32* order, u32* wg_row, u32* base, u32* blk, u32 nb, u32* flags,
                             u64* out_len) {
  const u32 grid = rc_group_grid(n, K, W);
  hipError_t e = hipMemsetAsync(order, 0xFF, (size_t)grid * W * sizeof(u32), stream);
  if (e != hipSuccess) return e;
  if (nb)
    hipLaunchKernelGGL(k_group_tile<0>, dim3(nb), dim3(64), 0, stream, class_of, n, K, nb, blk,
                       (const u32*)nullptr, (u32*)nullptr, (u32*)nullptr, (u64*)nullptr);
  hipLaunchKernelGGL(k_group_scan, dim3(1), dim3(1024), 0, stream, blk, nb, K, W, grid, base,
                     wg_row);
  if (nb)
    hipLaunchKernelGGL(k_group_tile<1>, dim3(nb), dim3(64), 0, stream, class_of, n, K, nb, blk,
                       (const u32*)base, order, flags, out_len);
  return hipGetLastError();
}

hipError_t rc_chunk_group_launch(hipStream_t stream, GroupScratch& sc, const uint8_t* class_of,
                                 u32 n, u32 K, u32 W, u32* flags, u64* out_len, GroupArgs* ga) {
  const u32 nb = (n + GROUP_TILE - 1) / GROUP_TILE;
  const size_t bytes = group_words(n, K, W, nb) * sizeof(u32);
  hipError_t e;
  if (!sc.done && (e = hipEventCreateWithFlags(&sc.done, hipEventDisableTiming)) != hipSuccess)
    return e;
  // another stream than the last launch's: its coder must have read the scratch before this
  // launch rewrites (or frees) it
  if (sc.used && sc.last != stream && (e = hipStreamWaitEvent(stream, sc.done, 0)) != hipSuccess)
    return e;
  if (sc.cap < bytes) {  // (stream-ordered: behind the launches that still read the old buffer)
    if (sc.buf && (e = hipFreeAsync(sc.buf, stream)) != hipSuccess) return e;
    sc.buf = nullptr;
    sc.cap = 0;
    const size_t cap = bytes + bytes / 4;
    if ((e = hipMallocAsync(&sc.buf, cap, stream)) != hipSuccess) return e;
    sc.cap = cap;
  }
  sc.last = stream;
  sc.used = true;
  const u32 grid = rc_group_grid(n, K, W);
  u32* order = (u32*)sc.buf;
  u32* wg_row = order + (size_t)grid * W;
  u32* base = wg_row + grid;
  u32* blk = base + 64;
  ga->order = order;
  ga->wg_row = wg_row;
  return group_into(stream, class_of, n, K, W, order, wg_row, base, blk, nb, flags, out_len);
}

hipError_t rc_chunk_group_done(hipStream_t stream, GroupScratch& sc, u32 W, u32 lut, u32 grid) {
  sc.last_w = W;
  sc.last_lut = lut;
  sc.last_grid = grid;
  return hipEventRecord(sc.done, stream);
}

void rc_chunk_group_release(GroupScratch& sc) {
  if (sc.done) {
    if (sc.used) (void)hipEventSynchronize(sc.done);
    (void)hipEventDestroy(sc.done);
  }
  if (sc.buf) (void)hipFree(sc.buf);
  sc = GroupScratch{};
}

// ------------------------------------------------------------------------------------------
// The grouped encoder
// ------------------------------------------------------------------------------------------
#define SINK_SLOTS 65536
static __device__ uint4 g_sink[SINK_SLOTS];  // dummy symbol tiles of dead lanes (rc_encode.hip)
RC_STAMP_DEFINE(enc_grp)  // (scratch -DRC_STAMP builds only)
#define RC_ENC_TU enc_grp

#define RC_ENC_GROUPED 1
#include "rc_encode_static.inc"

hipError_t rc_chunk_encode_launch(hipStream_t stream, const RcKnobs& k, const ModelArgs& a_in,
                                  int div, const ChunkSetArgs& cs, GroupScratch& sc,
                                  const uint8_t* class_of, const uint8_t* syms, const u64* sym_off,
                                  u32 n_chunks, uint8_t* out, const u64* out_off, u64* out_len,
                                  u32* flags) {
  GroupArgs g{nullptr, nullptr, cs.lut_stride, cs.symof_stride};
  const hipError_t e =
      rc_chunk_group_launch(stream, sc, class_of, n_chunks, cs.k, WG, flags, out_len, &g);
  if (e != hipSuccess) return e;
  const dim3 grid(rc_group_grid(n_chunks, cs.k, WG)), block(WG);
  ModelArgs a = a_in;
  auto go = [&](auto kern) {
    rc_prio_policy(a, kPrioEncoder, grid.x,
                   rc_resident_wgs(reinterpret_cast<const void*>(kern), WG, 0), k);
    hipLaunchKernelGGL(kern, grid, block, 0, stream, a, g, syms, sym_off, n_chunks, out, out_off,
                       out_len, flags);
  };
  if (div == DIV_POW2) {
    if (cs.smv == 2) go(k_encode_static_grouped<DIV_POW2, 2>);
    else go(k_encode_static_grouped<DIV_POW2, 1>);
  } else {
    if (cs.smv == 2) go(k_encode_static_grouped<DIV_MAGIC, 2>);
    else go(k_encode_static_grouped<DIV_MAGIC, 1>);
  }
  const hipError_t le = hipGetLastError();
  const hipError_t de = rc_chunk_group_done(stream, sc, WG, 0, grid.x);
  return le != hipSuccess ? le : de;
}

// ------------------------------------------------------------------------------------------
// Fitting the classes.  Costs are integers in units of 2^-16 bit.
// ------------------------------------------------------------------------------------------
#define COST_NONE 0xFFFFFFFFu  // a symbol the row cannot code

// One wave per chunk, waves striding over the chunks; the K x 256 cost table in LDS.  Lane l
// holds the counts of symbols 4l .. 4l + 3 (the row read once, 1 KiB per wave), multiplies them
// with each row's entries and the wave sums the products.
__global__ __launch_bounds__(256) void k_chunk_costs(const u32* __restrict__ hist, u32 n, u32 K,
                                                    const u32* __restrict__ cost,
                                                    uint8_t* __restrict__ best_row,
                                                    u64* __restrict__ best_cost,
                                                    u64* __restrict__ costs) {
  RC_VGPR_FLOOR_64();
  extern __shared__ u32 s_cost[];
  for (u32 j = threadIdx.x; j < K * 256; j += 256) s_cost[j] = cost[j];
  __syncthreads();
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u32 k = blockIdx.x * 4 + wave; k < n; k += gridDim.x * 4) {  // (wave-uniform)
    const uint4 h = reinterpret_cast<const uint4*>(hist + (size_t)k * 256)[lane];
    u64 best = ~0ull, mine = 0;
    u32 arg = 0;
    for (u32 r = 0; r < K; ++r) {
      const uint4 c = reinterpret_cast<const uint4*>(s_cost + r * 256)[lane];
      const bool none = (h.x && c.x == COST_NONE) | (h.y && c.y == COST_NONE) |
                        (h.z && c.z == COST_NONE) | (h.w && c.w == COST_NONE);
      u64 t = (u64)h.x * c.x + (u64)h.y * c.y + (u64)h.z * c.z + (u64)h.w * c.w;
#pragma unroll
      for (int o = 32; o; o >>= 1)
        t += ((u64)(u32)__shfl_xor((int)hi32(t), o) << 32) | (u32)__shfl_xor((int)(u32)t, o);
      if (__builtin_amdgcn_ballot_w64(none)) t = ~0ull;
      if (r == 0 || t < best) {  // (ties: the lowest row)
        best = t;
        arg = r;
      }
      if (lane == r) mine = t;
    }
    if (lane == 0) {
      best_row[k] = (uint8_t)arg;
      best_cost[k] = best;
    }
    if (costs && lane < K) costs[(size_t)k * K + lane] = mine;
  }
}

// Thread t owns symbol t: it adds the counts of its workgroup's chunks into its column of the
// K x 256 LDS sums (no atomics: nobody else touches the column), then adds the column to the
// result.  A chunk with class_of >= K is skipped.
__global__ __launch_bounds__(256) void k_hist_by_class(const u32* __restrict__ hist,
                                                      const uint8_t* __restrict__ class_of, u32 n,
                                                      u32 K, u32 per_wg,
                                                      u64* __restrict__ class_hist) {
  RC_VGPR_FLOOR_32();
  extern __shared__ u64 s_sum[];
  const u32 t = threadIdx.x;
  for (u32 c = 0; c < K; ++c) s_sum[c * 256 + t] = 0;
  const u32 k0 = blockIdx.x * per_wg;
  const u32 k1 = k0 + per_wg < n ? k0 + per_wg : n;
  for (u32 k = k0; k < k1; ++k) {
    const u32 c = class_of[k];
    if (c < K) s_sum[c * 256 + t] += hist[(size_t)k * 256 + t];
  }
  for (u32 c = 0; c < K; ++c) {
    const u64 v = s_sum[c * 256 + t];
    if (v) atomicAdd((unsigned long long*)(class_hist + c * 256 + t), (unsigned long long)v);
  }
}

extern "C" {

rc_status rc_cost_table(const uint32_t* c_freq_host, uint32_t n_symbols, uint32_t total_freq,
                        uint32_t* cost_out_host) {
  if (!c_freq_host || !cost_out_host || n_symbols < 1 || n_symbols > 256 || total_freq < 1)
    return RC_E_ARG;
  for (u32 s = 0; s < n_symbols; ++s) {
    const u32 c = c_freq_host[s];
    if (c > total_freq) return RC_E_ARG;
    cost_out_host[s] =
        c ? (u32)llround(65536.0 * log2((double)total_freq / (double)c)) : COST_NONE;
  }
  return RC_OK;
}

rc_status rc_chunk_set_costs(rc_ctx* ctx, const uint32_t* chunk_hist, uint32_t n_chunks,
                             const uint32_t* cost_host, uint32_t n_models, uint8_t* best_row,
                             uint64_t* best_cost, uint64_t* costs) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS || n_models < 1 || n_models > RC_MAX_SET_MODELS)
    return RC_E_ARG;
  if (n_chunks == 0) return RC_OK;
  if (!chunk_hist || !cost_host || !best_row || !best_cost) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  rc_svc_yield_all_();
  const size_t bytes = (size_t)n_models * 256 * sizeof(u32);
  if (set_allow_lds(reinterpret_cast<const void*>(k_chunk_costs)) != hipSuccess)
    return RC_E_DEVICE;
  u32* d = nullptr;
  if (hipMallocAsync((void**)&d, bytes, s) != hipSuccess) return RC_E_DEVICE;
  void* pin = rc_pinned_scratch_(bytes);
  if (!pin) {
    (void)hipFreeAsync(d, s);
    return RC_E_DEVICE;
  }
  memcpy(pin, cost_host, bytes);
  if (hipMemcpyAsync(d, pin, bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipFreeAsync(d, s);
    return RC_E_DEVICE;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) !=
      hipSuccess)
    cus = 256;
  // a wave per chunk; the workgroups one CU holds follow from the table's LDS (2 at K = 64)
  const u32 per_cu = std::max<u32>(1u, std::min<u32>(8u, (u32)(160u * 1024u / bytes)));
  const u32 grid = std::min<u32>((n_chunks + 3) / 4, (u32)cus * per_cu);
  hipLaunchKernelGGL(k_chunk_costs, dim3(grid), dim3(256), bytes, s, chunk_hist, n_chunks,
                     n_models, (const u32*)d, best_row, best_cost, costs);
  const bool ok = hipGetLastError() == hipSuccess;
  // the pinned staging is reused by this thread's next call: wait for the copy
  const bool fr = hipFreeAsync(d, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  return ok && fr ? RC_OK : RC_E_DEVICE;
}

rc_status rc_histogram_by_class(rc_ctx* ctx, const uint32_t* chunk_hist, const uint8_t* class_of,
                                uint32_t n_chunks, uint32_t n_models, uint64_t* class_hist) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS || n_models < 1 || n_models > RC_MAX_SET_MODELS)
    return RC_E_ARG;
  if (n_chunks == 0) return RC_OK;
  if (!chunk_hist || !class_of || !class_hist) return RC_E_ARG;
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  rc_svc_yield_all_();
  if (set_allow_lds(reinterpret_cast<const void*>(k_hist_by_class)) != hipSuccess)
    return RC_E_DEVICE;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) !=
      hipSuccess)
    cus = 256;
  // at least 64 chunks per workgroup, so that its final adds stay a small share of its reads
  const u32 per_wg = std::max<u32>(64u, (n_chunks + (u32)cus * 4 - 1) / ((u32)cus * 4));
  const u32 grid = (n_chunks + per_wg - 1) / per_wg;
  hipLaunchKernelGGL(k_hist_by_class, dim3(grid), dim3(256),
                     (size_t)n_models * 256 * sizeof(u64), ctx->cur, chunk_hist, class_of,
                     n_chunks, n_models, per_wg, class_hist);
  return hipGetLastError() == hipSuccess ? RC_OK : RC_E_DEVICE;
}

// Internal test hooks (not in include/range_coder.h).
// rc_chunk_group_plan_: the grouping rule on the host (no device needed): order_out
// [rc_group_grid * W] and wg_row_out [rc_group_grid], what the device step writes.
rc_status rc_chunk_group_plan_(const uint8_t* class_of, uint32_t n, uint32_t K, uint32_t W,
                               uint32_t* order_out, uint32_t* wg_row_out) {
  if ((n && !class_of) || !order_out || !wg_row_out || K < 1 || K > RC_MAX_SET_MODELS ||
      (W != 256 && W != 512 && W != 1024) || n > RC_MAX_CHUNKS)
    return RC_E_ARG;
  const u32 grid = rc_group_grid(n, K, W);
  std::fill(order_out, order_out + (size_t)grid * W, ~0u);
  std::fill(wg_row_out, wg_row_out + grid, ~0u);
  std::vector<u32> cnt(K, 0), next(K, 0);
  for (u32 k = 0; k < n; ++k)
    if (class_of[k] < K) ++cnt[class_of[k]];
  u32 acc = 0;
  for (u32 c = 0; c < K; ++c) {
    next[c] = acc;
    const u32 wgs = (cnt[c] + W - 1) / W;
    for (u32 g = 0; g < wgs; ++g) wg_row_out[acc / W + g] = c;
    acc += wgs * W;
  }
  for (u32 k = 0; k < n; ++k)
    if (class_of[k] < K) order_out[next[class_of[k]]++] = k;
  return RC_OK;
}

// rc_chunk_group_: the device step itself into the caller's device arrays (sized as above);
// stream-ordered.  flags_dev: n entries, RC_F_BAD_MODEL written where class_of >= K.
rc_status rc_chunk_group_(rc_ctx* ctx, const uint8_t* class_of, uint32_t n, uint32_t K,
                          uint32_t W, uint32_t* order_dev, uint32_t* wg_row_dev,
                          uint32_t* flags_dev) {
  if (!ctx || !order_dev || !wg_row_dev || !flags_dev || (n && !class_of) || K < 1 ||
      K > RC_MAX_SET_MODELS || (W != 256 && W != 512 && W != 1024) || n > RC_MAX_CHUNKS)
    return RC_E_ARG;
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  GroupArgs ga{};
  if (rc_chunk_group_launch(ctx->cur, ctx->group, class_of, n, K, W, flags_dev, nullptr, &ga) !=
      hipSuccess)
    return RC_E_DEVICE;
  const u32 grid = rc_group_grid(n, K, W);
  if (hipMemcpyAsync(order_dev, ga.order, (size_t)grid * W * 4, hipMemcpyDeviceToDevice,
                     ctx->cur) != hipSuccess ||
      hipMemcpyAsync(wg_row_dev, ga.wg_row, (size_t)grid * 4, hipMemcpyDeviceToDevice, ctx->cur) !=
          hipSuccess)
    return RC_E_DEVICE;
  // (the copies read the scratch: they are this launch's readers)
  if (rc_chunk_group_done(ctx->cur, ctx->group, W, 0, grid) != hipSuccess) return RC_E_DEVICE;
  return RC_OK;
}

// rc_chunk_last_: what the context's last chunk-set coder launch took, out[3] = {lanes per
// workgroup, the decoder's LUT (0: an encoder launch), workgroups}.  Tests and tools/
// kbench_chunk_set.py read which variant a launch really ran.
rc_status rc_chunk_last_(rc_ctx* ctx, uint32_t* out) {
  if (!ctx || !out) return RC_E_ARG;
  out[0] = ctx->group.last_w;
  out[1] = ctx->group.last_lut;
  out[2] = ctx->group.last_grid;
  return RC_OK;
}

}  // extern "C"
