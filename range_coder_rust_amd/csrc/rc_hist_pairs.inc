// rc_hist_pairs.inc — the source of k_histogram_pairs (rc_model_build.hip, which describes it),
// compiled twice: as k_histogram_pairs<PER> (lag 1, as it always was) and, with O1C_LAGGED
// defined, as k_histogram_pairs_lag<LAG> (rc_histogram_pairs_lagged; DESIGN.md §9.15): the
// previous symbol of position i is sym[i-LAG], and the positions i < LAG of a chunk go to `first`.
// A lane's 16 symbols still start at a multiple of 16 (and so of LAG) from the chunk's start: the
// context of its j-th symbol is its own (j - LAG)-th for j >= LAG and one of the LAG bytes before
// its first otherwise, a queue of LAG values whose slot is the compile-time j mod LAG.  The phase
// test and the budget (symbols read) are the same.
#ifdef O1C_LAGGED
template <int LAG>
__global__ __launch_bounds__(O1P_WG) void k_histogram_pairs_lag(
#else
template <bool PER>
__global__ __launch_bounds__(O1P_WG) void k_histogram_pairs(
#endif
    const uint8_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_chunks,
    u64* __restrict__ pair, u64* __restrict__ first, u32 period) {
#ifdef O1C_LAGGED
  constexpr bool PER = true;
#else
  constexpr int LAG = 1;
#endif
  extern __shared__ u32 s_pp[];
  const u32 tid = threadIdx.x;
  const u32 P = PER ? period : 1u, pm = P - 1;
  const u32 slices = O1P_SLICES * P;
  const u32 g = blockIdx.x % slices, w = blockIdx.x / slices;
  const u32 G = gridDim.x / slices;
  const u32 ph = g / O1P_SLICES;
  const u32 base = (g % O1P_SLICES) * O1P_ROWS;  // the slice's first context
  const bool do_first = first && g == 0;
  RC_VGPR_FLOOR_48();
  if (!pair && !do_first) return;  // (workgroup-uniform)
  u32* const s_first = s_pp + O1P_ROWS * 256u;
  for (u32 j = tid; j < O1P_WORDS; j += O1P_WG) s_pp[j] = 0;
  __syncthreads();
  auto flush = [&]() {
    __syncthreads();
    if (pair) {
      for (u32 j = tid; j < O1P_ROWS * 256u; j += O1P_WG) {
        const u32 v = s_pp[j];
        if (v) {
          atomicAdd(reinterpret_cast<unsigned long long*>(pair + ((u64)ph * 256u + base) * 256u + j),
                    (unsigned long long)v);
          s_pp[j] = 0;
        }
      }
    }
    if (do_first && tid < 256) {
      const u32 v = s_first[tid];
      if (v) {
        atomicAdd(reinterpret_cast<unsigned long long*>(first + tid), (unsigned long long)v);
        s_first[tid] = 0;
      }
    }
    __syncthreads();
  };
  u64 pending = 0;  // symbols counted since the last flush (workgroup-uniform)
  const u32 sub = tid / O1P_SUB, t = tid % O1P_SUB;
  // a round: O1P_Q consecutive chunks, one per O1P_SUB lanes.  Every thread reads the round's
  // lengths, so the budget and the flush (which has barriers) stay workgroup-uniform while the
  // sub-groups walk chunks of different lengths.
  for (u32 k0 = w * O1P_Q; k0 < n_chunks; k0 += G * O1P_Q) {
    u64 len[O1P_Q], nmax = 0;
#pragma unroll
    for (u32 q = 0; q < O1P_Q; ++q) {
      len[q] = k0 + q < n_chunks ? sym_off[k0 + q + 1] - sym_off[k0 + q] : 0;
      nmax = len[q] > nmax ? len[q] : nmax;
    }
    const u32 k = k0 + sub;
    const u64 s0 = k < n_chunks ? sym_off[k] : 0, n = k < n_chunks ? sym_off[k + 1] - s0 : 0;
    const uint8_t* p = syms + s0;
    for (u64 b0 = 0; b0 < nmax; b0 += O1P_SEG) {
      u64 cnt = 0;  // at most O1P_Q * O1P_SEG = 2^31
#pragma unroll
      for (u32 q = 0; q < O1P_Q; ++q)
        cnt += len[q] > b0 ? (len[q] - b0 < O1P_SEG ? len[q] - b0 : O1P_SEG) : 0;
      if (pending + cnt > 0xFFFFFFFFull) {
        flush();
        pending = 0;
      }
      pending += cnt;
      if (b0 >= n) continue;
      const u64 b1 = n - b0 < O1P_SEG ? n : b0 + O1P_SEG;
      if (!pair) {  // first symbols only (at a lag: the chunk's first LAG)
        if (b0 == 0 && t == 0) {
          if constexpr (LAG > 1) {
            for (u32 f = 0; f < (u32)LAG && f < n; ++f) atomicAdd(&s_first[p[f]], 1u);
          } else {
            atomicAdd(&s_first[p[0]], 1u);
          }
        }
        continue;
      }
      for (u64 i = b0 + 16ull * t; i < b1; i += 16ull * O1P_SUB) {
        if constexpr (LAG > 1) {
          // the contexts of the lane's next LAG symbols relative to the slice, slot j mod LAG for
          // its j-th symbol; the first LAG symbols of a chunk have none and are counted in the
          // first-symbol histogram
          u32 rq[LAG];
#pragma unroll
          for (int f = 0; f < LAG; ++f) rq[f] = i ? (u32)p[i - LAG + f] - base : 0x80000000u;
          if (i == 0 && do_first)
            for (u32 f = 0; f < (u32)LAG && f < n; ++f) atomicAdd(&s_first[p[f]], 1u);
          if (i + 16 <= b1) {
            const u32x4 v = *(const __attribute__((address_space(1))) u32x4_h1*)(p + i);
            const u32 ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const u32 s = (ws[q] >> (8 * j)) & 255u;
                const u32 rel = rq[(4 * q + j) % LAG];
                if (((u32)(4 * q + j) & pm) == ph && rel < O1P_ROWS)
                  atomicAdd(&s_pp[rel * 256u + s], 1u);
                rq[(4 * q + j) % LAG] = s - base;
              }
            }
          } else {
            for (u64 j = i; j < b1; ++j) {
              const u32 rel = j >= (u64)LAG ? (u32)p[j - LAG] - base : 0x80000000u;
              if (((u32)j & pm) == ph && rel < O1P_ROWS) atomicAdd(&s_pp[rel * 256u + p[j]], 1u);
            }
          }
          continue;
        }
        // the previous symbol relative to the slice; a chunk's first symbol has none (chunk
        // boundaries reset the context) and is counted in the first-symbol histogram
        u32 rel = i ? (u32)p[i - 1] - base : 0x80000000u;
        if (i == 0 && do_first) atomicAdd(&s_first[p[0]], 1u);
        if (i + 16 <= b1) {
          const u32x4 v = *(const __attribute__((address_space(1))) u32x4_h1*)(p + i);
          const u32 ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32 s = (ws[q] >> (8 * j)) & 255u;
              if (((u32)(4 * q + j) & pm) == ph && rel < O1P_ROWS)
                atomicAdd(&s_pp[rel * 256u + s], 1u);
              rel = s - base;
            }
          }
        } else {
          for (u64 j = i; j < b1; ++j) {
            const u32 s = p[j];
            if (((u32)j & pm) == ph && rel < O1P_ROWS) atomicAdd(&s_pp[rel * 256u + s], 1u);
            rel = s - base;
          }
        }
      }
    }
  }
  flush();
}
