// rc_ideal_bits_order1.inc — the source of k_ideal_bits_order1 (rc_model_build.hip, which
// describes it), compiled twice: as k_ideal_bits_order1<PER> (lag 1, as it always was) and, with
// O1C_LAGGED defined, as k_ideal_bits_order1_lag<LAG> (a lagged set, DESIGN.md §9.15): row_i =
// map[i mod P][sym[i-LAG]] and first_row for i < LAG.  Only the context read changes; the sums and
// their order, and so the accuracy bound, do not.
#ifdef O1C_LAGGED
template <int LAG>
__global__ __launch_bounds__(1024) void k_ideal_bits_order1_lag(
#else
template <bool PER>
__global__ __launch_bounds__(1024) void k_ideal_bits_order1(
#endif
    const double* __restrict__ icl, const uint8_t* __restrict__ map, u32 first_row, u32 K,
    const uint8_t* __restrict__ syms, const u64* __restrict__ sym_off, u32 n_chunks,
    double* __restrict__ bits, u32 period) {
#ifdef O1C_LAGGED
  constexpr bool PER = true;
#else
  constexpr int LAG = 1;
#endif
  extern __shared__ double s_o1i[];
  uint8_t* const s_map = reinterpret_cast<uint8_t*>(s_o1i + K * 256u);
  const u32 lane = threadIdx.x & 63, waves = blockDim.x >> 6, pm = PER ? period - 1 : 0u;
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (u32 j = threadIdx.x; j < K * 256u; j += blockDim.x) s_o1i[j] = icl[j];
  // (one map: a workgroup has 256 lanes or more)
  if (PER) {
    for (u32 j = threadIdx.x; j < period * 256u; j += blockDim.x) s_map[j] = map[j];
  } else if (threadIdx.x < 256) {
    s_map[threadIdx.x] = map[threadIdx.x];
  }
  __syncthreads();
  const u32 nw = gridDim.x * waves;
  for (u32 k = blockIdx.x * waves + wave; k < n_chunks; k += nw) {
    const u64 s0 = sym_off[k], n = sym_off[k + 1] - s0;
    const uint8_t* p = syms + s0;
    double acc = 0.0;
    for (u64 i = 16ull * lane; i < n; i += 16ull * 64) {
      if constexpr (LAG > 1) {
        // the rows of the lane's next LAG symbols, slot j mod LAG for its j-th (i is a multiple
        // of 16: that symbol has phase j mod P)
        u32 rq[LAG];
#pragma unroll
        for (int f = 0; f < LAG; ++f)
          rq[f] = i ? (u32)s_map[(((u32)f & pm) << 8) + p[i - LAG + f]] : first_row;
        if (i + 16 <= n) {
          const u32x4 v = *(const __attribute__((address_space(1))) u32x4_h1*)(p + i);
          const u32 ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32 s = (ws[q] >> (8 * j)) & 255u;
              acc += s_o1i[rq[(4 * q + j) % LAG] * 256u + s];
              rq[(4 * q + j) % LAG] = s_map[(((u32)(4 * q + j + LAG) & pm) << 8) + s];
            }
          }
        } else {
          for (u64 j = i; j < n; ++j) {
            const u32 row =
                j >= (u64)LAG ? (u32)s_map[(((u32)j & pm) << 8) + p[j - LAG]] : first_row;
            acc += s_o1i[row * 256u + p[j]];
          }
        }
        continue;
      }
      u32 row = i ? (u32)s_map[p[i - 1]] : first_row;  // chunk boundaries reset the context
      if (i + 16 <= n) {
        const u32x4 v = *(const __attribute__((address_space(1))) u32x4_h1*)(p + i);
        const u32 ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32 s = (ws[q] >> (8 * j)) & 255u;
            acc += s_o1i[row * 256u + s];
            row = s_map[(((u32)(4 * q + j + 1) & pm) << 8) + s];
          }
        }
      } else {
        for (u64 j = i; j < n; ++j) {
          const u32 s = p[j];
          acc += s_o1i[row * 256u + s];
          row = s_map[((((u32)j + 1u) & pm) << 8) + s];
        }
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
