// rc_encode.hip — k_encode_static, the static-model encoder (see rc_static.h for the design
// notes shared with the decoder).
#include "rc_static.h"

#include <map>
#include <mutex>
#include <tuple>

#include "rc_encode.inc"

#define SINK_SLOTS 65536
__device__ uint4 g_sink[SINK_SLOTS];  // dummy symbol tiles of dead lanes (contents irrelevant)
RC_STAMP_DEFINE(enc)  // (scratch -DRC_STAMP builds only)
#define RC_ENC_TU enc

#include "rc_encode_static.inc"

u32 rc_resident_wgs(const void* kernel, int block, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, size_t>, u32> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> g(mu);
  const auto key = std::make_tuple(dev, kernel, lds);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return cache[key] = (u32)(per_cu * cus);
}

hipError_t rc_static_encode_launch(hipStream_t stream, const RcKnobs& k, const ModelArgs& a_in,
                                   int div, int smv, const uint8_t* syms, const u64* sym_off,
                                   u32 n_chunks, uint8_t* out, const u64* out_off, u64* out_len,
                                   u32* flags) {
  const dim3 grid((n_chunks + WG - 1) / WG), block(WG);
  ModelArgs a = a_in;
  // (the launch's wave priorities: rc_static.h)
  auto go = [&](auto kern) {
    rc_prio_policy(a, kPrioEncoder, grid.x,
                   rc_resident_wgs(reinterpret_cast<const void*>(kern), WG, 0), k);
    hipLaunchKernelGGL(kern, grid, block, 0, stream, a, syms, sym_off, n_chunks, out, out_off,
                       out_len, flags);
  };
#ifdef RC_DEV_ONLY  // scratch builds for kernel tuning: the headline variants only
  if (div != DIV_POW2 || smv == 0) return hipErrorInvalidValue;
  if (a.flat) go(k_encode_static<DIV_POW2, 3>);
  else if (smv == 2) go(k_encode_static<DIV_POW2, 2>); else go(k_encode_static<DIV_POW2, 1>);
#else
  if (div == DIV_POW2) {
    if (a.flat) go(k_encode_static<DIV_POW2, 3>);  // the flat model (SM 3: no table reads)
    else if (smv == 2) go(k_encode_static<DIV_POW2, 2>);
    else if (smv == 1) go(k_encode_static<DIV_POW2, 1>);
    else go(k_encode_static<DIV_POW2, 0>);
  } else {
    if (smv == 2) go(k_encode_static<DIV_MAGIC, 2>);
    else if (smv == 1) go(k_encode_static<DIV_MAGIC, 1>);
    else go(k_encode_static<DIV_MAGIC, 0>);
  }
#endif
  return hipGetLastError();
}
