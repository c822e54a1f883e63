// rc_container.hip — the chunked container ("RCB1"): framing that makes a batch of coded chunks
// a self-describing codec.
//
// The reference's stream carries neither its symbol count nor its model: the decoder gets the
// count out of band (examples/sample_impl.rs:113-120) and the table from the caller
// (decoder.rs:38).  The container stores both, plus a per-chunk index, in front of the
// concatenated chunk streams.  Layout (little-endian, include/range_coder.h):
//   [0, 64)              header (rc_container_header)
//   [64, index_off)      model table: static -> n_symbols x u32 c_freq (cum = calc_cum), padded
//   [index_off, +16n)    per chunk {u64 symbol count, u64 code length}
//   [payload_off, end)   chunk k's code at payload_off + sum_{j<k} pad16(len_j), zero padded
// Every chunk stream starts 16-B aligned, so packing is a 16-B vector copy from the encoder's
// slots and the decoder reads the payload in place.
//
// GPU work: exclusive scans of the padded lengths / symbol counts (k_scan_*), the payload
// gather (k_pack_payload, HBM-bound), index writes and reads.
//
// "RCB2" (second half of the host side) is a second format with the same index
// and payload: it also frames order-1 sets and wide static models, and may carry one checksum
// of the decoded symbols per chunk (k_chunk_checksum, HBM-bound).  RCB1's entry points and
// kernels are unchanged by it.
#include "rc_host.h"

#include <string.h>

#include <algorithm>
#include <vector>

#define SWG 256
#define SPER 4                  // items per thread in a scan block
#define SBLK (SWG * SPER)       // items per scan block

static __device__ __forceinline__ u64 pad16(u64 v) { return (v + 15) & ~15ull; }

enum { SCAN_SRC_PLAIN = 0, SCAN_SRC_PAD16 = 1, SCAN_SRC_STRIDE2_PAD16 = 2, SCAN_SRC_STRIDE2 = 3,
       SCAN_SRC_DIFF = 4 };

// item i of the scan input: PLAIN v[i]; PAD16 pad16(v[i]); STRIDE2(_PAD16) (pad16)(v[2i + sel])
// (an index entry field); DIFF v[i+1] - v[i] (chunk sizes from offsets)
static __device__ __forceinline__ u64 scan_item(const u64* v, u32 i, int src, u32 sel) {
  switch (src) {
    case SCAN_SRC_PAD16: return pad16(v[i]);
    case SCAN_SRC_STRIDE2_PAD16: return pad16(v[2 * (u64)i + sel]);
    case SCAN_SRC_STRIDE2: return v[2 * (u64)i + sel];
    case SCAN_SRC_DIFF: return v[i + 1] - v[i];
    default: return v[i];
  }
}

// exclusive scan of one SBLK block; out[i] = base + prefix within the block, block total to
// sums[blockIdx] (pass 1) or, with add != nullptr, add[blockIdx] folded in (pass 3)
__global__ __launch_bounds__(SWG) void k_scan_block(const u64* __restrict__ v, u32 n, int src,
                                                    u32 sel, u64 base, u64* __restrict__ out,
                                                    u64* __restrict__ sums,
                                                    const u64* __restrict__ add) {
  __shared__ u64 s_w[SWG / 64];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 i0 = blockIdx.x * SBLK + tid * SPER;
  RC_VGPR_FLOOR_48();
  u64 x[SPER], t = 0;
#pragma unroll
  for (int j = 0; j < SPER; ++j) {
    x[j] = (i0 + j < n) ? scan_item(v, i0 + j, src, sel) : 0ull;
    t += x[j];
  }
  // inclusive wave scan of the thread totals
  u64 inc = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 y = ((u64)(u32)__shfl_up((int)hi32(inc), o) << 32) | (u32)__shfl_up((int)(u32)inc, o);
    if (lane >= (u32)o) inc += y;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  u64 wbase = 0;
  for (u32 w = 0; w < wave; ++w) wbase += s_w[w];
  if (sums) {  // pass 1: block totals only
    if (tid == SWG - 1) sums[blockIdx.x] = wbase + inc;
    return;
  }
  // single block, or pass 3 with the block's exclusive offset in add[]
  u64 run = base + (add ? add[blockIdx.x] : 0ull) + wbase + inc - t;
#pragma unroll
  for (int j = 0; j < SPER; ++j) {
    if (i0 + j < n) out[i0 + j] = run;
    run += x[j];
  }
  if (i0 < n && n <= i0 + SPER) out[n] = run;  // the total, by the thread of the last item
}

// the block sums of pass 1 -> their exclusive prefix (one WG, sequential over tiles)
__global__ __launch_bounds__(SWG) void k_scan_sums(u64* __restrict__ sums, u32 nb) {
  __shared__ u64 s[SWG];
  __shared__ u64 carry;
  const u32 tid = threadIdx.x;
  RC_VGPR_FLOOR_32();
  if (tid == 0) carry = 0;
  for (u32 b0 = 0; b0 < nb; b0 += SWG) {
    __syncthreads();
    const u64 v = (b0 + tid < nb) ? sums[b0 + tid] : 0ull;
    s[tid] = v;
    __syncthreads();
    for (u32 o = 1; o < SWG; o <<= 1) {  // Hillis-Steele inclusive scan in LDS
      const u64 y = tid >= o ? s[tid - o] : 0ull;
      __syncthreads();
      s[tid] += y;
      __syncthreads();
    }
    const u64 c = carry;
    if (b0 + tid < nb) sums[b0 + tid] = c + s[tid] - v;
    __syncthreads();
    if (tid == SWG - 1) carry = c + s[tid];
  }
}

// Exclusive scan (n items -> out[0..n], out[n] = base + total), stream-ordered.  tmp: >=
// ceil(n / SBLK) u64 of scratch.
static hipError_t device_scan(hipStream_t s, const u64* v, u32 n, int src, u32 sel, u64 base,
                              u64* out, u64* tmp) {
  const u32 nb = (n + SBLK - 1) / SBLK;
  if (nb <= 1) {
    hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(SWG), 0, s, v, n, src, sel, base, out,
                       (u64*)nullptr, (const u64*)nullptr);
    if (n == 0) {
      u64 z = base;  // empty: out[0] = base
      return hipMemcpyAsync(out, &z, 8, hipMemcpyHostToDevice, s) == hipSuccess &&
                     hipStreamSynchronize(s) == hipSuccess
                 ? hipSuccess
                 : hipErrorUnknown;
    }
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_scan_block, dim3(nb), dim3(SWG), 0, s, v, n, src, sel, base, out, tmp,
                     (const u64*)nullptr);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SWG), 0, s, tmp, nb);
  hipLaunchKernelGGL(k_scan_block, dim3(nb), dim3(SWG), 0, s, v, n, src, sel, base, out,
                     (u64*)nullptr, (const u64*)tmp);
  return hipGetLastError();
}

// payload gather: chunk k's code (len[k] bytes of its encoder slot) -> dst + doff[k], zero
// padded to 16 B; index entry k = {symbol count, code length}.  One wave per chunk (SWG / 64
// chunks per workgroup), grid-stride over the chunks.
__global__ __launch_bounds__(SWG) void k_pack_payload(const uint8_t* __restrict__ slots,
                                                      const u64* __restrict__ slot_off,
                                                      const u64* __restrict__ len,
                                                      const u64* __restrict__ sym_off,
                                                      u32 n_chunks, uint8_t* __restrict__ dst,
                                                      const u64* __restrict__ doff,
                                                      u64* __restrict__ index) {
  // one wave per chunk (four chunks per workgroup in flight, no barriers): a chunk's last
  // partial round of 16-B granules idles fewer lanes, and one chunk's offset loads overlap the
  // other waves' copies
  const u32 tid = threadIdx.x & 63;
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  RC_VGPR_FLOOR_32();
  for (u32 k = blockIdx.x * (SWG / 64) + wave; k < n_chunks; k += gridDim.x * (SWG / 64)) {
    const u64 l = len[k];
    const uint8_t* sp = slots + slot_off[k];
    uint8_t* dp = dst + doff[k];  // 16-B aligned
    if (tid == 0) {
      index[2 * (u64)k] = sym_off[k + 1] - sym_off[k];
      index[2 * (u64)k + 1] = l;
    }
    const u64 ng = pad16(l) >> 4;
    if (((uintptr_t)sp & 15) == 0) {
      const u64 full = l >> 4;  // whole granules inside the stream
      const u32x4* src = reinterpret_cast<const u32x4*>(sp);
      u64 g = tid;
      for (; g + 192 < full; g += 256) {  // four granules per lane in flight
        const u32x4 a = gload16(src + g), b = gload16(src + g + 64), c = gload16(src + g + 128),
                    d = gload16(src + g + 192);
        gstore128(dp + 16 * g, a);
        gstore128(dp + 16 * (g + 64), b);
        gstore128(dp + 16 * (g + 128), c);
        gstore128(dp + 16 * (g + 192), d);
      }
      for (; g < full; g += 64) gstore128(dp + 16 * g, gload16(src + g));
      if (tid == 0 && full < ng) {  // last partial granule: stream bytes, then zeros
        u32 w[4] = {0, 0, 0, 0};
        for (u32 j = 0; j < (u32)(l & 15); ++j) w[j >> 2] |= (u32)sp[16 * full + j] << (8 * (j & 3));
        u32x4 v;
        v.x = w[0];
        v.y = w[1];
        v.z = w[2];
        v.w = w[3];
        gstore128(dp + 16 * full, v);
      }
    } else {  // misaligned slot: dword-assembled granules
      for (u64 g = tid; g < ng; g += 64) {
        u32 w[4] = {0, 0, 0, 0};
        for (u32 j = 0; j < 16; ++j) {
          const u64 p = 16 * g + j;
          if (p < l) w[j >> 2] |= (u32)sp[p] << (8 * (j & 3));
        }
        u32x4 v;
        v.x = w[0];
        v.y = w[1];
        v.z = w[2];
        v.w = w[3];
        gstore128(dp + 16 * g, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// RCB2's per-chunk checksum (include/range_coder.h): S = sum_i fmix32(w_i + (i + 1) * GOLD) over
// the chunk's little-endian words, zero padded; sum = fmix32(S ^ (u32)L).  Order-free, so lanes
// accumulate privately and one butterfly ends the chunk.
// ------------------------------------------------------------------------------------------
#define CSUM_GOLD 0x9E3779B1u

typedef u32x4 u32x4_c1 __attribute__((aligned(1)));

static __device__ __forceinline__ u32 fmix32(u32 h) {  // MurmurHash3's 32-bit finaliser
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// the terms of words 4g .. 4g + 3 (granule g of the chunk; word indices count mod 2^32, as the
// definition's position term does)
static __device__ __forceinline__ u32 csum_granule(u32x4 v, u32 g) {
  const u32 b = (4u * g + 1u) * CSUM_GOLD;
  return fmix32(v.x + b) + fmix32(v.y + b + CSUM_GOLD) + fmix32(v.z + b + 2u * CSUM_GOLD) +
         fmix32(v.w + b + 3u * CSUM_GOLD);
}

// 16 bytes at any alignment, all of them inside the chunk (one unaligned global load, as the
// indexed encoder's index loads)
static __device__ __forceinline__ u32x4 gload16u(const uint8_t* p) {
  return *(const __attribute__((address_space(1))) u32x4_c1*)p;
}

// Chunk k = bytes [off[k] * sym_bytes, off[k+1] * sym_bytes) of data.  One wave per chunk
// (SWG / 64 chunks per workgroup, no barriers), grid-stride over the chunks, as k_pack_payload.
// Granules are counted from the chunk's first byte, whatever its alignment: granule g is the 16
// bytes at 16g, loaded whole only when all 16 lie inside the chunk, so a load never touches an
// aligned 16-B granule of memory that holds no byte of the chunk; the last L & 15 bytes are read
// one by one.  expect == nullptr: sums[k] = the checksum.  Otherwise nothing is stored and the
// lowest k whose checksum is not expect[k] goes to *first_bad (atomicMin).
__global__ __launch_bounds__(SWG) void k_chunk_checksum(const uint8_t* __restrict__ data,
                                                        const u64* __restrict__ off,
                                                        u32 n_chunks, u32 sym_bytes,
                                                        u32* __restrict__ sums,
                                                        const u32* __restrict__ expect,
                                                        u32* __restrict__ first_bad) {
  const u32 tid = threadIdx.x & 63;
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  RC_VGPR_FLOOR_64();  // (56 are used; allocations stay multiples of 16, rc_common.h)
  for (u32 k = blockIdx.x * (SWG / 64) + wave; k < n_chunks; k += gridDim.x * (SWG / 64)) {
    const u64 b = off[k], e = off[k + 1];
    const u64 l = e > b ? (e - b) * sym_bytes : 0ull;  // (offsets that run backwards: empty)
    const uint8_t* sp = data + b * sym_bytes;
    const u64 full = l >> 4;  // whole granules inside the chunk
    u32 acc = 0;
    u64 g = tid;
    for (; g + 192 < full; g += 256) {  // four granules per lane in flight
      const u32x4 v0 = gload16u(sp + 16 * g), v1 = gload16u(sp + 16 * (g + 64)),
                  v2 = gload16u(sp + 16 * (g + 128)), v3 = gload16u(sp + 16 * (g + 192));
      acc += csum_granule(v0, (u32)g) + csum_granule(v1, (u32)g + 64u) +
             csum_granule(v2, (u32)g + 128u) + csum_granule(v3, (u32)g + 192u);
    }
    for (; g < full; g += 64) acc += csum_granule(gload16u(sp + 16 * g), (u32)g);
    // the tail: word j of the last, partial granule, by lane j (bytes past the end are zero)
    const u32 rem = (u32)l & 15u;
    if (4u * tid < rem) {
      u32 w = 0;
      for (u32 j = 0; j < 4; ++j)
        if (4u * tid + j < rem) w |= (u32)sp[16 * full + 4u * tid + j] << (8 * j);
      acc += fmix32(w + (4u * (u32)full + tid + 1u) * CSUM_GOLD);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += (u32)__shfl_xor((int)acc, o);
    if (tid == 0) {
      const u32 sum = fmix32(acc ^ (u32)l);
      if (!expect)
        sums[k] = sum;
      else if (sum != expect[k])
        atomicMin(first_bad, k);
    }
  }
}

// index -> decode arguments: code_len[k] = index[2k+1]; entries with absurd sizes raise *bad
__global__ __launch_bounds__(SWG) void k_unpack_index(const u64* __restrict__ index, u32 n,
                                                      u64* __restrict__ code_len,
                                                      u32* __restrict__ bad) {
  const u32 k = blockIdx.x * SWG + threadIdx.x;
  RC_VGPR_FLOOR_32();
  if (k >= n) return;
  const u64 sc = index[2 * (u64)k], l = index[2 * (u64)k + 1];
  code_len[k] = l;
  if (sc > (1ull << 48) || l > (1ull << 48)) atomicOr(bad, 1u);
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
namespace {
u64 hpad16(u64 v) { return (v + 15) & ~15ull; }

struct Scratch {
  void* p = nullptr;
  hipStream_t s;
  explicit Scratch(hipStream_t st) : s(st) {}
  bool alloc(size_t n) { return hipMallocAsync(&p, n ? n : 16, s) == hipSuccess; }
  ~Scratch() {
    if (p) (void)hipFreeAsync(p, s);
  }
};

void put32(uint8_t* p, u32 v) { memcpy(p, &v, 4); }
void put64(uint8_t* p, u64 v) { memcpy(p, &v, 8); }
u32 get32(const uint8_t* p) {
  u32 v;
  memcpy(&v, p, 4);
  return v;
}
u64 get64(const uint8_t* p) {
  u64 v;
  memcpy(&v, p, 8);
  return v;
}
}  // namespace

extern "C" {

rc_status rc_container_info_parse(const uint8_t* head, uint64_t head_len, rc_container_info* info) {
  if (!head || !info) return RC_E_ARG;
  if (head_len < RC_CONTAINER_HEADER_BYTES) return RC_E_BAD_CONTAINER;
  if (memcmp(head, "RCB1", 4) != 0) return RC_E_BAD_CONTAINER;
  rc_container_info in;
  memset(&in, 0, sizeof in);
  const u32 vh = get32(head + 4);
  in.version = vh & 0xFFFF;
  if (in.version != 1 || (vh >> 16) != RC_CONTAINER_HEADER_BYTES) return RC_E_BAD_CONTAINER;
  in.kind = get32(head + 8);
  in.n_symbols = get32(head + 12);
  in.total_freq = get32(head + 16);
  in.increment = get32(head + 20);
  in.limit = get32(head + 24);
  in.period = get32(head + 28);
  in.n_chunks = get64(head + 32);
  in.n_syms = get64(head + 40);
  in.payload_bytes = get64(head + 48);
  if (in.kind > 1 || in.n_symbols < 1 || in.n_symbols > 256 || in.n_chunks > RC_MAX_CHUNKS)
    return RC_E_BAD_CONTAINER;
  in.table_off = RC_CONTAINER_HEADER_BYTES;
  in.index_off = in.table_off + (in.kind == 0 ? hpad16(4ull * in.n_symbols) : 0);
  in.payload_off = in.index_off + 16 * in.n_chunks;
  in.container_bytes = in.payload_off + in.payload_bytes;
  if (in.payload_bytes & 15 || in.payload_bytes > (1ull << 56)) return RC_E_BAD_CONTAINER;
  *info = in;
  return RC_OK;
}

rc_status rc_container_pack(rc_ctx* ctx, const rc_model* m, const uint8_t* slots_dev,
                            const uint64_t* slot_off_dev, const uint64_t* code_len_dev,
                            const uint64_t* sym_off_dev, uint32_t n_chunks, uint8_t* dst_dev,
                            uint64_t dst_cap, uint64_t* dst_len_host) {
  if (!ctx || !m || !dst_len_host || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_chunks && (!slots_dev || !slot_off_dev || !code_len_dev || !sym_off_dev)) return RC_E_ARG;
  // (RCB1 frames single-table one-byte models only)
  if (!rc_model_kind_ok(m, RC_KINDS_SINGLE) || m->device != dev) return RC_E_ARG;
  const int kind = m->kind;
  const u32 nsym = kind == 0 ? m->args.n : m->ap.n, total = m->args.total;
  const u32 inc = m->ap.inc, lim = m->ap.limit, per = m->period;
  const u32* const c_host = m->c_host;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  const u64 index_off = RC_CONTAINER_HEADER_BYTES + (kind == 0 ? hpad16(4ull * nsym) : 0);
  const u64 payload_off = index_off + 16ull * n_chunks;
  // scans: dst offsets of the padded streams, and the symbol total
  const u32 nb = (n_chunks + SBLK - 1) / SBLK;
  Scratch sc(s);
  if (!sc.alloc(8ull * (n_chunks + 1) * 2 + 8ull * (nb + 1))) return RC_E_DEVICE;
  u64* doff = (u64*)sc.p;
  u64* soff = doff + (n_chunks + 1);
  u64* tmp = soff + (n_chunks + 1);
  hipError_t e = device_scan(s, code_len_dev, n_chunks, SCAN_SRC_PAD16, 0, payload_off, doff, tmp);
  if (e == hipSuccess) e = device_scan(s, sym_off_dev, n_chunks, SCAN_SRC_DIFF, 0, 0, soff, tmp);
  // small read-backs and the header go through pinned memory: [0, 16) ends, [64, ...) header
  char* pin = (char*)rc_pinned_scratch_(64 + RC_CONTAINER_HEADER_BYTES + 1024 + 16);
  if (!pin) return RC_E_DEVICE;
  u64* ends = (u64*)pin;
  ends[0] = payload_off;
  ends[1] = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&ends[0], doff + n_chunks, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&ends[1], soff + n_chunks, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return RC_E_DEVICE;
  const u64 total_bytes = ends[0];
  *dst_len_host = total_bytes;
  if (!dst_dev || total_bytes > dst_cap) return RC_E_CAPACITY;
  // header + table (host-built, one copy)
  uint8_t head[RC_CONTAINER_HEADER_BYTES + 1024 + 16];
  memset(head, 0, sizeof head);
  memcpy(head, "RCB1", 4);
  put32(head + 4, 1u | ((u32)RC_CONTAINER_HEADER_BYTES << 16));
  put32(head + 8, (u32)kind);
  put32(head + 12, nsym);
  put32(head + 16, kind == 0 ? total : 0u);
  put32(head + 20, kind == 1 ? inc : 0u);
  put32(head + 24, kind == 1 ? lim : 0u);
  put32(head + 28, kind == 1 ? per : 0u);
  put64(head + 32, n_chunks);
  put64(head + 40, ends[1]);
  put64(head + 48, total_bytes - payload_off);
  if (kind == 0)
    for (u32 i = 0; i < nsym; ++i) put32(head + RC_CONTAINER_HEADER_BYTES + 4 * i, c_host[i]);
  memcpy(pin + 64, head, index_off);
  if (hipMemcpyAsync(dst_dev, pin + 64, index_off, hipMemcpyHostToDevice, s) != hipSuccess)
    return RC_E_DEVICE;
  if (n_chunks) {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const u32 grid = std::min<u32>((n_chunks + SWG / 64 - 1) / (SWG / 64), (u32)std::max(cus, 1) * 16);
    hipLaunchKernelGGL(k_pack_payload, dim3(grid), dim3(SWG), 0, s, slots_dev, slot_off_dev,
                       code_len_dev, sym_off_dev, n_chunks, dst_dev, doff,
                       reinterpret_cast<u64*>(dst_dev + index_off));
    if (hipGetLastError() != hipSuccess) return RC_E_DEVICE;
  }
  // the pinned staging is reused by this thread's next call: wait for its copy (and free the
  // scratch in order)
  return hipStreamSynchronize(s) == hipSuccess ? RC_OK : RC_E_DEVICE;
}

rc_status rc_container_offsets(rc_ctx* ctx, const uint8_t* container_dev,
                               const rc_container_info* info, uint64_t* code_off_dev,
                               uint64_t* code_len_dev, uint64_t* sym_off_dev) {
  if (!ctx || !container_dev || !info) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  const u32 n = (u32)info->n_chunks;
  if (info->n_chunks > RC_MAX_CHUNKS) return RC_E_BAD_CONTAINER;
  if (n && (!code_off_dev || !code_len_dev || !sym_off_dev)) return RC_E_ARG;
  DeviceGuard g(dev);
  const u64* index = reinterpret_cast<const u64*>(container_dev + info->index_off);
  const u32 nb = (n + SBLK - 1) / SBLK;
  // code_off needs n + 1 slots for the scan total: scratch, then copy the first n
  Scratch sc(s);
  if (!sc.alloc(8ull * (n + 1) + 8ull * (nb + 1) + 16)) return RC_E_DEVICE;
  u64* coff = (u64*)sc.p;
  u64* tmp = coff + (n + 1);
  u32* bad = reinterpret_cast<u32*>(tmp + nb + 1);
  hipError_t e = hipMemsetAsync(bad, 0, 4, s);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(k_unpack_index, dim3((n + SWG - 1) / SWG), dim3(SWG), 0, s, index, n,
                       code_len_dev, bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = device_scan(s, index, n, SCAN_SRC_STRIDE2_PAD16, 1, info->payload_off, coff, tmp);
  if (e == hipSuccess) e = device_scan(s, index, n, SCAN_SRC_STRIDE2, 0, 0, sym_off_dev, tmp);
  if (e == hipSuccess && n)
    e = hipMemcpyAsync(code_off_dev, coff, 8ull * n, hipMemcpyDeviceToDevice, s);
  u64* ends = (u64*)rc_pinned_scratch_(24);  // small read-backs through pinned memory
  if (!ends) return RC_E_DEVICE;
  ends[0] = ends[1] = ends[2] = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&ends[0], coff + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && n) e = hipMemcpyAsync(&ends[1], sym_off_dev + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&ends[2], bad, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return RC_E_DEVICE;
  const u32 hbad = (u32)ends[2];
  // the index must describe exactly the payload the header announces
  if (hbad || ends[0] != info->payload_off + info->payload_bytes || ends[1] != info->n_syms)
    return RC_E_BAD_CONTAINER;
  return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// RCB2 (include/range_coder.h): order-1 sets and wide models, per-chunk checksums
// ------------------------------------------------------------------------------------------
namespace {
const u32 C2_MARK = 0x32424352u;  // "RCB2" as a little-endian u32: rc_container2_info.reserved
// the largest table section: 64 rows of 256 u32 and a 256-byte map
const size_t C2_TABLE_MAX = 4ull * RC_MAX_SET_MODELS * 256 + 256;
// pinned staging of pack / model: [0, 64) read-backs, [64, ...) header + table as stored, then
// the model's rows as the device holds them (64 cum rows of 257 u32 and the 256-byte map)
const size_t C2_PIN_OUT = 64;
const size_t C2_PIN_RAW = C2_PIN_OUT + RC_CONTAINER_HEADER_BYTES + C2_TABLE_MAX + 16;
const size_t C2_PIN_BYTES = C2_PIN_RAW + 4ull * RC_MAX_SET_MODELS * 257 + 256;

u64 c2_table_bytes(u32 kind, u32 nsym, u32 k) {
  switch (kind) {
    case 0:
    case 3: return hpad16(4ull * nsym);
    case 2: return hpad16(4ull * k * nsym + nsym);
    default: return 0;
  }
}

const rc_container2_info* c2_info(const void* p) {
  const rc_container2_info* in = static_cast<const rc_container2_info*>(p);
  return in && in->reserved == C2_MARK ? in : nullptr;
}

// grid 0: as many workgroups as the chunks need, at most 16 per CU (k_pack_payload's shape)
hipError_t checksum_launch(hipStream_t s, int dev, const void* data, const u64* off, u32 n,
                           u32 sym_bytes, u32* sums, const u32* expect, u32* first_bad, u32 grid) {
  if (!n) return hipSuccess;
  if (!grid) {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    grid = std::min<u32>((n + SWG / 64 - 1) / (SWG / 64), (u32)std::max(cus, 1) * 16);
  }
  hipLaunchKernelGGL(k_chunk_checksum, dim3(grid), dim3(SWG), 0, s,
                     static_cast<const uint8_t*>(data), off, n, sym_bytes, sums, expect, first_bad);
  return hipGetLastError();
}
}  // namespace

extern "C" {

// host-only hook (not in the header; tests/test_gpu_container2.py): rc_checksum_batch with a
// given number of workgroups, so a test reaches the grid-stride rounds with few chunks
rc_status rc_checksum_batch_grid_(rc_ctx* ctx, const void* data_dev, const uint64_t* off_dev,
                                  uint32_t n_chunks, uint32_t sym_bytes, uint32_t* sums_dev,
                                  uint32_t grid) {
  if (!ctx || n_chunks > RC_MAX_CHUNKS || (sym_bytes != 1 && sym_bytes != 2) || grid > 65536)
    return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_chunks && (!data_dev || !off_dev || !sums_dev)) return RC_E_ARG;
  DeviceGuard g(dev);
  return checksum_launch(s, dev, data_dev, off_dev, n_chunks, sym_bytes, sums_dev, nullptr,
                         nullptr, grid) == hipSuccess
             ? RC_OK
             : RC_E_DEVICE;
}

rc_status rc_checksum_batch(rc_ctx* ctx, const void* data_dev, const uint64_t* off_dev,
                            uint32_t n_chunks, uint32_t sym_bytes, uint32_t* sums_dev) {
  return rc_checksum_batch_grid_(ctx, data_dev, off_dev, n_chunks, sym_bytes, sums_dev, 0);
}

rc_status rc_container2_info_parse(const uint8_t* head, uint64_t head_len, void* info2) {
  if (!head || !info2) return RC_E_ARG;
  if (head_len < RC_CONTAINER_HEADER_BYTES) return RC_E_BAD_CONTAINER;
  if (memcmp(head, "RCB2", 4) != 0) return RC_E_BAD_CONTAINER;
  rc_container2_info in;
  memset(&in, 0, sizeof in);
  const u32 vh = get32(head + 4);
  in.version = vh & 0xFFFF;
  if (in.version != 1 || (vh >> 16) != RC_CONTAINER_HEADER_BYTES) return RC_E_BAD_CONTAINER;
  in.reserved = C2_MARK;
  in.kind = get32(head + 8);
  in.n_symbols = get32(head + 12);
  in.total_freq = get32(head + 16);
  if (in.kind > 3) return RC_E_BAD_CONTAINER;
  if (in.kind == 1) {
    in.increment = get32(head + 20);
    in.limit = get32(head + 24);
    in.period = get32(head + 28);
  } else if (in.kind == 2) {
    in.n_models = get32(head + 20);
    in.first_row = get32(head + 24);
    if (in.n_models < 1 || in.n_models > RC_MAX_SET_MODELS || in.first_row >= in.n_models)
      return RC_E_BAD_CONTAINER;
  }
  in.n_chunks = get64(head + 32);
  in.n_syms = get64(head + 40);
  in.payload_bytes = get64(head + 48);
  in.flags = get32(head + 56);
  in.sym_bytes = in.kind == 3 ? 2 : 1;
  if (in.n_symbols < 1 || in.n_symbols > (in.kind == 3 ? RC_MAX_WIDE_SYMBOLS : 256u) ||
      in.n_chunks > RC_MAX_CHUNKS || (in.flags & ~RC_CONTAINER2_F_CHECKSUMS))
    return RC_E_BAD_CONTAINER;
  if (in.payload_bytes & 15 || in.payload_bytes > (1ull << 56)) return RC_E_BAD_CONTAINER;
  in.table_off = RC_CONTAINER_HEADER_BYTES;
  in.index_off = in.table_off + c2_table_bytes(in.kind, in.n_symbols, in.n_models);
  in.sum_off = in.index_off + 16 * in.n_chunks;
  in.payload_off = in.sum_off + (in.flags & RC_CONTAINER2_F_CHECKSUMS ? hpad16(4 * in.n_chunks) : 0);
  in.container_bytes = in.payload_off + in.payload_bytes;
  memcpy(info2, &in, sizeof in);
  return RC_OK;
}

rc_status rc_container2_pack(rc_ctx* ctx, const rc_model* m, const uint8_t* slots_dev,
                             const uint64_t* slot_off_dev, const uint64_t* code_len_dev,
                             const uint64_t* sym_off_dev, uint32_t n_chunks,
                             const uint32_t* sums_dev, uint8_t* dst_dev, uint64_t dst_cap,
                             uint64_t* dst_len_host) {
  if (!ctx || !m || !dst_len_host || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  if (n_chunks && (!slots_dev || !slot_off_dev || !code_len_dev || !sym_off_dev)) return RC_E_ARG;
  // what the model is: kind, sizes, and where its table comes from
  int kind = m->kind;
  u32 nsym = 0, total = 0, inc = 0, lim = 0, per = 0, k_rows = 0, first_row = 0;
  const u32 *c_host = nullptr, *rows_dev = nullptr;
  const uint8_t* map_dev = nullptr;
  // (a static set is not among them: it has no index stream to frame)
  if (!rc_model_kind_ok(m, RC_KINDS_SINGLE | 1u << RC_KIND_WIDE | 1u << RC_KIND_ORDER1))
    return RC_E_ARG;
  if (kind == RC_KIND_ORDER1) {
    // (RCB2 frames one map: a periodic order-1 set would lose its period, a lagged one its lag)
    if (m->o1.period > 1 || m->o1_lag > 1) return RC_E_ARG;
    kind = 2;
    rows_dev = m->o1.s.rows, map_dev = m->o1.map;
    first_row = m->o1.first_row, k_rows = m->o1.s.k, nsym = m->o1.s.m.n;
  } else if (kind == RC_KIND_WIDE) {
    kind = 3;
    rows_dev = m->wide.row, nsym = m->wide.m.n;
  } else {
    nsym = kind == 0 ? m->args.n : m->ap.n, total = m->args.total, c_host = m->c_host;
    inc = m->ap.inc, lim = m->ap.limit, per = m->period;
  }
  if (m->device != dev || nsym < 1 || nsym > (kind == 3 ? RC_MAX_WIDE_SYMBOLS : 256u) ||
      (kind == 2 && (k_rows < 1 || k_rows > RC_MAX_SET_MODELS)))
    return RC_E_ARG;
  DeviceGuard g(dev);
  rc_svc_yield_all_();
  const u64 index_off = RC_CONTAINER_HEADER_BYTES + c2_table_bytes((u32)kind, nsym, k_rows);
  const u64 sum_off = index_off + 16ull * n_chunks;
  const u64 payload_off = sum_off + (sums_dev ? hpad16(4ull * n_chunks) : 0);
  const u32 nb = (n_chunks + SBLK - 1) / SBLK;
  Scratch sc(s);
  if (!sc.alloc(8ull * (n_chunks + 1) * 2 + 8ull * (nb + 1))) return RC_E_DEVICE;
  u64* doff = (u64*)sc.p;
  u64* soff = doff + (n_chunks + 1);
  u64* tmp = soff + (n_chunks + 1);
  hipError_t e = device_scan(s, code_len_dev, n_chunks, SCAN_SRC_PAD16, 0, payload_off, doff, tmp);
  if (e == hipSuccess) e = device_scan(s, sym_off_dev, n_chunks, SCAN_SRC_DIFF, 0, 0, soff, tmp);
  char* pin = (char*)rc_pinned_scratch_(C2_PIN_BYTES);
  if (!pin) return RC_E_DEVICE;
  u64* ends = (u64*)pin;
  ends[0] = payload_off;
  ends[1] = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&ends[0], doff + n_chunks, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&ends[1], soff + n_chunks, 8, hipMemcpyDeviceToHost, s);
  // the device's cum rows (order-1: k_rows x 257 and the staged map; wide: nsym + 1)
  u32* raw = (u32*)(pin + C2_PIN_RAW);
  uint8_t* raw_map = (uint8_t*)(raw + (size_t)RC_MAX_SET_MODELS * 257);
  if (e == hipSuccess && kind == 2) {
    e = hipMemcpyAsync(raw, rows_dev, 4ull * k_rows * 257, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(raw_map, map_dev, 256, hipMemcpyDeviceToHost, s);
  } else if (e == hipSuccess && kind == 3) {
    e = hipMemcpyAsync(raw, rows_dev, 4ull * (nsym + 1), hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return RC_E_DEVICE;
  const u64 total_bytes = ends[0];
  *dst_len_host = total_bytes;
  if (!dst_dev || total_bytes > dst_cap) return RC_E_CAPACITY;
  uint8_t* head = (uint8_t*)pin + C2_PIN_OUT;
  memset(head, 0, index_off);
  uint8_t* tab = head + RC_CONTAINER_HEADER_BYTES;
  if (kind == 0) {
    for (u32 i = 0; i < nsym; ++i) put32(tab + 4 * i, c_host[i]);
  } else if (kind == 2) {
    total = raw[256];  // (a row's entries from nsym on hold the total)
    for (u32 r = 0; r < k_rows; ++r)
      for (u32 i = 0; i < nsym; ++i)
        put32(tab + 4 * ((size_t)r * nsym + i), raw[r * 257 + i + 1] - raw[r * 257 + i]);
    memcpy(tab + 4ull * k_rows * nsym, raw_map, nsym);
  } else if (kind == 3) {
    total = raw[nsym];
    for (u32 i = 0; i < nsym; ++i) put32(tab + 4 * i, raw[i + 1] - raw[i]);
  }
  memcpy(head, "RCB2", 4);
  put32(head + 4, 1u | ((u32)RC_CONTAINER_HEADER_BYTES << 16));
  put32(head + 8, (u32)kind);
  put32(head + 12, nsym);
  put32(head + 16, kind == 1 ? 0u : total);
  put32(head + 20, kind == 1 ? inc : kind == 2 ? k_rows : 0u);
  put32(head + 24, kind == 1 ? lim : kind == 2 ? first_row : 0u);
  put32(head + 28, kind == 1 ? per : 0u);
  put64(head + 32, n_chunks);
  put64(head + 40, ends[1]);
  put64(head + 48, total_bytes - payload_off);
  put32(head + 56, sums_dev ? RC_CONTAINER2_F_CHECKSUMS : 0u);
  if (hipMemcpyAsync(dst_dev, head, index_off, hipMemcpyHostToDevice, s) != hipSuccess)
    return RC_E_DEVICE;
  if (sums_dev && n_chunks) {
    const u64 nb4 = 4ull * n_chunks;
    if (hipMemcpyAsync(dst_dev + sum_off, sums_dev, nb4, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return RC_E_DEVICE;
    if (hpad16(nb4) > nb4 &&
        hipMemsetAsync(dst_dev + sum_off + nb4, 0, hpad16(nb4) - nb4, s) != hipSuccess)
      return RC_E_DEVICE;
  }
  if (n_chunks) {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const u32 grid = std::min<u32>((n_chunks + SWG / 64 - 1) / (SWG / 64), (u32)std::max(cus, 1) * 16);
    hipLaunchKernelGGL(k_pack_payload, dim3(grid), dim3(SWG), 0, s, slots_dev, slot_off_dev,
                       code_len_dev, sym_off_dev, n_chunks, dst_dev, doff,
                       reinterpret_cast<u64*>(dst_dev + index_off));
    if (hipGetLastError() != hipSuccess) return RC_E_DEVICE;
  }
  // the pinned staging is reused by this thread's next call: wait for its copy
  return hipStreamSynchronize(s) == hipSuccess ? RC_OK : RC_E_DEVICE;
}

rc_status rc_container2_offsets(rc_ctx* ctx, const uint8_t* container_dev, const void* info2,
                                uint64_t* code_off_dev, uint64_t* code_len_dev,
                                uint64_t* sym_off_dev) {
  const rc_container2_info* in = c2_info(info2);
  if (!in) return RC_E_ARG;
  // (rc_container2_info begins with rc_container_info's fields, and the index and the payload
  // are RCB1's)
  rc_container_info v1;
  memcpy(&v1, in, sizeof v1);
  return rc_container_offsets(ctx, container_dev, &v1, code_off_dev, code_len_dev, sym_off_dev);
}

rc_status rc_container2_model(rc_ctx* ctx, const uint8_t* container_dev, const void* info2,
                              rc_model** out) {
  const rc_container2_info* in = c2_info(info2);
  if (!ctx || !container_dev || !in || !out) return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  *out = nullptr;
  const u32 n = in->n_symbols, k = in->kind == 2 ? in->n_models : 1;
  if (in->kind > 3 || n < 1 || n > (in->kind == 3 ? RC_MAX_WIDE_SYMBOLS : 256u) || k < 1 ||
      k > RC_MAX_SET_MODELS || in->index_off != in->table_off + c2_table_bytes(in->kind, n, k))
    return RC_E_BAD_CONTAINER;
  rc_status rc;
  if (in->kind == 1) {
    rc = rc_model_create_adaptive(ctx, n, in->increment, in->limit, in->period, out);
    return rc == RC_E_BAD_MODEL ? RC_E_BAD_CONTAINER : rc;
  }
  DeviceGuard g(dev);
  char* pin = (char*)rc_pinned_scratch_(C2_PIN_BYTES);
  if (!pin) return RC_E_DEVICE;
  const u64 tbytes = in->index_off - in->table_off;
  if (hipMemcpyAsync(pin + C2_PIN_OUT, container_dev + in->table_off, tbytes,
                     hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return RC_E_DEVICE;
  // c as stored, cum by calc_cum (mod 2^32: a table that overflows does not sum to its total)
  // (copied out of the staging, which the next user of this thread's pinned buffer may move)
  const uint8_t* tab = (const uint8_t*)pin + C2_PIN_OUT;
  std::vector<u32> cv((size_t)k * n), cumv((size_t)k * n);
  std::vector<uint8_t> map(tab + 4ull * k * n, tab + 4ull * k * n + (in->kind == 2 ? n : 0));
  u32 *c = cv.data(), *cum = cumv.data();
  for (u32 r = 0; r < k; ++r) {
    u32 run = 0;
    for (u32 i = 0; i < n; ++i) {
      const u32 v = get32(tab + 4 * ((size_t)r * n + i));
      c[(size_t)r * n + i] = v;
      cum[(size_t)r * n + i] = run;
      run += v;
    }
  }
  if (in->kind == 0)
    rc = rc_model_create_static(ctx, n, c, cum, in->total_freq, out);
  else if (in->kind == 3)
    rc = rc_model_create_static_wide(ctx, n, c, cum, in->total_freq, out);
  else
    rc = rc_model_create_order1_set(ctx, k, n, c, cum, in->total_freq, map.data(), in->first_row,
                                    out);
  return rc == RC_E_BAD_MODEL ? RC_E_BAD_CONTAINER : rc;
}

rc_status rc_container2_verify(rc_ctx* ctx, const uint8_t* container_dev, const void* info2,
                               const void* syms_dev, const uint64_t* sym_off_dev,
                               uint64_t* first_bad_host) {
  const rc_container2_info* in = c2_info(info2);
  if (!ctx || !container_dev || !in || !first_bad_host || in->n_chunks > RC_MAX_CHUNKS ||
      (in->sym_bytes != 1 && in->sym_bytes != 2))
    return RC_E_ARG;
  const hipStream_t s = ctx->cur;
  const int dev = ctx->device;
  const u32 n = (u32)in->n_chunks;
  *first_bad_host = n;
  if (!(in->flags & RC_CONTAINER2_F_CHECKSUMS) || !n) return RC_OK;
  if (!syms_dev || !sym_off_dev) return RC_E_ARG;
  DeviceGuard g(dev);
  Scratch sc(s);
  if (!sc.alloc(16)) return RC_E_DEVICE;
  u32* bad = (u32*)sc.p;
  u32* back = (u32*)rc_pinned_scratch_(16);
  if (!back) return RC_E_DEVICE;
  back[0] = 0xFFFFFFFFu;
  hipError_t e = hipMemsetAsync(bad, 0xFF, 4, s);
  if (e == hipSuccess)
    e = checksum_launch(s, dev, syms_dev, sym_off_dev, n, in->sym_bytes, nullptr,
                        reinterpret_cast<const u32*>(container_dev + in->sum_off), bad, 0);
  if (e == hipSuccess) e = hipMemcpyAsync(back, bad, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return RC_E_DEVICE;
  if (back[0] == 0xFFFFFFFFu) return RC_OK;
  *first_bad_host = back[0];
  return RC_E_CHECKSUM;
}

}  // extern "C"
