// rc_kernels.hip — host side of the static-model coder (contexts, models, launches) and the
// synthetic workload generator.  The kernels: rc_encode.hip, rc_decode.inc (rc_static.h).  The
// context and the model themselves: rc_host.h.
#include "rc_host.h"

// ------------------------------------------------------------------------------------------
// Synthetic workload generator (inputs for bench/tests, generated directly in HBM)
// ------------------------------------------------------------------------------------------
static __device__ __forceinline__ u64 mix64(u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(WG) void k_synth(u64 seed, const uint8_t* __restrict__ inv,
                                             uint8_t* __restrict__ dst, u64 chunk_len,
                                             u64 total_words) {
  // one item = 16 symbols = 4 splitmix words; grid-stride (a launch is capped at 2^32 items)
  RC_VGPR_FLOOR_64();
  const u64 words_per_chunk = chunk_len >> 4;
  for (u64 g = (u64)blockIdx.x * WG + threadIdx.x; g < total_words; g += (u64)gridDim.x * WG) {
    const u64 chunk = g / words_per_chunk;
    const u64 w16 = g - chunk * words_per_chunk;
    u32 o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u64 word = mix64(seed + 0x9E3779B97F4A7C15ull * ((chunk << 32) + w16 * 4 + q + 1));
      o[q] = (u32)inv[word & 0xFFFF] | ((u32)inv[(word >> 16) & 0xFFFF] << 8) |
             ((u32)inv[(word >> 32) & 0xFFFF] << 16) | ((u32)inv[(word >> 48) & 0xFFFF] << 24);
    }
    reinterpret_cast<uint4*>(dst + chunk * chunk_len)[w16] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

__global__ __launch_bounds__(WG) void k_synth_generic(u64 seed, const uint8_t* __restrict__ inv,
                                                     uint8_t* __restrict__ dst, u64 chunk_len,
                                                     u32 n_chunks) {
  // one thread per chunk, byte stores: any chunk_len / alignment (small test inputs)
  RC_VGPR_FLOOR_64();
  const u32 chunk = blockIdx.x * WG + threadIdx.x;
  if (chunk >= n_chunks) return;
  for (u64 i = 0; i < chunk_len; ++i) {
    const u64 word = mix64(seed + 0x9E3779B97F4A7C15ull * (((u64)chunk << 32) + i / 4 + 1));
    dst[(u64)chunk * chunk_len + i] = inv[(word >> (16 * (i & 3))) & 0xFFFF];
  }
}

// ------------------------------------------------------------------------------------------
// Host side: contexts, models, launches
// ------------------------------------------------------------------------------------------
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rc_wide16_tables.h"
#include "rc_wide16_fine_tables.h"

// The only place the library reads its environment (tests/test_abi.py checks that no other
// source calls getenv): once per context, in rc_ctx_create.
RcKnobs rc_knobs_from_env() {
  auto str = [](const char* name) -> const char* {
    const char* e = getenv(name);
    return e && *e ? e : nullptr;
  };
  RcKnobs k;
  const char* e;
  k.prio = !((e = str("RC_PRIO")) && !strcmp(e, "off"));
  k.dec_pair = 0;
  if ((e = str("RC_DEC_PAIR"))) {
    const long x = strtol(e, nullptr, 10);
    k.dec_pair = x == 512 || x == 1024 || x == 4 || x == 6 ? (u32)x : 0u;
  }
  k.stream_service = !((e = str("RC_STREAM_SERVICE")) && e[0] == '0');
  k.stream_dma = (e = str("RC_STREAM_DMA")) && e[0] != '0';
  k.stream_direct = !((e = str("RC_STREAM_DIRECT")) && e[0] == '0');
  k.stream_batch_bytes = (e = str("RC_STREAM_BATCH_BYTES")) ? strtoull(e, nullptr, 0) : 0ull;
  k.hist_hot = !((e = str("RC_HIST_HOT")) && e[0] == '0');
  return k;
}

namespace {

thread_local char g_last_error[256] = "";

rc_status device_error(hipError_t e, const char* what) {
  snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, hipGetErrorString(e));
  return RC_E_DEVICE;
}

rc_status launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? RC_OK : device_error(e, "kernel launch");
}

struct PinnedScratch {
  void* p = nullptr;
  size_t cap = 0;
  ~PinnedScratch() {
    if (p) (void)hipHostFree(p);
  }
};
thread_local PinnedScratch t_pinned;

}  // namespace

void* rc_pinned_scratch_(size_t bytes) {
  if (bytes > (1u << 20)) return nullptr;
  if (t_pinned.cap < bytes) {
    if (t_pinned.p) (void)hipHostFree(t_pinned.p);
    t_pinned.p = nullptr;
    t_pinned.cap = 0;
    const size_t cap = std::max<size_t>(bytes, 1u << 16);
    if (hipHostMalloc(&t_pinned.p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    t_pinned.cap = cap;
  }
  return t_pinned.p;
}

// the division a model of `total` is coded with (its kernels' DIV)
static int div_of(u32 total) { return (total & (total - 1)) == 0 ? DIV_POW2 : DIV_MAGIC; }

// range_par_total's constants for `total` (DIV_POW2's shift, DIV_MAGIC's reciprocal and the
// small models' f64 1/total rounded up)
static void div_constants(ModelArgs& a, u32 total) {
  const bool pow2 = (total & (total - 1)) == 0;
  a.total = total;
  a.lg = pow2 ? (u32)__builtin_ctz(total) : 0u;
  a.magic = ~0ull / (u64)total;
  a.inv_up = 1.0 / (double)total;  // rounded up: inv_up * total >= 1 exactly
  if (std::fma(a.inv_up, (double)total, -1.0) < 0.0) a.inv_up = std::nextafter(a.inv_up, 2.0);
}

// The decoders' bucket table of a (c, cum, total) table, 2^bits buckets at most: per bucket
// s0 | s1 << 8 | split << 16 (s0 = the symbol containing the bucket's first frequency, s1 = the
// next symbol with c > 0 starting inside the bucket, split = its offset, 0xFFFF: none), padded
// to a power of two with the last bucket (the kernels mask the bucket index)
static std::vector<u32> bucket_table(u32 n_symbols, const u32* c_freq, const u32* cum_freq,
                                     u32 total_freq, u32 bits, u32* shift_out) {
  const u32 bl = bitlen(total_freq - 1);
  const u32 shift = bl > bits ? bl - bits : 0u;
  const u32 nb = ((total_freq - 1) >> shift) + 1;
  std::vector<u32> lt(nb);
  u32 s = 0;
  for (u32 b = 0; b < nb; ++b) {
    const u64 f0 = (u64)b << shift;
    const u64 f1 = std::min<u64>((u64)(b + 1) << shift, total_freq);
    while (s + 1 < n_symbols && (u64)cum_freq[s + 1] <= f0) ++s;
    u32 s1 = s, split = 0xFFFFu;
    for (u32 t = s + 1; t < n_symbols; ++t) {
      if ((u64)cum_freq[t] >= f1) break;
      if (c_freq[t] > 0) {
        if ((u64)cum_freq[t] - f0 <= 0xFFFFu) {
          s1 = t;
          split = (u32)((u64)cum_freq[t] - f0);
        }
        break;
      }
    }
    lt[b] = s | (s1 << 8) | (split << 16);
  }
  while (lt.size() & (lt.size() - 1)) lt.push_back(lt.back());
  *shift_out = shift;
  return lt;
}

// The direct-table decoder's q-to-symbol bytes (k_decode_static LUT 6, rc_static.h) of a checked
// table with 2048 < total <= 2^16: symof[q] = the symbol s with cum[s] <= q < cum[s] + c[s] for
// every q < total (a symbol with c == 0 owns no entry), padded to a power of two with the last
// entry (the kernel masks the index, so the padding must name symbols with c > 0 too)
static std::vector<uint8_t> symof_table(u32 n_symbols, const u32* c_freq, const u32* cum_freq,
                                        u32 total_freq) {
  std::vector<uint8_t> t((size_t)1 << bitlen(total_freq - 1));
  for (u32 s = 0; s < n_symbols; ++s)
    for (u32 q = cum_freq[s]; q < cum_freq[s] + c_freq[s]; ++q) t[q] = (uint8_t)s;
  for (size_t q = total_freq; q < t.size(); ++q) t[q] = t[total_freq - 1];
  return t;
}

// rc_model_create_static's checks of one row against a given total
static bool table_ok(u32 n_symbols, const u32* c_freq, const u32* cum_freq, u32 total_freq) {
  u64 acc = 0;
  for (u32 i = 0; i < n_symbols; ++i) {
    if ((u64)cum_freq[i] != acc) return false;
    acc += c_freq[i];
  }
  return acc == (u64)total_freq;
}

// what rc_model_create_static_set accepts (include/range_coder.h)
static rc_status set_check(u32 n_models, u32 n_symbols, const u32* c, const u32* cum,
                           u32 total) {
  if (!c || !cum) return RC_E_ARG;
  if (n_models < 1 || n_models > RC_MAX_SET_MODELS || n_symbols < 1 || n_symbols > 256 ||
      total < 256 || total > 65536)
    return RC_E_BAD_MODEL;
  for (u32 j = 0; j < n_models; ++j)
    if (!table_ok(n_symbols, c + (size_t)j * n_symbols, cum + (size_t)j * n_symbols, total))
      return RC_E_BAD_MODEL;
  return RC_OK;
}

// A new model of `kind` on the context's device that owns one allocation holding the host
// segments back to back (an empty one is skipped): every other field zero, div from the total.
// *base: the allocation, segment i at the sum of the sizes before it.
struct HostSeg {
  const void* p;
  size_t bytes;
};
static rc_status model_upload(rc_ctx* ctx, int kind, u32 total, std::initializer_list<HostSeg> segs,
                              rc_model** out, char** base) {
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  size_t bytes = 0;
  for (const HostSeg& sg : segs) bytes += sg.bytes;
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return RC_E_DEVICE;
  size_t at = 0;
  for (const HostSeg& sg : segs) {
    if (sg.bytes &&
        hipMemcpy((char*)d + at, sg.p, sg.bytes, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return RC_E_DEVICE;
    }
    at += sg.bytes;
  }
  rc_model* mm = new rc_model;
  memset(mm, 0, sizeof *mm);
  mm->kind = kind;
  mm->device = ctx->device;
  mm->div = div_of(total);
  mm->dmem = d;
  *out = mm;
  *base = (char*)d;
  return RC_OK;
}

// the ModelArgs of the set, order-1 and wide kernels: the alphabet, the total's constants and the
// decoder's buckets (the table pointers stay unused)
static void small_model_args(ModelArgs& m, u32 n_symbols, u32 total, u32 bits, u32 shift) {
  m.n = n_symbols;
  m.ftotal = (float)total;
  div_constants(m, total);
  m.lut_bits = bits;
  m.lut_shift = shift;
}

// The 8 words of a plan hook (rc_model_set_plan_, rc_model_order1_plan_, rc_model_wide_plan_):
// encoder {lanes per workgroup, dynamic LDS bytes, table layout, table bytes}, decoder {lanes,
// LDS bytes, log2 buckets per table, bucket shift}.
template <class Plan, class F>
static rc_status plan_hook(bool size_ok, u32 total, uint32_t* out, F plan) {
  if (!out) return RC_E_ARG;
  if (!size_ok || total < 256 || total > 65536) return RC_E_BAD_MODEL;
  Plan p;
  plan(&p);
  const u32 v[8] = {p.enc_lanes, p.enc_lds, p.enc_layout, p.enc_tab,
                    p.dec_lanes, p.dec_lds, p.dec_bits,   p.dec_shift};
  memcpy(out, v, sizeof v);
  return RC_OK;
}

// What every rc_{encode,decode}_batch* entry point does around its launch, in this order of
// precedence: null context or model and too many chunks, a model of another kind (kinds: the
// accepted ones as bits 1 << kind; kinds do not mix), a misaligned symbol pointer (the wide
// calls' 16-bit symbols), the empty batch (RC_OK), a null array, a model of another device; then
// the device, the stream service asked to yield, the launch and its error as `what`.
template <class Launch>
static rc_status batch_call(rc_ctx* ctx, const rc_model* m, u32 kinds, bool aligned,
                            uint32_t n_chunks, bool arrays, const char* what, Launch launch) {
  if (!ctx || !m || n_chunks > RC_MAX_CHUNKS) return RC_E_ARG;
  if (!rc_model_kind_ok(m, kinds) || !aligned) return RC_E_ARG;
  if (n_chunks == 0) return RC_OK;
  if (!arrays || m->device != ctx->device) return RC_E_ARG;
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  rc_svc_yield_all_();
  const hipError_t e = launch();
  return e == hipSuccess ? RC_OK : device_error(e, what);
}

// range / total through the static coders' three range_par_total forms (rc_static.h), under
// the decoders' rounding mode (f32 toward zero, rc_decode.inc): out[3i] the small-model f64
// form, out[3i + 1] the 64 x 64 magic product, out[3i + 2] the power-of-two shift.  For
// rc_test_range_par_total_ (tests/test_gpu_div.py).
__global__ __launch_bounds__(64) void k_test_range_par_total(const u64* __restrict__ ranges,
                                                             const ModelArgs* __restrict__ ms,
                                                             u32 n, u64* __restrict__ out) {
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3");
  const u32 i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const ModelArgs m = ms[i];
  const u64 r = ranges[i];
  out[3 * i] = range_par_total<DIV_MAGIC, 1>(r, m);
  out[3 * i + 1] = range_par_total<DIV_MAGIC, 0>(r, m);
  out[3 * i + 2] = range_par_total<DIV_POW2, 0>(r, m);
}

extern "C" {

const char* rc_last_error(void) { return g_last_error; }

const char* rc_status_string(rc_status s) {
  switch (s) {
    case RC_OK: return "ok";
    case RC_E_ARG: return "invalid argument";
    case RC_E_BAD_MODEL: return "frequency table rejected";
    case RC_E_DEVICE: return "HIP runtime error";
    case RC_E_NO_DEVICE: return "no usable gfx950 device";
    case RC_E_CHUNK: return "at least one chunk flagged";
    case RC_E_BAD_CONTAINER: return "malformed container";
    case RC_E_CAPACITY: return "destination too small";
    case RC_E_BAD_SYMBOL: return "symbol outside the alphabet";
    case RC_E_CHECKSUM: return "checksum mismatch";
    default: return "unknown status";
  }
}

rc_status rc_device_info(int device, char* buf, size_t buf_len) {
  if (!buf || !buf_len) return RC_E_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RC_E_NO_DEVICE;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) return RC_E_DEVICE;
  snprintf(buf, buf_len, "%s CUs=%d LDS/CU=%zu", p.gcnArchName, p.multiProcessorCount,
           (size_t)p.maxSharedMemoryPerMultiProcessor);
  return RC_OK;
}

rc_status rc_ctx_create(int device, rc_ctx** out) {
  if (!out) return RC_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RC_E_NO_DEVICE;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) return RC_E_DEVICE;
  if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return RC_E_NO_DEVICE;
  DeviceGuard g(device);
  if (!g.ok) return RC_E_DEVICE;
  rc_ctx* c = new rc_ctx;
  c->device = device;
  c->knobs = rc_knobs_from_env();
  if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return RC_E_DEVICE;
  }
  c->cur = c->own;
  if (hipMalloc((void**)&c->inv, 65536) != hipSuccess) {
    (void)hipStreamDestroy(c->own);
    delete c;
    return RC_E_DEVICE;
  }
  *out = c;
  return RC_OK;
}

rc_status rc_ctx_destroy(rc_ctx* ctx) {
  if (!ctx) return RC_E_ARG;
  DeviceGuard g(ctx->device);
  rc_stream_release_(ctx);
  rc_resume_release_(ctx);
  (void)hipStreamSynchronize(ctx->own);
  (void)hipStreamSynchronize(ctx->cur);
  (void)hipFree(ctx->inv);
  rc_chunk_group_release(ctx->group);
  (void)hipStreamDestroy(ctx->own);
  delete ctx;
  return RC_OK;
}

rc_status rc_ctx_set_stream(rc_ctx* ctx, void* hip_stream) {
  if (!ctx) return RC_E_ARG;
  ctx->cur = (hipStream_t)hip_stream;
  return RC_OK;
}

rc_status rc_ctx_reset_stream(rc_ctx* ctx) {
  if (!ctx) return RC_E_ARG;
  ctx->cur = ctx->own;
  return RC_OK;
}

rc_status rc_ctx_synchronize(rc_ctx* ctx) {
  if (!ctx) return RC_E_ARG;
  DeviceGuard g(ctx->device);
  return hipStreamSynchronize(ctx->cur) == hipSuccess ? RC_OK : RC_E_DEVICE;
}

// Everything rc_model_create_static works out on the host for a table: the class of the model
// (a.direct, a.flat, the bucket geometry, which tables it carries), the constants
// of its total and the four segments of its device snapshot.  a's table pointers stay null: they
// are set once the segments are uploaded.  rc_model_static_plan_ and rc_bucket_table_ report from
// the same function, so a test sees the class a model really gets.
struct StaticTables {
  ModelArgs a;
  std::vector<uint2> tab;      // [256] (cum, c)
  std::vector<u32> lut;        // the class's decoder table (buckets or direct entries)
  std::vector<u32> pair;       // pair buckets, or empty
  std::vector<uint8_t> symof;  // q-to-symbol bytes, or empty
  bool complete;               // 256 symbols, every c_freq > 0
};
static rc_status static_tables(u32 n_symbols, const u32* c_freq, const u32* cum_freq,
                               u32 total_freq, StaticTables* st) {
  if (n_symbols < 1 || n_symbols > 256 || total_freq < 1) return RC_E_BAD_MODEL;
  if (!table_ok(n_symbols, c_freq, cum_freq, total_freq)) return RC_E_BAD_MODEL;

  std::vector<uint2>& tab = st->tab;
  tab.resize(256);
  for (u32 i = 0; i < 256; ++i)
    tab[i] = i < n_symbols ? make_uint2(cum_freq[i], c_freq[i]) : make_uint2(0xFFFFFFFFu, 0u);

  ModelArgs& a = st->a;
  memset(&a, 0, sizeof a);
  a.n = n_symbols;
  a.total = total_freq;
  a.ftotal = (float)total_freq;
  div_constants(a, total_freq);
  // bucket table of 2^bits buckets: s0 = symbol containing the bucket's first frequency, s1 =
  // the next symbol with c > 0 starting inside the bucket, split = its offset (0xFFFF: none);
  // padded to a power of two (the kernel masks the bucket index) with the last bucket, so
  // exactly 2^bits entries whenever total > 2048
  const u32 bl = bitlen(total_freq - 1);
  auto bucket_lut = [&](u32 bits, u32* shift_out) {
    return bucket_table(n_symbols, c_freq, cum_freq, total_freq, bits, shift_out);
  };
  a.lut_bits = total_freq <= 65536 ? SM_LUT_BITS : LUT_BITS;
  std::vector<u32>& lut = st->lut;
  lut = bucket_lut(a.lut_bits, &a.lut_shift);
  a.lut_max = (u32)lut.size() - 1;
  if (total_freq > 2048 && lut.size() != (1u << a.lut_bits)) return RC_E_BAD_MODEL;  // unreachable

  if (total_freq <= 2048) {  // direct table: q -> s | cum << 8 | c << 20
    a.direct = 1;
    a.lut_shift = 0;
    a.lut_max = total_freq - 1;
    lut.assign(total_freq, 0);
    u32 sym = 0;
    for (u32 q = 0; q < total_freq; ++q) {
      while (sym + 1 < n_symbols && cum_freq[sym + 1] <= q) ++sym;
      lut[q] = sym | (cum_freq[sym] << 8) | (c_freq[sym] << 20);
    }
    while (lut.size() & (lut.size() - 1)) lut.push_back(lut.back());  // pow2 (masked index)
    a.lut_max = (u32)lut.size() - 1;
    if (total_freq >= 256 && total_freq <= 512) {  // 16-B entries {cum, c, s, 0}
      a.direct = 2;
      std::vector<u32> wide(4 * lut.size());
      for (size_t q = 0; q < lut.size(); ++q) {
        const u32 sq = lut[q] & 255u;
        wide[4 * q + 0] = cum_freq[sq];
        wide[4 * q + 1] = c_freq[sq];
        wide[4 * q + 2] = sq;
        const float tcf = (float)total_freq / (float)c_freq[sq];
        memcpy(&wide[4 * q + 3], &tcf, sizeof tcf);
      }
      lut.swap(wide);
    }
    // the flat model (raw bytes: configs[1]): cum[s] = s and c = 1 for every symbol
    bool flat = n_symbols == 256 && total_freq == 256;
    for (u32 i = 0; flat && i < 256; ++i) flat = c_freq[i] == 1;
    a.flat = flat ? 1u : 0u;
  }
  // pair buckets (k_decode_static LUT 3, rc_static.h): 2^15 < total <= 2^16, so buckets of 16
  // frequencies, and every c < 2^16 (16-bit fields).  Per bucket both candidates of its bucket
  // entry: s0 (holding the bucket's first frequency) and s1 (the next symbol with c > 0 that
  // starts inside the bucket; none: s1 = s0, so the choice between them does not matter).
  std::vector<u32>& pair = st->pair;
  pair.clear();
  u32 cmax = 0;
  for (u32 i = 0; i < n_symbols; ++i) cmax = std::max(cmax, c_freq[i]);
  if (!a.direct && total_freq > 32768 && total_freq <= 65536 && cmax < 65536) {
    pair.assign(PAIR_WORDS, 0);
    uint16_t* sp = (uint16_t*)pair.data();
    u32* ent = pair.data() + PAIR_S_WORDS;
    auto tcb = [&](u32 sym) {
      const float tcf = c_freq[sym] ? (float)total_freq / (float)c_freq[sym] : 0.0f;
      u32 b;
      memcpy(&b, &tcf, 4);
      return b;
    };
    u32 pshift = 0;
    const std::vector<u32> plut = bucket_lut(LUT_BITS, &pshift);  // 2^12 buckets of 16
    if (pshift != 4 || plut.size() != PAIR_BUCKETS) return RC_E_BAD_MODEL;  // unreachable
    for (u32 b = 0; b < PAIR_BUCKETS; ++b) {
      const u32 e = plut[b];  // (padded buckets repeat the last)
      const u32 s0 = e & 255u, s1 = (e >> 8) & 255u;  // (s1 = s0 where there is no split)
      sp[b] = (uint16_t)(s0 | s1 << 8);
      ent[4 * b + 0] = cum_freq[s0] | c_freq[s0] << 16;
      ent[4 * b + 1] = cum_freq[s1] | c_freq[s1] << 16;
      ent[4 * b + 2] = tcb(s0);
      ent[4 * b + 3] = tcb(s1);
    }
  }
  // small bucket models (the decoder's LUT 4, rc_static.h): 8-B buckets {16 s0 | 16 s1 << 16,
  // 0x4B400000 + cum[s1]} (s1's absolute cum; 0 without a split, where s1 = s0), at most
  // 2^SMB_LUT_BITS of them and at least 8 frequencies each, so the bucket's byte address is
  // (q >> la_shift) & la_mask with la_shift = lut_shift - 3 >= 0
  if (!a.direct && total_freq <= 65536) {
    const u32 bits = std::min<u32>(SMB_LUT_BITS, bl - 3);  // (total > 2048: bl >= 12)
    u32 shift = 0;
    const std::vector<u32> lt = bucket_lut(bits, &shift);
    if (shift < 3 || lt.size() != (1u << bits)) return RC_E_BAD_MODEL;  // unreachable
    std::vector<u32> l8(2 * lt.size());
    for (size_t b = 0; b < lt.size(); ++b) {
      const u32 e = lt[b], s0 = e & 255u, s1 = (e >> 8) & 255u, split = e >> 16;
      // (padded buckets repeat the last real one, (total - 1) >> shift)
      const u32 br = (u32)std::min<size_t>(b, (total_freq - 1) >> shift);
      // (as hint_floor's bits, 0x4B400000 + cum[s1]: the decoder compares the hint's raw bits)
      const u32 cum1 = 0x4B400000u + (split == 0xFFFFu ? 0u : (br << shift) + split);
      l8[2 * b] = 16 * s0 | (16 * s1) << 16;
      l8[2 * b + 1] = cum1;
    }
    a.lut_bits = bits;
    a.lut_shift = shift;
    a.la_shift = shift - 3;
    a.la_mask = ((u32)lt.size() - 1) << 3;
    a.la_magic = ldexpf(1.5f, 23 + (int)a.la_shift);
    a.lut_max = (u32)lt.size() - 1;
    lut.swap(l8);
  }
  // the same class through the direct q-to-symbol table (the decoder's LUT 6)
  std::vector<uint8_t>& symof = st->symof;
  symof.clear();
  if (!a.direct && total_freq <= 65536) {
    symof = symof_table(n_symbols, c_freq, cum_freq, total_freq);
    a.symof_mask = (u32)symof.size() - 1;
  }
  st->complete = n_symbols == 256;
  for (u32 i = 0; i < n_symbols; ++i) st->complete = st->complete && c_freq[i] > 0;
  return RC_OK;
}

// The encoder variant of a static model (k_encode_static's SM): 0 outside the small-model range,
// there 1 for an alphabet with a symbol the coder can reject and 2 for a complete one.  (The flat
// model runs variant 3 whatever this says: rc_static_encode_launch reads a.flat.)
static int static_smv(const ModelArgs& a, bool complete) {
  return rc_static_sm(a.total) ? (complete ? 2 : 1) : 0;
}

rc_status rc_model_create_static(rc_ctx* ctx, uint32_t n_symbols, const uint32_t* c_freq,
                                 const uint32_t* cum_freq, uint32_t total_freq, rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !out) return RC_E_ARG;
  *out = nullptr;
  StaticTables st;
  const rc_status built = static_tables(n_symbols, c_freq, cum_freq, total_freq, &st);
  if (built != RC_OK) return built;
  ModelArgs& a = st.a;
  const size_t tab_bytes = 256 * sizeof(uint2);
  const size_t lut_bytes = st.lut.size() * sizeof(u32);
  const size_t pair_bytes = st.pair.size() * sizeof(u32);
  rc_model* mm = nullptr;
  char* d = nullptr;
  const rc_status up = model_upload(
      ctx, RC_KIND_STATIC, total_freq,
      {{st.tab.data(), tab_bytes}, {st.lut.data(), lut_bytes}, {st.pair.data(), pair_bytes},
       {st.symof.data(), st.symof.size()}},
      &mm, &d);
  if (up != RC_OK) return up;
  a.tab = (const uint2*)d;
  a.lut = (const u32*)(d + tab_bytes);
  a.pair = pair_bytes ? (const u32*)(d + tab_bytes + lut_bytes) : nullptr;
  // (every segment before it is a multiple of 16 B long: the kernel copies the table as words)
  a.symof = st.symof.empty() ? nullptr
                             : (const uint8_t*)(d + tab_bytes + lut_bytes + pair_bytes);
  mm->args = a;
  for (u32 i = 0; i < n_symbols; ++i) mm->c_host[i] = c_freq[i];
  mm->complete = st.complete;
  *out = mm;
  return RC_OK;
}

rc_status rc_model_create_adaptive(rc_ctx* ctx, uint32_t n_symbols, uint32_t increment,
                                   uint32_t limit, uint32_t period, rc_model** out) {
  if (!ctx || !out) return RC_E_ARG;
  *out = nullptr;
  const u64 grow = (u64)increment * period;  // total growth between two halving checks
  if (n_symbols < 1 || n_symbols > 256 || increment < 1 || period < 1 || period > 65536 ||
      (period & (period - 1)) != 0 || grow + n_symbols > limit || limit + grow > 65535)
    return RC_E_BAD_MODEL;
  // range_par_total (range_coder.rs:38-40) divides by a total that changes every symbol: the
  // kernels multiply by floor((2^64 - 1) / total) from this table (exact after one correction)
  std::vector<u64> magic(65536, 0);
  for (u32 t = 1; t < 65536; ++t) magic[t] = ~0ull / t;
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  void* d = nullptr;
  if (hipMalloc(&d, magic.size() * sizeof(u64)) != hipSuccess) return RC_E_DEVICE;
  if (hipMemcpy(d, magic.data(), magic.size() * sizeof(u64), hipMemcpyHostToDevice) !=
      hipSuccess) {
    (void)hipFree(d);
    return RC_E_DEVICE;
  }
  rc_model* mm = new rc_model;
  memset(mm, 0, sizeof *mm);
  mm->kind = 1;
  mm->device = ctx->device;
  mm->dmem = d;
  mm->ap = AdaptParams{n_symbols, increment, limit, period - 1, (const u64*)d};
  mm->period = period;
  *out = mm;
  return RC_OK;
}

rc_status rc_model_destroy(rc_model* m) {
  if (!m) return RC_E_ARG;
  DeviceGuard g(m->device);
  if (m->dmem) (void)hipFree(m->dmem);
  delete m;
  return RC_OK;
}

rc_status rc_encode_batch(rc_ctx* ctx, const rc_model* m, const uint8_t* syms,
                          const uint64_t* sym_off, uint32_t n_chunks, uint8_t* out,
                          const uint64_t* out_off, uint64_t* out_len, uint32_t* flags) {
  // (a static model set is coded by the indexed calls only, a wide model by the wide calls only)
  return batch_call(
      ctx, m, RC_KINDS_SINGLE, true, n_chunks,
      syms && sym_off && out && out_off && out_len && flags,
      m && m->kind == RC_KIND_ADAPTIVE ? "adaptive encode launch" : "encode launch", [&] {
        if (m->kind == RC_KIND_ADAPTIVE)
          return rc_adaptive_encode_launch(ctx->cur, m->ap, syms, sym_off, n_chunks, out, out_off,
                                           out_len, flags);
        const int smv = static_smv(m->args, m->complete);
        return rc_static_encode_launch(ctx->cur, ctx->knobs, m->args, m->div, smv, syms, sym_off,
                                       n_chunks, out, out_off, out_len, flags);
      });
}

rc_status rc_decode_batch(rc_ctx* ctx, const rc_model* m, const uint8_t* code,
                          const uint64_t* code_off, const uint64_t* code_len, uint8_t* syms_out,
                          const uint64_t* sym_off, uint32_t n_chunks, uint32_t* flags) {
  return batch_call(
      ctx, m, RC_KINDS_SINGLE, true, n_chunks,
      code && code_off && code_len && syms_out && sym_off && flags,
      m && m->kind == RC_KIND_ADAPTIVE ? "adaptive decode launch" : "decode launch", [&] {
        if (m->kind == RC_KIND_ADAPTIVE)
          return rc_adaptive_decode_launch(ctx->cur, m->ap, code, code_off, code_len, syms_out,
                                           sym_off, n_chunks, flags);
        const bool sm = rc_static_sm(m->args.total);
        return m->div == DIV_POW2
                   ? rc_static_decode_launch_pow2(ctx->cur, ctx->knobs, m->args, sm, code,
                                                  code_off, code_len, syms_out, sym_off, n_chunks,
                                                  flags)
                   : rc_static_decode_launch_magic(ctx->cur, ctx->knobs, m->args, sm, code,
                                                   code_off, code_len, syms_out, sym_off, n_chunks,
                                                   flags);
      });
}

// Internal test hook (not in include/range_coder.h; host only, no device needed): the
// q-to-symbol table rc_model_create_static builds for a model of the direct-table decoder's class
// (2048 < total <= 2^16), into out[0 .. cap); *size: its length, a power of two >= total.
rc_status rc_symof_table_(uint32_t n_symbols, const uint32_t* c_freq, const uint32_t* cum_freq,
                          uint32_t total_freq, uint8_t* out, uint32_t cap, uint32_t* size) {
  if (!c_freq || !cum_freq || !out || !size) return RC_E_ARG;
  if (n_symbols < 1 || n_symbols > 256 || total_freq <= 2048 || total_freq > 65536 ||
      !table_ok(n_symbols, c_freq, cum_freq, total_freq))
    return RC_E_BAD_MODEL;
  const std::vector<uint8_t> t = symof_table(n_symbols, c_freq, cum_freq, total_freq);
  *size = (u32)t.size();
  if (t.size() > cap) return RC_E_ARG;
  memcpy(out, t.data(), t.size());
  return RC_OK;
}

// Internal test hook (host only): the class rc_model_create_static sorts a table into, as the
// launchers read it.  out[9] = {sm (the kernels' SM variants), direct (0 buckets,
// 1 4-byte direct entries, 2 16-byte direct entries), flat, has_pair, has_symof, lut_bits,
// lut_shift, div (0 DIV_POW2, 1 DIV_MAGIC), the encoder variant rc_encode_batch launches (0
// wide, 1 small and incomplete, 2 small and complete, 3 flat)}.
rc_status rc_model_static_plan_(uint32_t n_symbols, const uint32_t* c_freq,
                                const uint32_t* cum_freq, uint32_t total_freq, uint32_t* out) {
  if (!c_freq || !cum_freq || !out) return RC_E_ARG;
  StaticTables st;
  const rc_status built = static_tables(n_symbols, c_freq, cum_freq, total_freq, &st);
  if (built != RC_OK) return built;
  const ModelArgs& a = st.a;
  const u32 v[9] = {(u32)rc_static_sm(a.total), a.direct, a.flat, (u32)!st.pair.empty(),
                    (u32)!st.symof.empty(), a.lut_bits, a.lut_shift, (u32)div_of(a.total),
                    a.flat ? 3u : (u32)static_smv(a, st.complete)};
  memcpy(out, v, sizeof v);
  return RC_OK;
}

// Internal test hook (host only): the bucket words s0 | s1 << 8 | split << 16 that the wide
// bucket decoder (k_decode_static LUT 0) gets for a model of total > 2^16, into out[0 .. cap);
// *size: their number (2^LUT_BITS).
rc_status rc_bucket_table_(uint32_t n_symbols, const uint32_t* c_freq, const uint32_t* cum_freq,
                           uint32_t total_freq, uint32_t* out, uint32_t cap, uint32_t* size) {
  if (!c_freq || !cum_freq || !out || !size) return RC_E_ARG;
  StaticTables st;
  const rc_status built = static_tables(n_symbols, c_freq, cum_freq, total_freq, &st);
  if (built != RC_OK) return built;
  if (rc_static_sm(st.a.total) || st.a.direct) return RC_E_BAD_MODEL;
  *size = (u32)st.lut.size();
  if (st.lut.size() > cap) return RC_E_ARG;
  memcpy(out, st.lut.data(), st.lut.size() * sizeof(u32));
  return RC_OK;
}

// ---- static model sets (rc_indexed.h; kernels in rc_indexed.hip) ----

// Internal test hooks (not in include/range_coder.h; host only, no device needed).
// rc_model_set_check_: rc_model_create_static_set's validation of its tables.
rc_status rc_model_set_check_(uint32_t n_models, uint32_t n_symbols, const uint32_t* c_freq,
                              const uint32_t* cum_freq, uint32_t total_freq) {
  return set_check(n_models, n_symbols, c_freq, cum_freq, total_freq);
}
// rc_model_set_plan_: what the launchers use for a set of n_models rows of total total_freq (a
// launch too small to reach every CU with such workgroups runs fewer lanes, rc_indexed.hip),
// out[8] = encoder {lanes per workgroup, dynamic LDS bytes, table layout (0: 8-B (cum, c)
// entries, 1: cum-only rows), table bytes}, decoder {lanes, LDS bytes, log2 buckets per row,
// bucket shift}.
rc_status rc_model_set_plan_(uint32_t n_models, uint32_t total_freq, uint32_t* out) {
  return plan_hook<SetPlan>(n_models >= 1 && n_models <= RC_MAX_SET_MODELS, total_freq, out,
                            [&](SetPlan* p) { rc_set_plan(n_models, total_freq, p); });
}

// The device snapshot of a checked set for `plan` (rc_set_plan's, or rc_order1_plan's with maps:
// the period x 256 context-map bytes of an order-1 set, kept behind the tables, and its lag)
static rc_status set_build(rc_ctx* ctx, int kind, uint32_t n_models, uint32_t n_symbols,
                           const uint32_t* c_freq, const uint32_t* cum_freq, uint32_t total_freq,
                           const SetPlan& plan, const uint8_t* maps, uint32_t period,
                           uint32_t lag, uint32_t first_row, rc_model** out) {
  if (!plan.enc_lanes || !plan.dec_lanes) return RC_E_BAD_MODEL;  // unreachable
  // cum rows, cum[0 .. 256] with the entries from n_symbols on holding the total (so a symbol
  // past the alphabet has c = 0 in the encoder's cum-only layout), and the rows' buckets
  // s0 | s1 << 8 | cum[s1] << 16 (s1 = s0 and cum 0 where no symbol starts inside the bucket)
  const u32 nb = 1u << plan.dec_bits;
  std::vector<u32> rows((size_t)n_models * SET_ROW_WORDS), lut((size_t)n_models * nb);
  for (u32 j = 0; j < n_models; ++j) {
    const u32* c = c_freq + (size_t)j * n_symbols;
    const u32* cum = cum_freq + (size_t)j * n_symbols;
    u32* row = rows.data() + (size_t)j * SET_ROW_WORDS;
    for (u32 s = 0; s < SET_ROW_WORDS; ++s) row[s] = s < n_symbols ? cum[s] : total_freq;
    u32 shift = 0;
    const std::vector<u32> lt = bucket_table(n_symbols, c, cum, total_freq, plan.dec_bits, &shift);
    if (shift != plan.dec_shift || lt.size() > nb) return RC_E_BAD_MODEL;  // unreachable
    const u32 last = (total_freq - 1) >> shift;  // (padded buckets repeat the last real one)
    for (u32 b = 0; b < nb; ++b) {
      const u32 br = std::min(b, last);
      const u32 e = lt[std::min<size_t>(br, lt.size() - 1)];
      const u32 split = e >> 16;
      const u32 cum1 = split == 0xFFFFu ? 0u : (br << shift) + split;
      lut[(size_t)j * nb + b] = (e & 0xFFFFu) | (cum1 << 16);
    }
  }
  const size_t row_bytes = rows.size() * sizeof(u32), lut_bytes = lut.size() * sizeof(u32);
  rc_model* mm = nullptr;
  char* d = nullptr;
  const rc_status up = model_upload(
      ctx, kind, total_freq,
      {{rows.data(), row_bytes}, {lut.data(), lut_bytes}, {maps, maps ? period * 256u : 0u}}, &mm,
      &d);
  if (up != RC_OK) return up;
  mm->plan = plan;
  SetArgs& a = kind != RC_KIND_ORDER1 ? mm->set : mm->o1.s;
  small_model_args(a.m, n_symbols, total_freq, plan.dec_bits, plan.dec_shift);
  a.rows = (const u32*)d;
  a.lut = (const u32*)(d + row_bytes);
  a.k = n_models;
  a.tab_bytes = plan.enc_tab;
  if (kind == RC_KIND_ORDER1) {
    mm->o1.map = (const uint8_t*)(d + row_bytes + lut_bytes);
    mm->o1.first_row = first_row;
    mm->o1.period = period;
    mm->o1_lag = lag;
  }
  *out = mm;
  return RC_OK;
}

rc_status rc_model_create_static_set(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                     const uint32_t* c_freq, const uint32_t* cum_freq,
                                     uint32_t total_freq, rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !out) return RC_E_ARG;
  *out = nullptr;
  const rc_status ok = set_check(n_models, n_symbols, c_freq, cum_freq, total_freq);
  if (ok != RC_OK) return ok;
  SetPlan plan;
  rc_set_plan(n_models, total_freq, &plan);
  return set_build(ctx, RC_KIND_SET, n_models, n_symbols, c_freq, cum_freq, total_freq, plan,
                   nullptr, 0, 0, 0, out);
}

rc_status rc_encode_batch_indexed(rc_ctx* ctx, const rc_model* set, const uint8_t* syms,
                                  const uint8_t* idx, const uint64_t* sym_off,
                                  uint32_t n_chunks, uint8_t* out, const uint64_t* out_off,
                                  uint64_t* out_len, uint32_t* flags) {
  return batch_call(ctx, set, 1u << RC_KIND_SET, true, n_chunks,
                    syms && idx && sym_off && out && out_off && out_len && flags,
                    "indexed encode launch", [&] {
                      return rc_set_encode_launch(ctx->cur, ctx->knobs, set->set, set->div,
                                                  set->plan, syms, idx, sym_off, n_chunks, out,
                                                  out_off, out_len, flags);
                    });
}

rc_status rc_decode_batch_indexed(rc_ctx* ctx, const rc_model* set, const uint8_t* code,
                                  const uint64_t* code_off, const uint64_t* code_len,
                                  const uint8_t* idx, uint8_t* syms_out, const uint64_t* sym_off,
                                  uint32_t n_chunks, uint32_t* flags) {
  return batch_call(ctx, set, 1u << RC_KIND_SET, true, n_chunks,
                    code && code_off && code_len && idx && syms_out && sym_off && flags,
                    "indexed decode launch", [&] {
                      return rc_set_decode_launch(ctx->cur, ctx->knobs, set->set, set->div,
                                                  set->plan, code, code_off, code_len, idx,
                                                  syms_out, sym_off, n_chunks, flags);
                    });
}

// ---- static chunk sets (rc_chunk_set.h; kernels in rc_chunk_set.hip, rc_decode_grouped_*.hip) ----

// The rows of a checked chunk set as the static coders' tables: per row what static_tables builds
// for it, less what a chunk set does not carry (no row is flat and none has pair tables: DESIGN.md
// §9.20).  With one total the class, the constants and the table sizes are those of the total, so
// the rows' ModelArgs differ in the table pointers alone: *a is row 0's (pointers null), and the
// segments hold the rows back to back.
struct ChunkSetTables {
  ModelArgs a;
  ChunkSetArgs cs;
  std::vector<uint2> tab;
  std::vector<u32> lut;
  std::vector<uint8_t> symof;
};
static rc_status chunk_set_tables(u32 n_models, u32 n_symbols, const u32* c, const u32* cum,
                                  u32 total, ChunkSetTables* t) {
  bool complete = true;
  for (u32 j = 0; j < n_models; ++j) {
    StaticTables st;
    const rc_status built = static_tables(n_symbols, c + (size_t)j * n_symbols,
                                          cum + (size_t)j * n_symbols, total, &st);
    if (built != RC_OK) return built;
    if (j == 0) {
      t->a = st.a;
      t->a.flat = 0;
      t->cs.lut_stride = (u32)st.lut.size();
      t->cs.symof_stride = (u32)st.symof.size();
    }
    // (unreachable: the sizes follow from the total)
    if (st.tab.size() != 256 || st.lut.size() != t->cs.lut_stride ||
        st.symof.size() != t->cs.symof_stride || (st.lut.size() & 3) || (st.symof.size() & 15))
      return RC_E_BAD_MODEL;
    t->tab.insert(t->tab.end(), st.tab.begin(), st.tab.end());
    t->lut.insert(t->lut.end(), st.lut.begin(), st.lut.end());
    t->symof.insert(t->symof.end(), st.symof.begin(), st.symof.end());
    complete = complete && st.complete;
  }
  t->cs.k = n_models;
  t->cs.smv = complete ? 2u : 1u;
  return RC_OK;
}

// Internal test hooks (not in include/range_coder.h; host only, no device needed).
// rc_chunk_set_check_: rc_model_create_chunk_set's validation of its tables (the static set's).
rc_status rc_chunk_set_check_(uint32_t n_models, uint32_t n_symbols, const uint32_t* c_freq,
                              const uint32_t* cum_freq, uint32_t total_freq) {
  return set_check(n_models, n_symbols, c_freq, cum_freq, total_freq);
}
// rc_chunk_set_plan_: what the launchers use for the set, out[10] = {the encoder variant (2: every
// row complete, else 1), the decoder's LUT when the direct q-to-symbol table is not taken (2, 1
// or 4), its lanes per workgroup, has_symof (LUT 6 can be taken), div (0 DIV_POW2, 1 DIV_MAGIC),
// tab stride (bytes between two rows), lut stride (bytes), symof stride (bytes), has_pair (0),
// flat (0)}.
rc_status rc_chunk_set_plan_(uint32_t n_models, uint32_t n_symbols, const uint32_t* c_freq,
                             const uint32_t* cum_freq, uint32_t total_freq, uint32_t* out) {
  if (!out) return RC_E_ARG;
  const rc_status ok = set_check(n_models, n_symbols, c_freq, cum_freq, total_freq);
  if (ok != RC_OK) return ok;
  ChunkSetTables t;
  const rc_status built = chunk_set_tables(n_models, n_symbols, c_freq, cum_freq, total_freq, &t);
  if (built != RC_OK) return built;
  int lut = 0;
  const u32 lanes = rc_chunk_decode_class(t.a, &lut);
  const u32 v[10] = {t.cs.smv, (u32)lut, lanes, (u32)(t.cs.symof_stride != 0),
                     (u32)div_of(total_freq), 256u * (u32)sizeof(uint2), 4u * t.cs.lut_stride,
                     t.cs.symof_stride, t.a.pair ? 1u : 0u, t.a.flat};
  memcpy(out, v, sizeof v);
  return RC_OK;
}

rc_status rc_model_create_chunk_set(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                    const uint32_t* c_freq, const uint32_t* cum_freq,
                                    uint32_t total_freq, rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !out) return RC_E_ARG;
  *out = nullptr;
  const rc_status ok = set_check(n_models, n_symbols, c_freq, cum_freq, total_freq);
  if (ok != RC_OK) return ok;
  ChunkSetTables t;
  const rc_status built = chunk_set_tables(n_models, n_symbols, c_freq, cum_freq, total_freq, &t);
  if (built != RC_OK) return built;
  const size_t tab_bytes = t.tab.size() * sizeof(uint2), lut_bytes = t.lut.size() * sizeof(u32);
  rc_model* mm = nullptr;
  char* d = nullptr;
  const rc_status up = model_upload(
      ctx, RC_KIND_CHUNK_SET, total_freq,
      {{t.tab.data(), tab_bytes}, {t.lut.data(), lut_bytes}, {t.symof.data(), t.symof.size()}},
      &mm, &d);
  if (up != RC_OK) return up;
  t.a.tab = (const uint2*)d;
  t.a.lut = (const u32*)(d + tab_bytes);
  t.a.pair = nullptr;
  t.a.symof = t.symof.empty() ? nullptr : (const uint8_t*)(d + tab_bytes + lut_bytes);
  mm->args = t.a;
  mm->cset = t.cs;
  *out = mm;
  return RC_OK;
}

rc_status rc_encode_batch_chunk_set(rc_ctx* ctx, const rc_model* set, const uint8_t* class_of,
                                    const uint8_t* syms, const uint64_t* sym_off,
                                    uint32_t n_chunks, uint8_t* out, const uint64_t* out_off,
                                    uint64_t* out_len, uint32_t* flags) {
  return batch_call(ctx, set, 1u << RC_KIND_CHUNK_SET, true, n_chunks,
                    class_of && syms && sym_off && out && out_off && out_len && flags,
                    "chunk-set encode launch", [&] {
                      return rc_chunk_encode_launch(ctx->cur, ctx->knobs, set->args, set->div,
                                                    set->cset, ctx->group, class_of, syms, sym_off,
                                                    n_chunks, out, out_off, out_len, flags);
                    });
}

rc_status rc_decode_batch_chunk_set(rc_ctx* ctx, const rc_model* set, const uint8_t* class_of,
                                    const uint8_t* code, const uint64_t* code_off,
                                    const uint64_t* code_len, uint8_t* syms_out,
                                    const uint64_t* sym_off, uint32_t n_chunks, uint32_t* flags) {
  return batch_call(
      ctx, set, 1u << RC_KIND_CHUNK_SET, true, n_chunks,
      class_of && code && code_off && code_len && syms_out && sym_off && flags,
      "chunk-set decode launch", [&] {
        return set->div == DIV_POW2
                   ? rc_chunk_decode_launch_pow2(ctx->cur, ctx->knobs, set->args, set->cset,
                                                 ctx->group, class_of, code, code_off, code_len,
                                                 syms_out, sym_off, n_chunks, flags)
                   : rc_chunk_decode_launch_magic(ctx->cur, ctx->knobs, set->args, set->cset,
                                                  ctx->group, class_of, code, code_off, code_len,
                                                  syms_out, sym_off, n_chunks, flags);
      });
}

// ---- order-1 sets (rc_order1.h; kernels in rc_order1.hip) ----

// One description of an order-1 set for the plain, periodic and lagged calls: (period, lag) is
// (1, 1), (period, 1) or (period, lag).

// What the constructors accept: a period and a lag of 1, 2, 4 or 8 (RC_E_ARG, before any table is
// looked at), the set's rules, then a first_row and `period` map slices that name rows of the set
// (the map's rules do not depend on the lag)
static rc_status order1_check(u32 n_models, u32 n_symbols, const u32* c, const u32* cum,
                              u32 total, u32 period, u32 lag, const uint8_t* ctx_map,
                              u32 first_row) {
  if (!ctx_map || !o1_period_ok(period) || !o1_lag_ok(lag)) return RC_E_ARG;
  const rc_status ok = set_check(n_models, n_symbols, c, cum, total);
  if (ok != RC_OK) return ok;
  if (first_row >= n_models) return RC_E_BAD_MODEL;
  for (u32 i = 0; i < period * n_symbols; ++i)
    if (ctx_map[i] >= n_models) return RC_E_BAD_MODEL;
  return RC_OK;
}

// rc_model_set_plan_ for an order-1 set of `period` maps (the decoder's LDS includes them; at
// period 1 the encoder's numbers are the set's).  The plan does not depend on the lag: a lagged
// set stages what the periodic set of its (K, total, P) stages and keeps its contexts in registers.
static rc_status order1_plan_hook(u32 n_models, u32 total, u32 period, u32 lag, uint32_t* out) {
  if (!o1_period_ok(period) || !o1_lag_ok(lag)) return RC_E_ARG;
  return plan_hook<SetPlan>(n_models >= 1 && n_models <= RC_MAX_SET_MODELS, total, out,
                            [&](SetPlan* p) { rc_order1_plan(n_models, total, period, p); });
}

static rc_status order1_create(rc_ctx* ctx, u32 n_models, u32 n_symbols, const u32* c_freq,
                               const u32* cum_freq, u32 total_freq, u32 period, u32 lag,
                               const uint8_t* ctx_map, u32 first_row, rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !ctx_map || !out) return RC_E_ARG;
  *out = nullptr;
  // (a bad period or lag is the check's first refusal)
  const rc_status ok = order1_check(n_models, n_symbols, c_freq, cum_freq, total_freq, period, lag,
                                    ctx_map, first_row);
  if (ok != RC_OK) return ok;
  SetPlan plan;
  rc_order1_plan(n_models, total_freq, period, &plan);
  // the kernels stage 256 entries per slice: a symbol past the alphabet (a flagged chunk) maps to
  // row 0
  uint8_t maps[O1_MAX_PERIOD * 256] = {0};
  for (u32 ph = 0; ph < period; ++ph)
    memcpy(maps + 256 * ph, ctx_map + (size_t)ph * n_symbols, n_symbols);
  return set_build(ctx, RC_KIND_ORDER1, n_models, n_symbols, c_freq, cum_freq, total_freq, plan,
                   maps, period, lag, first_row, out);
}

// Internal test hooks (not in include/range_coder.h; host only, no device needed): the
// constructors' validation and their plan, for rc_model_create_order1_set
// (tests/test_order1_model.py), _periodic (tests/test_periodic_model.py) and _lagged
// (tests/test_lag_model.py).
rc_status rc_model_order1_check_(uint32_t n_models, uint32_t n_symbols, const uint32_t* c_freq,
                                 const uint32_t* cum_freq, uint32_t total_freq,
                                 const uint8_t* ctx_map, uint32_t first_row) {
  return order1_check(n_models, n_symbols, c_freq, cum_freq, total_freq, 1, 1, ctx_map, first_row);
}
rc_status rc_model_order1_check_periodic_(uint32_t n_models, uint32_t n_symbols,
                                          const uint32_t* c_freq, const uint32_t* cum_freq,
                                          uint32_t total_freq, uint32_t period,
                                          const uint8_t* ctx_map, uint32_t first_row) {
  return order1_check(n_models, n_symbols, c_freq, cum_freq, total_freq, period, 1, ctx_map,
                      first_row);
}
rc_status rc_model_order1_check_lagged_(uint32_t n_models, uint32_t n_symbols,
                                        const uint32_t* c_freq, const uint32_t* cum_freq,
                                        uint32_t total_freq, uint32_t period, uint32_t lag,
                                        const uint8_t* ctx_map, uint32_t first_row) {
  return order1_check(n_models, n_symbols, c_freq, cum_freq, total_freq, period, lag, ctx_map,
                      first_row);
}
rc_status rc_model_order1_plan_(uint32_t n_models, uint32_t total_freq, uint32_t* out) {
  return order1_plan_hook(n_models, total_freq, 1, 1, out);
}
rc_status rc_model_order1_plan_periodic_(uint32_t n_models, uint32_t total_freq, uint32_t period,
                                         uint32_t* out) {
  return order1_plan_hook(n_models, total_freq, period, 1, out);
}
rc_status rc_model_order1_plan_lagged_(uint32_t n_models, uint32_t total_freq, uint32_t period,
                                       uint32_t lag, uint32_t* out) {
  return order1_plan_hook(n_models, total_freq, period, lag, out);
}

rc_status rc_model_create_order1_set(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                     const uint32_t* c_freq, const uint32_t* cum_freq,
                                     uint32_t total_freq, const uint8_t* ctx_map,
                                     uint32_t first_row, rc_model** out) {
  return order1_create(ctx, n_models, n_symbols, c_freq, cum_freq, total_freq, 1, 1, ctx_map,
                       first_row, out);
}
rc_status rc_model_create_order1_set_periodic(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                              const uint32_t* c_freq, const uint32_t* cum_freq,
                                              uint32_t total_freq, uint32_t period,
                                              const uint8_t* ctx_map, uint32_t first_row,
                                              rc_model** out) {
  return order1_create(ctx, n_models, n_symbols, c_freq, cum_freq, total_freq, period, 1, ctx_map,
                       first_row, out);
}
rc_status rc_model_create_order1_set_lagged(rc_ctx* ctx, uint32_t n_models, uint32_t n_symbols,
                                            const uint32_t* c_freq, const uint32_t* cum_freq,
                                            uint32_t total_freq, uint32_t period, uint32_t lag,
                                            const uint8_t* ctx_map, uint32_t first_row,
                                            rc_model** out) {
  return order1_create(ctx, n_models, n_symbols, c_freq, cum_freq, total_freq, period, lag,
                       ctx_map, first_row, out);
}

rc_status rc_encode_batch_order1(rc_ctx* ctx, const rc_model* o1, const uint8_t* syms,
                                 const uint64_t* sym_off, uint32_t n_chunks, uint8_t* out,
                                 const uint64_t* out_off, uint64_t* out_len, uint32_t* flags) {
  return batch_call(ctx, o1, 1u << RC_KIND_ORDER1, true, n_chunks,
                    syms && sym_off && out && out_off && out_len && flags,
                    "order-1 encode launch", [&] {
                      return rc_order1_encode_launch(ctx->cur, ctx->knobs, o1->o1, o1->o1_lag,
                                                     o1->div, o1->plan, syms, sym_off, n_chunks,
                                                     out, out_off, out_len, flags);
                    });
}

rc_status rc_decode_batch_order1(rc_ctx* ctx, const rc_model* o1, const uint8_t* code,
                                 const uint64_t* code_off, const uint64_t* code_len,
                                 uint8_t* syms_out, const uint64_t* sym_off, uint32_t n_chunks,
                                 uint32_t* flags) {
  return batch_call(ctx, o1, 1u << RC_KIND_ORDER1, true, n_chunks,
                    code && code_off && code_len && syms_out && sym_off && flags,
                    "order-1 decode launch", [&] {
                      return rc_order1_decode_launch(ctx->cur, ctx->knobs, o1->o1, o1->o1_lag,
                                                     o1->div, o1->plan, code, code_off, code_len,
                                                     syms_out, sym_off, n_chunks, flags);
                    });
}

// rc_encode_host / rc_decode_host: the pipelined host path lives in rc_stream.hip

rc_status rc_synth_fill(rc_ctx* ctx, uint64_t seed, const uint8_t* inv_cdf_host,
                        uint8_t* syms_dev, uint64_t chunk_len, uint32_t n_chunks) {
  if (!ctx || !inv_cdf_host || !syms_dev) return RC_E_ARG;
  if (n_chunks == 0 || chunk_len == 0) return RC_OK;
  DeviceGuard g(ctx->device);
  if (!g.ok) return RC_E_DEVICE;
  const uint8_t* dinv = ctx->inv;
  void* pin = rc_pinned_scratch_(65536);
  if (!pin) return RC_E_DEVICE;
  memcpy(pin, inv_cdf_host, 65536);
  hipError_t e = hipMemcpyAsync(ctx->inv, pin, 65536, hipMemcpyHostToDevice, ctx->cur);
  if (e != hipSuccess) return device_error(e, "rc_synth_fill copy");
  if ((chunk_len & 15) == 0 && ((uintptr_t)syms_dev & 15) == 0) {
    const u64 words = (chunk_len >> 4) * (u64)n_chunks;
    const u64 blocks = std::min<u64>((words + WG - 1) / WG, 1u << 16);
    hipLaunchKernelGGL(k_synth, dim3((u32)blocks), dim3(WG), 0, ctx->cur, seed,
                       dinv, syms_dev, chunk_len, words);
  } else {
    hipLaunchKernelGGL(k_synth_generic, dim3((n_chunks + WG - 1) / WG), dim3(WG), 0, ctx->cur,
                       seed, dinv, syms_dev, chunk_len, n_chunks);
  }
  rc_status st = launch_status();
  // the pinned staging is reused by this thread's next call: wait for the copy
  if (st == RC_OK && (e = hipStreamSynchronize(ctx->cur)) != hipSuccess)
    return device_error(e, "rc_synth_fill sync");
  return st;
}

// Internal test hook (not in include/range_coder.h): range / total for n (range, total) pairs
// through k_test_range_par_total; out: 3 n results (host memory).  Synchronous.
rc_status rc_test_range_par_total_(rc_ctx* ctx, const uint64_t* ranges, const uint32_t* totals,
                                   uint32_t n, uint64_t* out) {
  if (!ctx || !ranges || !totals || !out || n == 0 || n > (1u << 20)) return RC_E_ARG;
  std::vector<ModelArgs> ms(n);
  for (u32 i = 0; i < n; ++i) {
    if (totals[i] == 0) return RC_E_BAD_MODEL;
    memset(&ms[i], 0, sizeof(ModelArgs));
    div_constants(ms[i], totals[i]);
  }
  DeviceGuard g(ctx->device);
  char* d = nullptr;
  const size_t b_r = 8ull * n, b_m = sizeof(ModelArgs) * n, b_o = 24ull * n;
  if (hipMalloc((void**)&d, b_r + b_m + b_o) != hipSuccess) return RC_E_DEVICE;
  rc_status st = RC_OK;
  if (hipMemcpy(d, ranges, b_r, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + b_r, ms.data(), b_m, hipMemcpyHostToDevice) != hipSuccess) {
    st = RC_E_DEVICE;
  } else {
    hipLaunchKernelGGL(k_test_range_par_total, dim3((n + 63) / 64), dim3(64), 0, ctx->cur,
                       (const u64*)d, (const ModelArgs*)(d + b_r), n, (u64*)(d + b_r + b_m));
    st = launch_status();
    if (st == RC_OK && (hipStreamSynchronize(ctx->cur) != hipSuccess ||
                        hipMemcpy(out, d + b_r + b_m, b_o, hipMemcpyDeviceToHost) != hipSuccess))
      st = RC_E_DEVICE;
  }
  (void)hipFree(d);
  return st;
}

}  // extern "C"

// ---- wide static models (rc_wide.h; kernels in rc_wide.hip) ----

// what rc_model_create_static_wide accepts (include/range_coder.h)
static rc_status wide_check(u32 n_symbols, const u32* c, const u32* cum, u32 total) {
  if (!c || !cum) return RC_E_ARG;
  if (n_symbols < 1 || n_symbols > RC_MAX_WIDE_SYMBOLS || total < 256 || total > 65536)
    return RC_E_BAD_MODEL;
  return table_ok(n_symbols, c, cum, total) ? RC_OK : RC_E_BAD_MODEL;
}

// The wide decoder's buckets, 2^bits of them: per bucket s_lo | s_hi << 16, FreqTable::find_index
// of the bucket's first and of its last frequency (the last s with cum[s] <= f; both have c > 0),
// padded with the last real bucket (the kernel masks the bucket index).  *stride_out: the first
// stride of the kernel's search, the largest power of two below the widest bucket's symbol count
// s_hi - s_lo + 1 (0 when every bucket names one symbol).
static std::vector<u32> wide_buckets(u32 n, const u32* cum, u32 total, u32 bits, u32 shift,
                                     u32* stride_out) {
  const u32 nb = 1u << bits, last = (total - 1) >> shift;
  std::vector<u32> lt(nb);
  u32 s = 0, widest = 1;
  auto advance = [&](u32 f) {  // the last s with cum[s] <= f (f rises from call to call)
    while (s + 1 < n && cum[s + 1] <= f) ++s;
    return s;
  };
  for (u32 b = 0; b <= last && b < nb; ++b) {
    const u32 f0 = b << shift;
    const u32 f1 = std::min<u64>((u64)(b + 1) << shift, total);
    const u32 lo = advance(f0), hi = advance(f1 - 1);
    lt[b] = lo | (hi << 16);
    widest = std::max(widest, hi - lo + 1);
  }
  for (u32 b = last + 1; b < nb; ++b) lt[b] = lt[last];
  *stride_out = widest > 1 ? 1u << (bitlen(widest - 1) - 1) : 0u;
  return lt;
}

extern "C" {

// Internal test hooks (not in include/range_coder.h; host only, no device needed).
// rc_model_wide_check_: rc_model_create_static_wide's validation of its table.
rc_status rc_model_wide_check_(uint32_t n_symbols, const uint32_t* c_freq,
                               const uint32_t* cum_freq, uint32_t total_freq) {
  return wide_check(n_symbols, c_freq, cum_freq, total_freq);
}
// rc_model_wide_plan_: what the launchers use for a table of n_symbols symbols and total
// total_freq (a launch too small to reach every CU with such workgroups runs fewer lanes),
// out[8] = encoder {lanes per workgroup, dynamic LDS bytes, table layout (0: 8-B (cum, c)
// entries, 1: cum-only row), table bytes}, decoder {lanes, LDS bytes, log2 buckets, bucket shift}.
rc_status rc_model_wide_plan_(uint32_t n_symbols, uint32_t total_freq, uint32_t* out) {
  return plan_hook<WidePlan>(n_symbols >= 1 && n_symbols <= RC_MAX_WIDE_SYMBOLS, total_freq, out,
                             [&](WidePlan* p) { rc_wide_plan(n_symbols, total_freq, p); });
}

rc_status rc_model_create_static_wide(rc_ctx* ctx, uint32_t n_symbols, const uint32_t* c_freq,
                                      const uint32_t* cum_freq, uint32_t total_freq,
                                      rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !out) return RC_E_ARG;
  *out = nullptr;
  const rc_status ok = wide_check(n_symbols, c_freq, cum_freq, total_freq);
  if (ok != RC_OK) return ok;
  WidePlan plan;
  rc_wide_plan(n_symbols, total_freq, &plan);
  if (!plan.enc_lanes || !plan.dec_lanes) return RC_E_BAD_MODEL;  // unreachable
  // the cum row cum[0 .. n + 1] with cum[n] = cum[n + 1] = total (so c = cum[s + 1] - cum[s] for
  // every symbol, and 0 for the entry a symbol past the alphabet is clamped to), and the buckets
  std::vector<u32> row(n_symbols + 2);
  for (u32 s = 0; s < n_symbols + 2; ++s) row[s] = s < n_symbols ? cum_freq[s] : total_freq;
  u32 top_stride = 0;
  const std::vector<u32> lut =
      wide_buckets(n_symbols, cum_freq, total_freq, plan.dec_bits, plan.dec_shift,
                   &top_stride);
  const size_t row_bytes = row.size() * sizeof(u32), lut_bytes = lut.size() * sizeof(u32);
  rc_model* mm = nullptr;
  char* d = nullptr;
  const rc_status up = model_upload(ctx, RC_KIND_WIDE, total_freq,
                                    {{row.data(), row_bytes}, {lut.data(), lut_bytes}}, &mm, &d);
  if (up != RC_OK) return up;
  mm->wplan = plan;
  WideArgs& a = mm->wide;
  small_model_args(a.m, n_symbols, total_freq, plan.dec_bits, plan.dec_shift);
  a.row = (const u32*)d;
  a.lut = (const u32*)(d + row_bytes);
  a.top_stride = top_stride;
  a.tab_bytes = plan.enc_tab;
  *out = mm;
  return RC_OK;
}

rc_status rc_encode_batch_wide(rc_ctx* ctx, const rc_model* wide, const void* syms,
                               const uint64_t* sym_off, uint32_t n_chunks, uint8_t* out,
                               const uint64_t* out_off, uint64_t* out_len, uint32_t* flags) {
  return batch_call(ctx, wide, 1u << RC_KIND_WIDE, ((uintptr_t)syms & 1u) == 0, n_chunks,
                    syms && sym_off && out && out_off && out_len && flags, "wide encode launch",
                    [&] {
                      return rc_wide_encode_launch(ctx->cur, ctx->knobs, wide->wide, wide->div,
                                                   wide->wplan, (const uint16_t*)syms, sym_off,
                                                   n_chunks, out, out_off, out_len, flags);
                    });
}

rc_status rc_decode_batch_wide(rc_ctx* ctx, const rc_model* wide, const uint8_t* code,
                               const uint64_t* code_off, const uint64_t* code_len,
                               void* syms_out, const uint64_t* sym_off, uint32_t n_chunks,
                               uint32_t* flags) {
  return batch_call(ctx, wide, 1u << RC_KIND_WIDE, ((uintptr_t)syms_out & 1u) == 0, n_chunks,
                    code && code_off && code_len && syms_out && sym_off && flags,
                    "wide decode launch", [&] {
                      return rc_wide_decode_launch(ctx->cur, ctx->knobs, wide->wide, wide->div,
                                                   wide->wplan, code, code_off, code_len,
                                                   (uint16_t*)syms_out, sym_off, n_chunks, flags);
                    });
}

}  // extern "C"

// ---- wide16 static models (rc_wide16.h; kernels in rc_wide16.hip) ----

// what rc_model_create_static_wide16 accepts (include/range_coder.h)
static rc_status wide16_check(u32 n_symbols, const u32* c, const u32* cum, u32 total) {
  if (!c || !cum) return RC_E_ARG;
  if (n_symbols < 1 || n_symbols > RC_MAX_WIDE16_SYMBOLS || total < 256 || total > 65536)
    return RC_E_BAD_MODEL;
  return table_ok(n_symbols, c, cum, total) ? RC_OK : RC_E_BAD_MODEL;
}

extern "C" {

// Internal test hooks (not in include/range_coder.h; host only, no device needed).
// rc_model_wide16_check_: rc_model_create_static_wide16's validation of its table.
rc_status rc_model_wide16_check_(uint32_t n_symbols, const uint32_t* c_freq,
                                 const uint32_t* cum_freq, uint32_t total_freq) {
  return wide16_check(n_symbols, c_freq, cum_freq, total_freq);
}
// rc_model_wide16_plan_: what the launchers use for a table of n_symbols symbols and total
// total_freq, out[8] = encoder {lanes per workgroup, dynamic LDS bytes (rings only), 0, bytes of
// the entries in device memory}, decoder {lanes, LDS bytes, log2 of the q-to-symbol table's
// entries, 0}.
rc_status rc_model_wide16_plan_(uint32_t n_symbols, uint32_t total_freq, uint32_t* out) {
  return plan_hook<Wide16Plan>(n_symbols >= 1 && n_symbols <= RC_MAX_WIDE16_SYMBOLS, total_freq,
                               out,
                               [&](Wide16Plan* p) { rc_wide16_plan(n_symbols, total_freq, p); });
}

rc_status rc_model_create_static_wide16(rc_ctx* ctx, uint32_t n_symbols, const uint32_t* c_freq,
                                        const uint32_t* cum_freq, uint32_t total_freq,
                                        rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !out) return RC_E_ARG;
  *out = nullptr;
  const rc_status ok = wide16_check(n_symbols, c_freq, cum_freq, total_freq);
  if (ok != RC_OK) return ok;
  Wide16Plan plan;
  rc_wide16_plan(n_symbols, total_freq, &plan);
  const Wide16Tables t = wide16_build_tables(n_symbols, c_freq, cum_freq, total_freq);
  // (the 8-B entries first: the allocation's alignment is theirs; then the row, then the halfwords)
  const size_t enc_bytes = t.enc.size() * sizeof(u32), row_bytes = t.row.size() * sizeof(u32),
               symof_bytes = t.symof.size() * sizeof(uint16_t);
  rc_model* mm = nullptr;
  char* d = nullptr;
  const rc_status up = model_upload(
      ctx, RC_KIND_WIDE16, total_freq,
      {{t.enc.data(), enc_bytes}, {t.row.data(), row_bytes}, {t.symof.data(), symof_bytes}}, &mm,
      &d);
  if (up != RC_OK) return up;
  mm->w16plan = plan;
  Wide16Args& a = mm->w16;
  small_model_args(a.m, n_symbols, total_freq, plan.dec_bits, plan.dec_shift);
  a.enc = (const uint2*)d;
  a.row = (const u32*)(d + enc_bytes);
  a.symof = (const uint16_t*)(d + enc_bytes + row_bytes);
  a.enc_clamp = t.enc_clamp;
  a.qmask = (u32)t.symof.size() - 1u;
  *out = mm;
  return RC_OK;
}

rc_status rc_encode_batch_wide16(rc_ctx* ctx, const rc_model* wide16, const void* syms,
                                 const uint64_t* sym_off, uint32_t n_chunks, uint8_t* out,
                                 const uint64_t* out_off, uint64_t* out_len, uint32_t* flags) {
  return batch_call(ctx, wide16, 1u << RC_KIND_WIDE16, ((uintptr_t)syms & 1u) == 0, n_chunks,
                    syms && sym_off && out && out_off && out_len && flags,
                    "wide16 encode launch", [&] {
                      if (wide16->w16_fine)
                        return rc_wide16_fine_encode_launch(ctx->cur, ctx->knobs, wide16->w16f,
                                                            wide16->div, wide16->w16plan,
                                                            (const uint16_t*)syms, sym_off,
                                                            n_chunks, out, out_off, out_len,
                                                            flags);
                      return rc_wide16_encode_launch(ctx->cur, ctx->knobs, wide16->w16,
                                                     wide16->div, wide16->w16plan,
                                                     (const uint16_t*)syms, sym_off, n_chunks,
                                                     out, out_off, out_len, flags);
                    });
}

rc_status rc_decode_batch_wide16(rc_ctx* ctx, const rc_model* wide16, const uint8_t* code,
                                 const uint64_t* code_off, const uint64_t* code_len,
                                 void* syms_out, const uint64_t* sym_off, uint32_t n_chunks,
                                 uint32_t* flags) {
  return batch_call(ctx, wide16, 1u << RC_KIND_WIDE16, ((uintptr_t)syms_out & 1u) == 0,
                    n_chunks, code && code_off && code_len && syms_out && sym_off && flags,
                    "wide16 decode launch", [&] {
                      if (wide16->w16_fine)
                        return rc_wide16_fine_decode_launch(ctx->cur, ctx->knobs, wide16->w16f,
                                                            wide16->div, wide16->w16plan, code,
                                                            code_off, code_len,
                                                            (uint16_t*)syms_out, sym_off,
                                                            n_chunks, flags);
                      return rc_wide16_decode_launch(ctx->cur, ctx->knobs, wide16->w16,
                                                     wide16->div, wide16->w16plan, code, code_off,
                                                     code_len, (uint16_t*)syms_out, sym_off,
                                                     n_chunks, flags);
                    });
}

}  // extern "C"

// ---- wide16 fine models (rc_wide16_fine.h; kernels in rc_wide16_fine.hip) ----

// what rc_model_create_static_wide16_fine accepts (include/range_coder.h)
static rc_status wide16_fine_check(u32 n_symbols, const u32* c, const u32* cum, u32 total) {
  if (!c || !cum) return RC_E_ARG;
  if (n_symbols < 1 || n_symbols > RC_MAX_WIDE16_SYMBOLS || total <= 65536u ||
      total > RC_MAX_WIDE16_FINE_TOTAL)
    return RC_E_BAD_MODEL;
  return table_ok(n_symbols, c, cum, total) ? RC_OK : RC_E_BAD_MODEL;
}

extern "C" {

// Internal test hooks (not in include/range_coder.h; host only, no device needed).
// rc_model_wide16_fine_check_: rc_model_create_static_wide16_fine's validation of its table.
rc_status rc_model_wide16_fine_check_(uint32_t n_symbols, const uint32_t* c_freq,
                                      const uint32_t* cum_freq, uint32_t total_freq) {
  return wide16_fine_check(n_symbols, c_freq, cum_freq, total_freq);
}
// rc_model_wide16_fine_plan_: what the launchers use for a table of n_symbols symbols and total
// total_freq, out[8] = encoder {lanes per workgroup, dynamic LDS bytes (rings only), 0, bytes of
// the entries in device memory}, decoder {lanes, LDS bytes, log2 of the bucket count, the bucket
// shift}.
rc_status rc_model_wide16_fine_plan_(uint32_t n_symbols, uint32_t total_freq, uint32_t* out) {
  if (!out) return RC_E_ARG;
  Wide16Plan p;
  rc_wide16_fine_plan(n_symbols, total_freq, &p);
  if (!p.enc_lanes) return RC_E_BAD_MODEL;
  const u32 v[8] = {p.enc_lanes, p.enc_lds, p.enc_layout, p.enc_tab,
                    p.dec_lanes, p.dec_lds, p.dec_bits,   p.dec_shift};
  memcpy(out, v, sizeof v);
  return RC_OK;
}

rc_status rc_model_create_static_wide16_fine(rc_ctx* ctx, uint32_t n_symbols,
                                             const uint32_t* c_freq, const uint32_t* cum_freq,
                                             uint32_t total_freq, rc_model** out) {
  if (!ctx || !c_freq || !cum_freq || !out) return RC_E_ARG;
  *out = nullptr;
  const rc_status ok = wide16_fine_check(n_symbols, c_freq, cum_freq, total_freq);
  if (ok != RC_OK) return ok;
  Wide16Plan plan;
  rc_wide16_fine_plan(n_symbols, total_freq, &plan);
  const Wide16FineTables t =
      wide16_fine_build_tables(n_symbols, c_freq, cum_freq, total_freq, plan.dec_bits);
  // (the 8-B entries first: the allocation's alignment is theirs; then the 4-B cum row, then the
  // halfwords, the occupied symbols an even count so that the buckets stay 4-B aligned)
  const size_t enc_bytes = t.enc.size() * sizeof(u32), rcum_bytes = t.rcum.size() * sizeof(u32),
               occ_bytes = t.occ.size() * sizeof(uint16_t),
               bucket_bytes = t.bucket.size() * sizeof(uint16_t);
  rc_model* mm = nullptr;
  char* d = nullptr;
  const rc_status up = model_upload(ctx, RC_KIND_WIDE16, total_freq,
                                    {{t.enc.data(), enc_bytes},
                                     {t.rcum.data(), rcum_bytes},
                                     {t.occ.data(), occ_bytes},
                                     {t.bucket.data(), bucket_bytes}},
                                    &mm, &d);
  if (up != RC_OK) return up;
  mm->w16plan = plan;
  mm->w16_fine = true;
  Wide16FineArgs& a = mm->w16f;
  small_model_args(a.m, n_symbols, total_freq, plan.dec_bits, plan.dec_shift);
  a.enc = (const uint2*)d;
  a.rcum = (const u32*)(d + enc_bytes);
  a.occ = (const uint16_t*)(d + enc_bytes + rcum_bytes);
  a.bucket = (const uint16_t*)(d + enc_bytes + rcum_bytes + occ_bytes);
  a.enc_clamp = t.enc_clamp;
  a.shift = t.shift;
  a.qmax = total_freq - 1u;
  *out = mm;
  return RC_OK;
}

}  // extern "C"
