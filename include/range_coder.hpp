// range_coder.hpp — C++ host API over the C ABI (include/range_coder.h), mirroring the public
// surface of diegodox/range_coder_rust (src/lib.rs:1-13) for host programs.
//
//   trait PModel            (src/pmodel.rs:4-41)         -> rc::PModel (abstract class)
//   FreqTable example model (examples/sample_impl.rs)    -> rc::FreqTable
//   RangeCoder accessors      (src/range_coder.rs:26-146) -> rc::RangeCoder (a state snapshot)
//   Encoder::new/encode/peek_code/finish, pub range_coder
//                             (src/encoder.rs:7-55)       -> rc::Encoder (model read per call;
//                                                           encode() returns a ByteCount)
//   Decoder::new/decode/range_coder/data
//                             (src/decoder.rs:6-55)       -> rc::Decoder (model read per call)
//   error::RangeCoderError     (src/error.rs:3-13)       -> rc::RangeCoderError (exception)
//   (new) batch API                                      -> rc::encode_chunks / decode_chunks
//   (new) batch API, a model per symbol                  -> rc::ModelSet::encode_chunks /
//                                                           decode_chunks
//
// rc::ModelSet is declared only where <hip/hip_runtime_api.h> can be included: the indexed entry
// points take device memory alone, so its chunk helpers allocate and copy with the HIP runtime
// themselves.  Everything else in this header needs the C ABI only and is there either way.
//
// Header-only; link with librc_amd.so.  Everything runs on the GPU through the C ABI: there is
// no CPU implementation of the coder in the product.
#ifndef RANGE_CODER_AMD_HPP
#define RANGE_CODER_AMD_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "range_coder.h"

namespace rc {

class RangeCoderError : public std::runtime_error {
 public:
  // error.rs:3-13: which reference error a BAD_MODEL flag stands for, with its payload
  enum Kind { OTHER = 0, LOWER_BOUND_OVERFLOW, UPPER_BOUND_OVERFLOW, DIVIDE_BY_ZERO };
  RangeCoderError(const std::string& what, int status = 0, uint32_t flags = 0)
      : std::runtime_error(what), status(status), flags(flags) {}
  int status;      // rc_status of the failing call
  uint32_t flags;  // RC_F_* of the failing chunk (0 if not chunk-specific)
  Kind kind = OTHER;
  // LowerBoundOverflow {lower_bound, add_val, range} / UpperBoundOverflow {lower_bound, range}
  uint64_t lower_bound = 0, add_val = 0, range = 0;
};

inline void check(rc_status s, const char* what) {
  if (s != RC_OK) {
    std::string msg = std::string(what) + ": " + rc_status_string(s);
    if (s == RC_E_DEVICE) msg += std::string(" (") + rc_last_error() + ")";
    throw RangeCoderError(msg, s);
  }
}

inline std::string flag_string(uint32_t f) {
  std::string s;
  if (f & RC_F_ZERO_FREQ) s += "ZERO_FREQ|";
  if (f & RC_F_BAD_SYMBOL) s += "BAD_SYMBOL|";
  if (f & RC_F_CAPACITY) s += "CAPACITY|";
  if (f & RC_F_TRUNCATED) s += "TRUNCATED|";
  if (f & RC_F_CORRUPT) s += "CORRUPT|";
  if (f & RC_F_TOO_LONG) s += "TOO_LONG|";
  if (f & RC_F_BAD_MODEL) s += "BAD_MODEL|";
  if (f & RC_F_FINISHED) s += "FINISHED|";
  if (!s.empty()) s.pop_back();
  return s;
}

class Decoder;

// trait PModel (src/pmodel.rs:4-41)
class PModel {
 public:
  static constexpr size_t kCanonical = ~(size_t)0;
  virtual ~PModel() = default;
  virtual uint32_t c_freq(size_t index) const = 0;    // pmodel.rs:6
  virtual uint32_t cum_freq(size_t index) const = 0;  // pmodel.rs:8
  virtual uint32_t total_freq() const = 0;            // pmodel.rs:10
  // pmodel.rs:12.  Not overridden (returns kCanonical): the GPU decoder evaluates
  // FreqTable::find_index (sample_impl.rs:27-45) itself and decodes ahead.  Overridden:
  // Decoder::decode calls it at every symbol with the decoder (range_coder(), data() give the
  // exact state), as decoder.rs:40 does, and param_update uses the index it returns.
  virtual size_t find_index(const Decoder&) const { return kCanonical; }
  // An override that keeps FreqTable's binary-search semantics may return true here to keep
  // the decode-ahead path (its find_index is then not called).
  virtual bool canonical_find_index() const { return false; }
  // pmodel.rs:14-40
  virtual double ideal_code_length(size_t index) const {
    const double p = (double)c_freq(index);
    if (p == 0.0) throw RangeCoderError("code length is undefind when probability is zero");
    return (std::log((double)total_freq()) - std::log(p)) / std::log(2.0);
  }
  // Alphabet size: not a trait method in the reference (FreqTable::alphabet_count,
  // sample_impl.rs:55-57) but needed to snapshot the table for the GPU.
  virtual size_t alphabet_count() const = 0;
};

// examples/sample_impl.rs:4-70
class FreqTable : public PModel {
 public:
  explicit FreqTable(size_t alphabet_count) : c_(alphabet_count, 0), cum_(alphabet_count, 0) {}
  size_t alphabet_count() const override { return c_.size(); }
  void add_alphabet_freq(size_t index) { c_.at(index) += 1; }  // :58-60
  void calc_cum() {                                             // :61-69
    uint32_t t = 0;
    for (size_t i = 0; i < c_.size(); ++i) {
      cum_[i] = t;
      t += c_[i];
    }
    total_ = t;
  }
  uint32_t c_freq(size_t i) const override { return c_.at(i); }
  uint32_t cum_freq(size_t i) const override { return cum_.at(i); }
  uint32_t total_freq() const override { return total_; }

 private:
  std::vector<uint32_t> c_, cum_;
  uint32_t total_ = 0;
};

// One device (rc_ctx)
class Context {
 public:
  explicit Context(int device = 0) { check(rc_ctx_create(device, &ctx_), "rc_ctx_create"); }
  ~Context() {
    if (ctx_) rc_ctx_destroy(ctx_);
  }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  rc_ctx* get() const { return ctx_; }
  static Context& default_context() {
    static Context c(0);
    return c;
  }

 private:
  rc_ctx* ctx_ = nullptr;
};

namespace detail {
// a slot large enough for n symbols of a table (or tables) with counts c in nearly every case:
// the worst symbol's bits, 2 % and 64 bytes of slack, a multiple of 16
inline uint64_t slot_capacity(const std::vector<uint32_t>& c, uint32_t total, uint64_t n) {
  uint32_t cmin = 0xFFFFFFFFu;
  for (uint32_t x : c)
    if (x && x < cmin) cmin = x;
  const double bits = std::log2((double)total / (double)cmin);
  return ((uint64_t)std::ceil(n * bits / 8.0 * 1.02 + 64.0) + 15) & ~(uint64_t)15;
}
}  // namespace detail

// Device snapshot of a PModel's (c_freq, cum_freq, total_freq) table (rc_model)
class Model {
 public:
  Model(Context& ctx, const PModel& pm) : Model(ctx, snapshot_c(pm), snapshot_cum(pm), pm.total_freq()) {}
  Model(Context& ctx, const std::vector<uint32_t>& c, const std::vector<uint32_t>& cum,
        uint32_t total)
      : ctx_(&ctx), c_(c) {
    check(rc_model_create_static(ctx.get(), (uint32_t)c.size(), c.data(), cum.data(), total, &m_),
          "rc_model_create_static");
    total_ = total;
  }
  ~Model() {
    if (m_) rc_model_destroy(m_);
  }
  Model(const Model&) = delete;
  Model& operator=(const Model&) = delete;
  rc_model* get() const { return m_; }
  Context& ctx() const { return *ctx_; }
  // a slot large enough for n symbols in nearly every case (CAPACITY chunks are retried)
  uint64_t slot_capacity(uint64_t n) const { return detail::slot_capacity(c_, total_, n); }

 private:
  static std::vector<uint32_t> snapshot_c(const PModel& pm) {
    std::vector<uint32_t> v(pm.alphabet_count());
    for (size_t i = 0; i < v.size(); ++i) v[i] = pm.c_freq(i);
    return v;
  }
  static std::vector<uint32_t> snapshot_cum(const PModel& pm) {
    std::vector<uint32_t> v(pm.alphabet_count());
    for (size_t i = 0; i < v.size(); ++i) v[i] = pm.cum_freq(i);
    return v;
  }
  Context* ctx_;
  rc_model* m_ = nullptr;
  std::vector<uint32_t> c_;
  uint32_t total_ = 0;
};

// Encode many independent chunks (one reference Encoder each) in one launch.
inline std::vector<std::vector<uint8_t>> encode_chunks(
    const Model& m, const std::vector<std::vector<uint8_t>>& chunks) {
  const uint32_t n = (uint32_t)chunks.size();
  std::vector<uint64_t> sym_off(n + 1, 0), cap(n), out_off(n + 1, 0), out_len(n);
  std::vector<uint32_t> flags(n);
  for (uint32_t k = 0; k < n; ++k) {
    sym_off[k + 1] = sym_off[k] + chunks[k].size();
    cap[k] = m.slot_capacity(chunks[k].size());
  }
  std::vector<uint8_t> syms(sym_off[n] ? sym_off[n] : 1);
  for (uint32_t k = 0; k < n; ++k)
    std::copy(chunks[k].begin(), chunks[k].end(), syms.begin() + sym_off[k]);
  std::vector<uint8_t> out;
  for (int attempt = 0; attempt < 2; ++attempt) {
    for (uint32_t k = 0; k < n; ++k) out_off[k + 1] = out_off[k] + cap[k];
    out.assign(out_off[n] ? out_off[n] : 1, 0);
    rc_status s = rc_encode_host(m.ctx().get(), m.get(), syms.data(), sym_off.data(), n,
                                 out.data(), out_off.data(), out_len.data(), flags.data());
    if (s != RC_OK && s != RC_E_CHUNK) check(s, "rc_encode_host");
    bool retry = false;
    for (uint32_t k = 0; k < n; ++k)
      if (flags[k] == RC_F_CAPACITY) {  // exact length is known: retry with it
        cap[k] = (out_len[k] + 15) & ~(uint64_t)15;
        retry = true;
      }
    if (!retry) break;
  }
  std::vector<std::vector<uint8_t>> res(n);
  for (uint32_t k = 0; k < n; ++k) {
    if (flags[k])
      throw RangeCoderError("chunk " + std::to_string(k) + ": " + flag_string(flags[k]),
                            RC_E_CHUNK, flags[k]);
    res[k].assign(out.begin() + out_off[k], out.begin() + out_off[k] + out_len[k]);
  }
  return res;
}

// Decode many independent streams; counts[k] symbols each (out-of-band, sample_impl.rs:113-120)
inline std::vector<std::vector<uint8_t>> decode_chunks(
    const Model& m, const std::vector<std::vector<uint8_t>>& codes,
    const std::vector<uint64_t>& counts) {
  const uint32_t n = (uint32_t)codes.size();
  std::vector<uint64_t> code_off(n), code_len(n), sym_off(n + 1, 0);
  std::vector<uint32_t> flags(n);
  uint64_t tot = 0;
  for (uint32_t k = 0; k < n; ++k) {
    code_off[k] = tot;
    code_len[k] = codes[k].size();
    tot += codes[k].size();
    sym_off[k + 1] = sym_off[k] + counts.at(k);
  }
  std::vector<uint8_t> code(tot + 16, 0), syms(sym_off[n] ? sym_off[n] : 1);
  for (uint32_t k = 0; k < n; ++k)
    std::copy(codes[k].begin(), codes[k].end(), code.begin() + code_off[k]);
  rc_status s = rc_decode_host(m.ctx().get(), m.get(), code.data(), code_off.data(),
                               code_len.data(), syms.data(), sym_off.data(), n, flags.data());
  if (s != RC_OK && s != RC_E_CHUNK) check(s, "rc_decode_host");
  std::vector<std::vector<uint8_t>> res(n);
  for (uint32_t k = 0; k < n; ++k) {
    if (flags[k])
      throw RangeCoderError("chunk " + std::to_string(k) + ": " + flag_string(flags[k]),
                            RC_E_CHUNK, flags[k]);
    res[k].assign(syms.begin() + sym_off[k], syms.begin() + sym_off[k + 1]);
  }
  return res;
}

#if __has_include(<hip/hip_runtime_api.h>)
}  // namespace rc
#include <hip/hip_runtime_api.h>
namespace rc {

namespace detail {
// a device buffer, optionally filled from a host vector (synchronous copies)
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  explicit DevBuf(size_t n) : bytes(n ? n : 1) {
    if (hipMalloc(&p, bytes) != hipSuccess) throw RangeCoderError("hipMalloc", RC_E_DEVICE);
  }
  template <class T>
  explicit DevBuf(const std::vector<T>& v) : DevBuf(v.size() * sizeof(T)) {
    if (!v.empty() &&
        hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(p);
      throw RangeCoderError("hipMemcpy", RC_E_DEVICE);
    }
  }
  ~DevBuf() { (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void download(void* dst) const {
    if (hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
      throw RangeCoderError("hipMemcpy", RC_E_DEVICE);
  }
  uint8_t* u8() const { return (uint8_t*)p; }
  const uint64_t* u64() const { return (const uint64_t*)p; }
};

// n vectors (part(k), k < n) back to back, at least one element, with their offsets in off[n + 1]
template <class T, class Part>
std::vector<T> concat(uint32_t n, Part part, std::vector<uint64_t>& off, size_t spare = 0) {
  off.assign(n + 1, 0);
  for (uint32_t k = 0; k < n; ++k) off[k + 1] = off[k] + part(k).size();
  std::vector<T> all(off[n] + spare ? off[n] + spare : 1);
  for (uint32_t k = 0; k < n; ++k) std::copy(part(k).begin(), part(k).end(), all.begin() + off[k]);
  return all;
}

inline void throw_flagged(const std::vector<uint32_t>& flags) {
  for (size_t k = 0; k < flags.size(); ++k)
    if (flags[k])
      throw RangeCoderError("chunk " + std::to_string(k) + ": " + flag_string(flags[k]),
                            RC_E_CHUNK, flags[k]);
}

// Encode the chunks of syms (sym_off[n + 1]) into slots of slot(symbols) bytes with one
// batch(syms_dev, sym_off_dev, n, out_dev, out_off_dev, out_len_dev, flags_dev) call, and once
// more with exact slots if a chunk overflowed its first one.
template <class Sym, class Slot, class Batch>
std::vector<std::vector<uint8_t>> encode_chunks(rc_ctx* ctx, const std::vector<Sym>& syms,
                                                const std::vector<uint64_t>& sym_off, Slot slot,
                                                Batch batch) {
  const uint32_t n = (uint32_t)sym_off.size() - 1;
  std::vector<uint64_t> cap(n), out_off(n + 1, 0), out_len(n);
  std::vector<uint32_t> flags(n);
  for (uint32_t k = 0; k < n; ++k) cap[k] = slot(sym_off[k + 1] - sym_off[k]);
  DevBuf d_syms(syms), d_soff(sym_off), d_len(8ull * n), d_flags(4ull * n);
  std::vector<uint8_t> out;
  for (int attempt = 0; attempt < 2 && n; ++attempt) {
    for (uint32_t k = 0; k < n; ++k) out_off[k + 1] = out_off[k] + cap[k];
    DevBuf d_ooff(out_off), d_out(out_off[n] ? out_off[n] : 1);
    batch((const Sym*)d_syms.p, d_soff.u64(), n, d_out.u8(), d_ooff.u64(), (uint64_t*)d_len.p,
          (uint32_t*)d_flags.p);
    check(rc_ctx_synchronize(ctx), "rc_ctx_synchronize");
    d_len.download(out_len.data());
    d_flags.download(flags.data());
    out.resize(d_out.bytes);
    d_out.download(out.data());
    bool retry = false;
    for (uint32_t k = 0; k < n; ++k)
      if (flags[k] == RC_F_CAPACITY) {  // exact length is known: retry with it
        cap[k] = (out_len[k] + 15) & ~(uint64_t)15;
        retry = true;
      }
    if (!retry) break;
  }
  throw_flagged(flags);
  std::vector<std::vector<uint8_t>> res(n);
  for (uint32_t k = 0; k < n; ++k)
    res[k].assign(out.begin() + out_off[k], out.begin() + out_off[k] + out_len[k]);
  return res;
}

// Decode n streams, code(k) holding count(k) symbols (the count is out-of-band,
// sample_impl.rs:113-120), with one batch(code_dev, code_off_dev, code_len_dev, syms_dev,
// sym_off_dev, n, flags_dev) call.
template <class Sym, class Code, class Count, class Batch>
std::vector<std::vector<Sym>> decode_chunks(rc_ctx* ctx, uint32_t n, Code code_of, Count count,
                                            Batch batch) {
  std::vector<uint64_t> code_off, sym_off(n + 1, 0);
  const std::vector<uint8_t> code = concat<uint8_t>(n, code_of, code_off, 16);
  std::vector<uint64_t> code_len(n);
  std::vector<uint32_t> flags(n);
  for (uint32_t k = 0; k < n; ++k) {
    code_len[k] = code_of(k).size();
    sym_off[k + 1] = sym_off[k] + count(k);
  }
  code_off.pop_back();
  std::vector<Sym> syms(sym_off[n] ? sym_off[n] : 1);
  if (n) {
    DevBuf d_code(code), d_coff(code_off), d_clen(code_len), d_soff(sym_off),
        d_syms(sizeof(Sym) * syms.size()), d_flags(4ull * n);
    batch(d_code.u8(), d_coff.u64(), d_clen.u64(), (Sym*)d_syms.p, d_soff.u64(), n,
          (uint32_t*)d_flags.p);
    check(rc_ctx_synchronize(ctx), "rc_ctx_synchronize");
    d_flags.download(flags.data());
    d_syms.download(syms.data());
  }
  throw_flagged(flags);
  std::vector<std::vector<Sym>> res(n);
  for (uint32_t k = 0; k < n; ++k)
    res[k].assign(syms.begin() + sym_off[k], syms.begin() + sym_off[k + 1]);
  return res;
}
}  // namespace detail

// A static model set (rc_model_create_static_set): K tables over one alphabet and one
// total_freq, and batch coding with a model chosen per symbol -- symbol i of a chunk is coded as
// encoder.encode(&models[idx[i]], sym[i]) and decoded as decoder.decode(&models[idx[i]]).  The
// indexed entry points take device memory only, so the chunk helpers stage through buffers
// they allocate with the HIP runtime (hence this part needs its header).
class ModelSet {
 public:
  // one chunk: its symbols (encode) or code bytes (decode), and one model index per symbol
  struct Chunk {
    std::vector<uint8_t> data, idx;
  };

  ModelSet(Context& ctx, const std::vector<const PModel*>& models) : ctx_(&ctx) {
    if (models.empty()) throw RangeCoderError("empty model set", RC_E_BAD_MODEL);
    n_ = (uint32_t)models[0]->alphabet_count();
    total_ = models[0]->total_freq();
    for (const PModel* pm : models) {
      if (pm->alphabet_count() != n_ || pm->total_freq() != total_)
        throw RangeCoderError("the models of a set share one alphabet and one total_freq",
                              RC_E_BAD_MODEL);
      for (uint32_t i = 0; i < n_; ++i) {
        c_.push_back(pm->c_freq(i));
        cum_.push_back(pm->cum_freq(i));
      }
    }
    check(rc_model_create_static_set(ctx.get(), (uint32_t)models.size(), n_, c_.data(),
                                     cum_.data(), total_, &m_),
          "rc_model_create_static_set");
  }
  ~ModelSet() {
    if (m_) rc_model_destroy(m_);
  }
  ModelSet(const ModelSet&) = delete;
  ModelSet& operator=(const ModelSet&) = delete;
  rc_model* get() const { return m_; }
  Context& ctx() const { return *ctx_; }
  uint64_t slot_capacity(uint64_t n) const { return detail::slot_capacity(c_, total_, n); }

  // Encode many independent chunks, a model per symbol, in one launch.
  std::vector<std::vector<uint8_t>> encode_chunks(const std::vector<Chunk>& chunks) const {
    const uint32_t n = (uint32_t)chunks.size();
    for (uint32_t k = 0; k < n; ++k)
      if (chunks[k].data.size() != chunks[k].idx.size())
        throw RangeCoderError("chunk " + std::to_string(k) + ": one index per symbol", RC_E_ARG);
    std::vector<uint64_t> sym_off;
    const auto syms = detail::concat<uint8_t>(
        n, [&](uint32_t k) -> const std::vector<uint8_t>& { return chunks[k].data; }, sym_off);
    const detail::DevBuf d_idx(detail::concat<uint8_t>(
        n, [&](uint32_t k) -> const std::vector<uint8_t>& { return chunks[k].idx; }, sym_off));
    return detail::encode_chunks(
        ctx_->get(), syms, sym_off, [&](uint64_t len) { return slot_capacity(len); },
        [&](const uint8_t* s, const uint64_t* soff, uint32_t nc, uint8_t* out,
            const uint64_t* ooff, uint64_t* len, uint32_t* flags) {
          check(rc_encode_batch_indexed(ctx_->get(), m_, s, d_idx.u8(), soff, nc, out, ooff, len,
                                        flags),
                "rc_encode_batch_indexed");
        });
  }

  // Decode many independent streams: chunk k gives idx.size() symbols (the count is
  // out-of-band, sample_impl.rs:113-120), symbol i with model idx[i].
  std::vector<std::vector<uint8_t>> decode_chunks(const std::vector<Chunk>& chunks) const {
    const uint32_t n = (uint32_t)chunks.size();
    std::vector<uint64_t> sym_off;
    const detail::DevBuf d_idx(detail::concat<uint8_t>(
        n, [&](uint32_t k) -> const std::vector<uint8_t>& { return chunks[k].idx; }, sym_off));
    return detail::decode_chunks<uint8_t>(
        ctx_->get(), n, [&](uint32_t k) -> const std::vector<uint8_t>& { return chunks[k].data; },
        [&](uint32_t k) { return (uint64_t)chunks[k].idx.size(); },
        [&](const uint8_t* code, const uint64_t* coff, const uint64_t* clen, uint8_t* syms,
            const uint64_t* soff, uint32_t nc, uint32_t* flags) {
          check(rc_decode_batch_indexed(ctx_->get(), m_, code, coff, clen, d_idx.u8(), syms, soff,
                                        nc, flags),
                "rc_decode_batch_indexed");
        });
  }

 private:
  Context* ctx_;
  rc_model* m_ = nullptr;
  std::vector<uint32_t> c_, cum_;
  uint32_t n_ = 0, total_ = 0;
};

// A static chunk set (rc_model_create_chunk_set): K tables over one alphabet and one total_freq,
// and batch coding with a model chosen per CHUNK -- chunk k is coded exactly as a static Model of
// row class_of[k] codes it.  The chunk-set entry points take device memory only, so the chunk
// helpers stage through buffers they allocate with the HIP runtime.
class ChunkSet {
 public:
  ChunkSet(Context& ctx, const std::vector<const PModel*>& models) : ctx_(&ctx) {
    if (models.empty()) throw RangeCoderError("empty chunk set", RC_E_BAD_MODEL);
    n_ = (uint32_t)models[0]->alphabet_count();
    total_ = models[0]->total_freq();
    for (const PModel* pm : models) {
      if (pm->alphabet_count() != n_ || pm->total_freq() != total_)
        throw RangeCoderError("the models of a set share one alphabet and one total_freq",
                              RC_E_BAD_MODEL);
      for (uint32_t i = 0; i < n_; ++i) {
        c_.push_back(pm->c_freq(i));
        cum_.push_back(pm->cum_freq(i));
      }
    }
    check(rc_model_create_chunk_set(ctx.get(), (uint32_t)models.size(), n_, c_.data(),
                                    cum_.data(), total_, &m_),
          "rc_model_create_chunk_set");
  }
  ~ChunkSet() {
    if (m_) rc_model_destroy(m_);
  }
  ChunkSet(const ChunkSet&) = delete;
  ChunkSet& operator=(const ChunkSet&) = delete;
  rc_model* get() const { return m_; }
  Context& ctx() const { return *ctx_; }
  uint64_t slot_capacity(uint64_t n) const { return detail::slot_capacity(c_, total_, n); }

  // Encode many independent chunks in one launch, chunk k with row class_of[k].
  std::vector<std::vector<uint8_t>> encode_chunks(
      const std::vector<std::vector<uint8_t>>& chunks, const std::vector<uint8_t>& class_of) const {
    const uint32_t n = (uint32_t)chunks.size();
    if (class_of.size() != n) throw RangeCoderError("one class per chunk", RC_E_ARG);
    std::vector<uint64_t> sym_off;
    const auto syms = detail::concat<uint8_t>(
        n, [&](uint32_t k) -> const std::vector<uint8_t>& { return chunks[k]; }, sym_off);
    const detail::DevBuf d_cls(class_of);
    return detail::encode_chunks(
        ctx_->get(), syms, sym_off, [&](uint64_t len) { return slot_capacity(len); },
        [&](const uint8_t* s, const uint64_t* soff, uint32_t nc, uint8_t* out,
            const uint64_t* ooff, uint64_t* len, uint32_t* flags) {
          check(rc_encode_batch_chunk_set(ctx_->get(), m_, d_cls.u8(), s, soff, nc, out, ooff,
                                          len, flags),
                "rc_encode_batch_chunk_set");
        });
  }

  // Decode many independent streams: counts[k] symbols from codes[k] with row class_of[k] (the
  // count is out-of-band, sample_impl.rs:113-120).
  std::vector<std::vector<uint8_t>> decode_chunks(const std::vector<std::vector<uint8_t>>& codes,
                                                  const std::vector<uint64_t>& counts,
                                                  const std::vector<uint8_t>& class_of) const {
    const uint32_t n = (uint32_t)codes.size();
    if (class_of.size() != n || counts.size() != n)
      throw RangeCoderError("one class and one count per chunk", RC_E_ARG);
    const detail::DevBuf d_cls(class_of);
    return detail::decode_chunks<uint8_t>(
        ctx_->get(), n, [&](uint32_t k) -> const std::vector<uint8_t>& { return codes[k]; },
        [&](uint32_t k) { return counts[k]; },
        [&](const uint8_t* code, const uint64_t* coff, const uint64_t* clen, uint8_t* syms,
            const uint64_t* soff, uint32_t nc, uint32_t* flags) {
          check(rc_decode_batch_chunk_set(ctx_->get(), m_, d_cls.u8(), code, coff, clen, syms,
                                          soff, nc, flags),
                "rc_decode_batch_chunk_set");
        });
  }

 private:
  Context* ctx_;
  rc_model* m_ = nullptr;
  std::vector<uint32_t> c_, cum_;
  uint32_t n_ = 0, total_ = 0;
};

// A row's integer costs for fitting a chunk set (rc_cost_table): round(65536 log2(total / c)),
// RC_COST_NONE where c == 0.
inline std::vector<uint32_t> cost_table(const std::vector<uint32_t>& c_freq, uint32_t total) {
  std::vector<uint32_t> out(c_freq.size());
  check(rc_cost_table(c_freq.data(), (uint32_t)c_freq.size(), total, out.data()),
        "rc_cost_table");
  return out;
}

// An order-1 set (rc_model_create_order1_set): K tables over one alphabet and one total_freq
// plus a context map, and batch coding in which the previous symbol of the chunk picks the
// table -- symbol 0 of a chunk is coded with models[first_row], symbol i > 0 as
// encoder.encode(&models[ctx_map[sym[i-1]]], sym[i]), and decoded the same way from the symbols
// decoded so far.  The order-1 entry points take device memory only, so the chunk helpers stage
// through buffers they allocate with the HIP runtime.
class Order1Set {
 public:
  // ctx_map: one row per symbol of the alphabet (each < models.size()); first_row likewise
  Order1Set(Context& ctx, const std::vector<const PModel*>& models,
            const std::vector<uint8_t>& ctx_map, uint32_t first_row)
      : ctx_(&ctx) {
    if (models.empty()) throw RangeCoderError("empty model set", RC_E_BAD_MODEL);
    n_ = (uint32_t)models[0]->alphabet_count();
    total_ = models[0]->total_freq();
    if (ctx_map.size() < n_)
      throw RangeCoderError("the context map needs one row per symbol", RC_E_BAD_MODEL);
    for (const PModel* pm : models) {
      if (pm->alphabet_count() != n_ || pm->total_freq() != total_)
        throw RangeCoderError("the models of a set share one alphabet and one total_freq",
                              RC_E_BAD_MODEL);
      for (uint32_t i = 0; i < n_; ++i) {
        c_.push_back(pm->c_freq(i));
        cum_.push_back(pm->cum_freq(i));
      }
    }
    check(rc_model_create_order1_set(ctx.get(), (uint32_t)models.size(), n_, c_.data(),
                                     cum_.data(), total_, ctx_map.data(), first_row, &m_),
          "rc_model_create_order1_set");
  }
  ~Order1Set() {
    if (m_) rc_model_destroy(m_);
  }
  Order1Set(const Order1Set&) = delete;
  Order1Set& operator=(const Order1Set&) = delete;
  rc_model* get() const { return m_; }
  Context& ctx() const { return *ctx_; }
  uint64_t slot_capacity(uint64_t n) const { return detail::slot_capacity(c_, total_, n); }

  // Encode many independent chunks of symbols in one launch.
  std::vector<std::vector<uint8_t>> encode_chunks(
      const std::vector<std::vector<uint8_t>>& chunks) const {
    std::vector<uint64_t> sym_off;
    const auto syms = detail::concat<uint8_t>(
        (uint32_t)chunks.size(),
        [&](uint32_t k) -> const std::vector<uint8_t>& { return chunks[k]; }, sym_off);
    return detail::encode_chunks(
        ctx_->get(), syms, sym_off, [&](uint64_t len) { return slot_capacity(len); },
        [&](const uint8_t* s, const uint64_t* soff, uint32_t nc, uint8_t* out,
            const uint64_t* ooff, uint64_t* len, uint32_t* flags) {
          check(rc_encode_batch_order1(ctx_->get(), m_, s, soff, nc, out, ooff, len, flags),
                "rc_encode_batch_order1");
        });
  }

  // Decode many independent streams: counts[k] symbols from codes[k] (the count is out-of-band,
  // sample_impl.rs:113-120).
  std::vector<std::vector<uint8_t>> decode_chunks(const std::vector<std::vector<uint8_t>>& codes,
                                                  const std::vector<uint64_t>& counts) const {
    const uint32_t n = (uint32_t)codes.size();
    if (counts.size() != n) throw RangeCoderError("one symbol count per stream", RC_E_ARG);
    return detail::decode_chunks<uint8_t>(
        ctx_->get(), n, [&](uint32_t k) -> const std::vector<uint8_t>& { return codes[k]; },
        [&](uint32_t k) { return counts[k]; },
        [&](const uint8_t* code, const uint64_t* coff, const uint64_t* clen, uint8_t* syms,
            const uint64_t* soff, uint32_t nc, uint32_t* flags) {
          check(rc_decode_batch_order1(ctx_->get(), m_, code, coff, clen, syms, soff, nc, flags),
                "rc_decode_batch_order1");
        });
  }

 private:
  Context* ctx_;
  rc_model* m_ = nullptr;
  std::vector<uint32_t> c_, cum_;
  uint32_t n_ = 0, total_ = 0;
};

// A wide static model (rc_model_create_static_wide): one table over up to RC_MAX_WIDE_SYMBOLS
// 16-bit symbols -- the reference's PModel is indexed with usize (pmodel.rs:6-12), and a
// FreqTable::new(alphabet_count) may hold any number of symbols.  Symbol i of a chunk is coded as
// encoder.encode(&table, sym[i]) and decoded as decoder.decode(&table).  The wide entry points
// take device memory only: encode_batch / decode_batch are their typed (uint16_t) forms, and the
// chunk helpers stage through buffers they allocate with the HIP runtime.
class WideModel {
 public:
  WideModel(Context& ctx, const PModel& pm) : ctx_(&ctx) {
    const uint32_t n = (uint32_t)pm.alphabet_count();
    for (uint32_t i = 0; i < n; ++i) {
      c_.push_back(pm.c_freq(i));
      cum_.push_back(pm.cum_freq(i));
    }
    total_ = pm.total_freq();
    create();
  }
  WideModel(Context& ctx, const std::vector<uint32_t>& c, const std::vector<uint32_t>& cum,
            uint32_t total)
      : ctx_(&ctx), c_(c), cum_(cum), total_(total) {
    if (c.size() != cum.size()) throw RangeCoderError("c and cum differ in length", RC_E_BAD_MODEL);
    create();
  }
  ~WideModel() {
    if (m_) rc_model_destroy(m_);
  }
  WideModel(const WideModel&) = delete;
  WideModel& operator=(const WideModel&) = delete;
  rc_model* get() const { return m_; }
  Context& ctx() const { return *ctx_; }
  uint64_t slot_capacity(uint64_t n) const { return detail::slot_capacity(c_, total_, n); }

  // rc_encode_batch_wide / rc_decode_batch_wide on typed device pointers (asynchronous)
  void encode_batch(const uint16_t* syms_dev, const uint64_t* sym_off_dev, uint32_t n_chunks,
                    uint8_t* out_dev, const uint64_t* out_off_dev, uint64_t* out_len_dev,
                    uint32_t* flags_dev) const {
    check(rc_encode_batch_wide(ctx_->get(), m_, syms_dev, sym_off_dev, n_chunks, out_dev,
                               out_off_dev, out_len_dev, flags_dev),
          "rc_encode_batch_wide");
  }
  void decode_batch(const uint8_t* code_dev, const uint64_t* code_off_dev,
                    const uint64_t* code_len_dev, uint16_t* syms_out_dev,
                    const uint64_t* sym_off_dev, uint32_t n_chunks, uint32_t* flags_dev) const {
    check(rc_decode_batch_wide(ctx_->get(), m_, code_dev, code_off_dev, code_len_dev,
                               syms_out_dev, sym_off_dev, n_chunks, flags_dev),
          "rc_decode_batch_wide");
  }

  // Encode many independent chunks of 16-bit symbols in one launch.
  std::vector<std::vector<uint8_t>> encode_chunks(
      const std::vector<std::vector<uint16_t>>& chunks) const {
    std::vector<uint64_t> sym_off;
    const auto syms = detail::concat<uint16_t>(
        (uint32_t)chunks.size(),
        [&](uint32_t k) -> const std::vector<uint16_t>& { return chunks[k]; }, sym_off);
    return detail::encode_chunks(
        ctx_->get(), syms, sym_off, [&](uint64_t len) { return slot_capacity(len); },
        [&](const uint16_t* s, const uint64_t* soff, uint32_t nc, uint8_t* out,
            const uint64_t* ooff, uint64_t* len, uint32_t* flags) {
          encode_batch(s, soff, nc, out, ooff, len, flags);
        });
  }

  // Decode many independent streams; counts[k] symbols each (out-of-band,
  // sample_impl.rs:113-120)
  std::vector<std::vector<uint16_t>> decode_chunks(const std::vector<std::vector<uint8_t>>& codes,
                                                   const std::vector<uint64_t>& counts) const {
    return detail::decode_chunks<uint16_t>(
        ctx_->get(), (uint32_t)codes.size(),
        [&](uint32_t k) -> const std::vector<uint8_t>& { return codes[k]; },
        [&](uint32_t k) { return counts.at(k); },
        [&](const uint8_t* code, const uint64_t* coff, const uint64_t* clen, uint16_t* syms,
            const uint64_t* soff, uint32_t nc, uint32_t* flags) {
          decode_batch(code, coff, clen, syms, soff, nc, flags);
        });
  }

 private:
  void create() {
    check(rc_model_create_static_wide(ctx_->get(), (uint32_t)c_.size(), c_.data(), cum_.data(),
                                      total_, &m_),
          "rc_model_create_static_wide");
  }
  Context* ctx_;
  rc_model* m_ = nullptr;
  std::vector<uint32_t> c_, cum_;
  uint32_t total_ = 0;
};

// A wide16 static model (rc_model_create_static_wide16): WideModel's interface over an alphabet of
// up to RC_MAX_WIDE16_SYMBOLS (2^16) 16-bit symbols, its tables in device memory.  For an
// alphabet WideModel accepts too, both give the same bytes.
class Wide16Model {
 public:
  Wide16Model(Context& ctx, const PModel& pm) : Wide16Model(ctx, pm, false) {}
  Wide16Model(Context& ctx, const std::vector<uint32_t>& c, const std::vector<uint32_t>& cum,
              uint32_t total)
      : Wide16Model(ctx, c, cum, total, false) {}
  ~Wide16Model() {
    if (m_) rc_model_destroy(m_);
  }
  Wide16Model(const Wide16Model&) = delete;
  Wide16Model& operator=(const Wide16Model&) = delete;
  rc_model* get() const { return m_; }
  Context& ctx() const { return *ctx_; }
  uint64_t slot_capacity(uint64_t n) const { return detail::slot_capacity(c_, total_, n); }

  // rc_encode_batch_wide16 / rc_decode_batch_wide16 on typed device pointers (asynchronous)
  void encode_batch(const uint16_t* syms_dev, const uint64_t* sym_off_dev, uint32_t n_chunks,
                    uint8_t* out_dev, const uint64_t* out_off_dev, uint64_t* out_len_dev,
                    uint32_t* flags_dev) const {
    check(rc_encode_batch_wide16(ctx_->get(), m_, syms_dev, sym_off_dev, n_chunks, out_dev,
                                 out_off_dev, out_len_dev, flags_dev),
          "rc_encode_batch_wide16");
  }
  void decode_batch(const uint8_t* code_dev, const uint64_t* code_off_dev,
                    const uint64_t* code_len_dev, uint16_t* syms_out_dev,
                    const uint64_t* sym_off_dev, uint32_t n_chunks, uint32_t* flags_dev) const {
    check(rc_decode_batch_wide16(ctx_->get(), m_, code_dev, code_off_dev, code_len_dev,
                                 syms_out_dev, sym_off_dev, n_chunks, flags_dev),
          "rc_decode_batch_wide16");
  }

  // Encode many independent chunks of 16-bit symbols in one launch.
  std::vector<std::vector<uint8_t>> encode_chunks(
      const std::vector<std::vector<uint16_t>>& chunks) const {
    std::vector<uint64_t> sym_off;
    const auto syms = detail::concat<uint16_t>(
        (uint32_t)chunks.size(),
        [&](uint32_t k) -> const std::vector<uint16_t>& { return chunks[k]; }, sym_off);
    return detail::encode_chunks(
        ctx_->get(), syms, sym_off, [&](uint64_t len) { return slot_capacity(len); },
        [&](const uint16_t* s, const uint64_t* soff, uint32_t nc, uint8_t* out,
            const uint64_t* ooff, uint64_t* len, uint32_t* flags) {
          encode_batch(s, soff, nc, out, ooff, len, flags);
        });
  }

  // Decode many independent streams; counts[k] symbols each (out-of-band,
  // sample_impl.rs:113-120)
  std::vector<std::vector<uint16_t>> decode_chunks(const std::vector<std::vector<uint8_t>>& codes,
                                                   const std::vector<uint64_t>& counts) const {
    return detail::decode_chunks<uint16_t>(
        ctx_->get(), (uint32_t)codes.size(),
        [&](uint32_t k) -> const std::vector<uint8_t>& { return codes[k]; },
        [&](uint32_t k) { return counts.at(k); },
        [&](const uint8_t* code, const uint64_t* coff, const uint64_t* clen, uint16_t* syms,
            const uint64_t* soff, uint32_t nc, uint32_t* flags) {
          decode_batch(code, coff, clen, syms, soff, nc, flags);
        });
  }

 protected:
  // fine: the table is a wide16 fine model's (Wide16FineModel), which the same batch calls code
  Wide16Model(Context& ctx, const PModel& pm, bool fine) : ctx_(&ctx) {
    const uint32_t n = (uint32_t)pm.alphabet_count();
    for (uint32_t i = 0; i < n; ++i) {
      c_.push_back(pm.c_freq(i));
      cum_.push_back(pm.cum_freq(i));
    }
    total_ = pm.total_freq();
    create(fine);
  }
  Wide16Model(Context& ctx, const std::vector<uint32_t>& c, const std::vector<uint32_t>& cum,
              uint32_t total, bool fine)
      : ctx_(&ctx), c_(c), cum_(cum), total_(total) {
    if (c.size() != cum.size()) throw RangeCoderError("c and cum differ in length", RC_E_BAD_MODEL);
    create(fine);
  }

 private:
  void create(bool fine) {
    if (fine)
      check(rc_model_create_static_wide16_fine(ctx_->get(), (uint32_t)c_.size(), c_.data(),
                                               cum_.data(), total_, &m_),
            "rc_model_create_static_wide16_fine");
    else
      check(rc_model_create_static_wide16(ctx_->get(), (uint32_t)c_.size(), c_.data(),
                                          cum_.data(), total_, &m_),
            "rc_model_create_static_wide16");
  }
  Context* ctx_;
  rc_model* m_ = nullptr;
  std::vector<uint32_t> c_, cum_;
  uint32_t total_ = 0;
};

// A wide16 fine model (rc_model_create_static_wide16_fine): Wide16Model's interface for a table
// whose total lies above 2^16, up to RC_MAX_WIDE16_FINE_TOTAL (2^24).  A table with a smaller total
// is Wide16Model's and is refused here.
class Wide16FineModel : public Wide16Model {
 public:
  Wide16FineModel(Context& ctx, const PModel& pm) : Wide16Model(ctx, pm, true) {}
  Wide16FineModel(Context& ctx, const std::vector<uint32_t>& c, const std::vector<uint32_t>& cum,
                  uint32_t total)
      : Wide16Model(ctx, c, cum, total, true) {}
};
#endif  // the HIP runtime API header

// RangeCoder (src/range_coder.rs:7-146): the public accessors of a coder state (a snapshot: a
// stream's state lives with its GPU calls, rc_stream_state)
class RangeCoder {
 public:
  static constexpr uint64_t TOP8 = 1ull << 56;   // range_coder.rs:23
  static constexpr uint64_t TOP16 = 1ull << 48;  // range_coder.rs:24
  RangeCoder() = default;                         // Default (:13-20)
  RangeCoder(uint64_t lower_bound, uint64_t range) : low_(lower_bound), range_(range) {}
  static RangeCoder new_() { return RangeCoder(); }
  uint64_t lower_bound() const { return low_; }  // :30-32
  uint64_t range() const { return range_; }      // :33-35
  uint64_t range_par_total(uint32_t total_freq) const {  // :38-40
    if (total_freq == 0) throw RangeCoderError("range_par_total: attempt to divide by zero");
    return range_ / total_freq;
  }
  uint64_t upper_bound() const {  // :138-146
    const uint64_t u = low_ + range_;
    if (u < low_) throw RangeCoderError("UpperBoundOverflow");
    return u;
  }
  bool operator==(const RangeCoder& o) const { return low_ == o.low_ && range_ == o.range_; }

 private:
  uint64_t low_ = 0, range_ = ~0ull;
};

inline void throw_flags(uint32_t f, const std::string& where) {
  if (f) throw RangeCoderError(where + ": " + flag_string(f), RC_E_CHUNK, f);
}

// The reference's error for a BAD_MODEL symbol coded from state (low, range) with (c, cum,
// total): param_update's own arithmetic (range_coder.rs:53-81, :138-146; u64 products wrap).
[[noreturn]] inline void throw_bad_model(uint64_t low, uint64_t range, uint32_t c, uint32_t cum,
                                         uint32_t total, const std::string& where) {
  RangeCoderError e(where + ": BAD_MODEL", RC_E_CHUNK, RC_F_BAD_MODEL);
  if (total == 0) {
    e = RangeCoderError(where + ": range_par_total: attempt to divide by zero", RC_E_CHUNK,
                        RC_F_BAD_MODEL);
    e.kind = RangeCoderError::DIVIDE_BY_ZERO;
    throw e;
  }
  const uint64_t r = range / total, nr = r * c, add = r * cum;
  if (low + add < add) {
    e = RangeCoderError(where + ": LowerBoundOverflow", RC_E_CHUNK, RC_F_BAD_MODEL);
    e.kind = RangeCoderError::LOWER_BOUND_OVERFLOW;
    e.lower_bound = low, e.add_val = add, e.range = nr;
  } else if (low + add + nr < nr) {
    e = RangeCoderError(where + ": UpperBoundOverflow", RC_E_CHUNK, RC_F_BAD_MODEL);
    e.kind = RangeCoderError::UPPER_BOUND_OVERFLOW;
    e.lower_bound = low + add, e.range = nr;
  }
  throw e;
}

class Encoder;

// Encoder::encode's return value (encoder.rs:34-36: the bytes that symbol settled).  Symbols
// are staged and coded on the GPU in batches; converting to uint32_t flushes them if needed.
// Valid while its Encoder lives.
class ByteCount {
 public:
  ByteCount(Encoder* e, uint64_t i) : e_(e), i_(i) {}
  operator uint32_t() const;

 private:
  Encoder* e_;
  uint64_t i_;
};

// Encoder (src/encoder.rs:7-55) for one stream, with the reference's per-call semantics:
// encode() reads (c_freq(index), cum_freq(index), total_freq()) at that call
// (encoder.rs:24-31), so a PModel the caller changes between calls is coded exactly as the
// reference codes it.  The staged triples are coded by the resumable stream kernel
// (rc_stream_encode_host) when a result is needed: peek_code(), range_coder(), finish(), a
// ByteCount's value, or every 2^20 symbols.  No length limit.
class Encoder {
 public:
  static constexpr size_t FLUSH_AT = 1u << 20;
  explicit Encoder(Context& ctx = Context::default_context()) : ctx_(&ctx) {}
  Encoder(const Encoder&) = delete;
  Encoder& operator=(const Encoder&) = delete;
  static Encoder new_() { return Encoder(); }  // encoder.rs:14-16

  ByteCount encode(const PModel& pm, size_t index) {  // encoder.rs:24-37
    if (finished_) throw RangeCoderError("encode after finish", RC_E_CHUNK, RC_F_FINISHED);
    if (index >= pm.alphabet_count())  // sample_impl.rs:19: get(index).unwrap() panics
      throw RangeCoderError("symbol index outside the alphabet", RC_E_CHUNK, RC_F_BAD_SYMBOL);
    const uint32_t c = pm.c_freq(index), cum = pm.cum_freq(index), total = pm.total_freq();
    if (c == 0)  // range_coder.rs:83-85 would never terminate
      throw RangeCoderError("encode: c_freq == 0", RC_E_CHUNK, RC_F_ZERO_FREQ);
    if (total == 0)  // range_coder.rs:38-40 divides by zero
      throw RangeCoderError("encode: total_freq == 0", RC_E_CHUNK, RC_F_BAD_MODEL);
    trip_.insert(trip_.end(), {c, cum, total});
    const uint64_t i = staged0_ + trip_.size() / 3 - 1;
    if (trip_.size() >= 3 * FLUSH_AT) flush(false);
    return ByteCount(this, i);
  }
  const std::vector<uint8_t>& peek_code() {  // encoder.rs:18-20
    flush(false);
    return code_;
  }
  RangeCoder range_coder() {  // the pub field of encoder.rs:8 (a snapshot)
    flush(false);
    return RangeCoder(st_.lower_bound, st_.range);
  }
  std::vector<uint8_t> finish() {  // encoder.rs:40-46
    if (finished_) throw RangeCoderError("finish twice", RC_E_CHUNK, RC_F_FINISHED);
    flush(true);
    finished_ = true;
    return code_;
  }
  uint32_t count(uint64_t i) {
    if (i >= staged0_) flush(false);
    if (i >= counts_.size()) throw RangeCoderError("symbol not coded (an earlier one failed)");
    return counts_[i];
  }

 private:
  void flush(bool finish) {
    const uint64_t n = trip_.size() / 3;
    if (n == 0 && !finish) return;
    throw_flags(st_.flags, "encode");
    const uint64_t cap = RC_STREAM_MAX_BYTES(n, finish);
    std::vector<uint8_t> out(cap ? cap : 1), nb(n ? n : 1);
    uint64_t len = 0;
    uint32_t fl = 0;
    const uint64_t n0 = st_.n;
    const rc_status s = rc_stream_encode_host(ctx_->get(), &st_, trip_.data(), n, out.data(), cap,
                                              &len, nb.data(), finish ? 1u : 0u, &fl);
    if (s != RC_OK && s != RC_E_CHUNK) check(s, "rc_stream_encode_host");
    code_.insert(code_.end(), out.begin(), out.begin() + len);
    const uint64_t done = st_.n - n0;
    counts_.insert(counts_.end(), nb.begin(), nb.begin() + done);
    staged0_ += n;
    const std::string where = "encode (symbol " + std::to_string(st_.n) + ")";
    if ((fl & RC_F_BAD_MODEL) && done < n) {
      const uint32_t* t = trip_.data() + 3 * done;
      const uint32_t c = t[0], cum = t[1], total = t[2];
      trip_.clear();
      throw_bad_model(st_.lower_bound, st_.range, c, cum, total, where);
    }
    trip_.clear();
    throw_flags(fl, where);
  }
  Context* ctx_;
  rc_stream_state st_ = RC_STREAM_STATE_INIT;
  std::vector<uint8_t> code_, counts_;
  std::vector<uint32_t> trip_;
  uint64_t staged0_ = 0;
  bool finished_ = false;
};

inline ByteCount::operator uint32_t() const { return e_->count(i_); }

// Decoder (src/decoder.rs:6-55) for one stream, with the reference's per-call semantics:
// decode() reads the model's table at that call and decodes with FreqTable::find_index's
// binary search and param_update (sample_impl.rs:27-45, decoder.rs:38-54) on the GPU
// (rc_stream_decode_host).  Symbols are decoded ahead in blocks that double while the table
// stays the same; when the caller's table changes the state at that symbol is re-derived, so
// every symbol is decoded with the table held at its call.  A PModel that overrides find_index
// gets it called per symbol and its index decoded (one GPU step per symbol, launch-bound).
class Decoder {
 public:
  static constexpr uint64_t MAX_BLOCK = 1u << 20;
  // Decoder::new (decoder.rs:14-23): a code shorter than 8 bytes panics there
  explicit Decoder(std::vector<uint8_t> code, Context& ctx = Context::default_context())
      : Decoder(std::move(code), ~0ull, ctx) {}
  // n_symbols: the out-of-band count (sample_impl.rs:113-120); only bounds the decode-ahead
  Decoder(std::vector<uint8_t> code, uint64_t n_symbols, Context& ctx = Context::default_context())
      : ctx_(&ctx), code_(std::move(code)), limit_(n_symbols) {
    if (code_.size() < 8)
      throw RangeCoderError("code shorter than 8 bytes", RC_E_CHUNK, RC_F_TRUNCATED);
    Table t{{1}, {0}, 1};
    run(start_, t, 0, nullptr);  // prime the data window
    end_ = start_;
  }
  static Decoder new_(std::vector<uint8_t> code) { return Decoder(std::move(code)); }

  size_t decode(const PModel& pm) {  // decoder.rs:38-54
    if (!pm.canonical_find_index()) {
      const size_t idx = pm.find_index(*this);  // reads range_coder() / data() at this symbol
      if (idx != PModel::kCanonical) return decode_index(pm, idx);
    }
    table_of(pm, tmp_);  // (into reused vectors: no allocation per call)
    Table& t = tmp_;
    const bool same = have_ && t == sig_;
    if (same && bpos_ < buf_.size()) {
      ++taken_;
      return buf_[bpos_++];
    }
    if (same && err_) decode_error(end_, t, err_);
    block_ = (same && bpos_ == buf_.size()) ? std::min<uint64_t>(2 * block_, MAX_BLOCK) : 1;
    rc_stream_state st = here();
    uint64_t n = block_;
    if (limit_ != ~0ull) n = std::max<uint64_t>(1, std::min<uint64_t>(n, limit_ - taken_));
    const rc_stream_state start = st;
    std::vector<uint8_t>& out = spare_;  // (reused: swapped with buf_ below)
    out.resize(n);
    const uint32_t fl = run(st, t, n, out.data());
    out.resize(st.n - start.n);
    start_ = start;
    end_ = st;
    buf_.swap(out);
    bpos_ = 0;
    std::swap(sig_, t);  // (member-wise: the vectors swap their storage)
    have_ = true;
    err_ = fl;
    if (buf_.empty()) decode_error(start, sig_, fl);
    ++taken_;
    return buf_[bpos_++];
  }
  RangeCoder range_coder() const {  // decoder.rs:24-26 (a snapshot)
    const rc_stream_state st = here();
    return RangeCoder(st.lower_bound, st.range);
  }
  uint64_t data() const { return here().data; }  // decoder.rs:27-29

 private:
  struct Table {
    std::vector<uint32_t> c, cum;
    uint32_t total;
    bool operator==(const Table& o) const { return total == o.total && c == o.c && cum == o.cum; }
  };
  // decoder.rs:38-54 with the caller's find_index: param_update and shift_left_buffer for the
  // index it returned, on the GPU (a one-entry table, so the kernel's search has no choice)
  size_t decode_index(const PModel& pm, size_t idx) {
    const rc_stream_state st = here();
    Table t{{pm.c_freq(idx)}, {pm.cum_freq(idx)}, pm.total_freq()};
    rc_stream_state nxt = st;
    uint8_t sym = 0;
    const uint32_t fl = run(nxt, t, 1, &sym);
    const std::string where = "decode (symbol " + std::to_string(taken_) + ")";
    if (nxt.n == st.n) {
      if (fl & RC_F_BAD_MODEL) throw_bad_model(st.lower_bound, st.range, t.c[0], t.cum[0], t.total, where);
      throw_flags(fl, where);
    }
    start_ = end_ = nxt;
    buf_.clear();
    bpos_ = 0;
    have_ = false;
    err_ = 0;
    ++taken_;
    return idx;
  }
  // the reference's error for a decode that stopped at state st under table t
  [[noreturn]] void decode_error(const rc_stream_state& st, const Table& t, uint32_t fl) const {
    const std::string where = "decode (symbol " + std::to_string(taken_) + ")";
    if ((fl & RC_F_BAD_MODEL) && t.total && !t.c.empty()) {
      // the index FreqTable::find_index chose (sample_impl.rs:29-44), for the error's payload
      const uint64_t rf = (st.data - st.lower_bound) / (st.range / t.total);
      size_t left = 0, right = t.c.size() - 1;
      while (left < right) {
        const size_t mid = (left + right) / 2;
        if ((uint64_t)t.cum[mid + 1] <= rf) left = mid + 1;
        else right = mid;
      }
      throw_bad_model(st.lower_bound, st.range, t.c[left], t.cum[left], t.total, where);
    }
    if (fl & RC_F_BAD_MODEL) throw_bad_model(st.lower_bound, st.range, 0, 0, t.total, where);
    throw_flags(fl ? fl : RC_F_CORRUPT, where);
    throw RangeCoderError(where);
  }
  static void table_of(const PModel& pm, Table& t) {
    const size_t n = pm.alphabet_count();
    t.c.resize(n);
    t.cum.resize(n);
    for (size_t i = 0; i < n; ++i) {
      t.c[i] = pm.c_freq(i);
      t.cum[i] = pm.cum_freq(i);
    }
    t.total = pm.total_freq();
  }
  uint32_t run(rc_stream_state& st, const Table& t, uint64_t n, uint8_t* out) const {
    uint32_t fl = 0;
    uint8_t dummy = 0;
    const rc_status s = rc_stream_decode_host(ctx_->get(), t.c.data(), t.cum.data(),
                                              (uint32_t)t.c.size(), t.total, &st, code_.data(),
                                              code_.size(), out ? out : &dummy, n, &fl);
    if (s != RC_OK && s != RC_E_CHUNK) check(s, "rc_stream_decode_host");
    return fl;
  }
  // the state at the current symbol (re-derived inside a block, which then starts here)
  rc_stream_state here() const {
    if (bpos_ == 0) return start_;
    if (bpos_ == buf_.size()) {
      rc_stream_state st = end_;
      st.flags = 0;
      return st;
    }
    rc_stream_state st = start_;
    std::vector<uint8_t> tmp(bpos_);
    run(st, sig_, bpos_, tmp.data());
    start_ = st;
    buf_.erase(buf_.begin(), buf_.begin() + bpos_);
    bpos_ = 0;
    return st;
  }
  // (the decode-ahead block is a cache of the stream: range_coder() / data() re-derive into it)
  Context* ctx_;
  std::vector<uint8_t> code_;
  mutable std::vector<uint8_t> buf_;
  uint64_t limit_;
  mutable rc_stream_state start_ = RC_STREAM_STATE_INIT;
  rc_stream_state end_ = RC_STREAM_STATE_INIT;
  mutable size_t bpos_ = 0;
  Table sig_, tmp_;                // the table of the decoded-ahead block; the caller's, read now
  std::vector<uint8_t> spare_;     // the next block's symbols before they replace buf_
  bool have_ = false;
  uint32_t err_ = 0;
  uint64_t block_ = 1, taken_ = 0;
};

}  // namespace rc

#endif  // RANGE_CODER_AMD_HPP
