// rc_wide16_fine_tables.h — the device tables of a wide16 fine model (rc_wide16_fine.h), built on
// the host from a checked table (cum[0] = 0, cum[i + 1] = cum[i] + c[i], sum(c) = total, 1 <= n <=
// 65536, 65536 < total <= 2^24).  Plain C++ with no device code and no HIP header, so that a
// stand-alone host program can include it (tests/native/wide16_fine_tables_check.cpp).
//
// One entry per q, the wide16 models' decoder table, is out of reach here (2^24 halfwords), so the
// decoder's tables are laid over the occupied symbols (c > 0) alone, in rank order: rank j is the
// j-th occupied symbol.  A q is found through a bucket table over its top bits, which names the
// rank that owns the bucket's first q; the ranks of one bucket are then at most 2^shift + 1
// however long the runs of zero-frequency symbols between them, and every rank read has c > 0.
#pragma once
#include <stdint.h>

#include <vector>

#include "range_coder.h"

struct Wide16FineTables {
  // encoder: (cum, c) per symbol, enc_core's SM = 0 form: a symbol with c = 0 keeps c = 0, and
  // entry n, which a symbol >= n is clamped to, is the poison entry (0xFFFFFFFF, 0).  n = 65536
  // has no poison entry: every 16-bit value is a symbol.  2 words per entry.
  std::vector<uint32_t> enc;
  uint32_t enc_clamp;  // the index a symbol is clamped to: min(s, enc_clamp)
  // decoder: the m occupied symbols in ascending order (padded with one zero to an even count)
  std::vector<uint16_t> occ;
  uint32_t m;
  // decoder: rcum[j] = cum[occ[j]] for j < m, rcum[m] = rcum[m + 1] = total, so that rank j's
  // frequency is rcum[j + 1] - rcum[j]
  std::vector<uint32_t> rcum;
  // decoder: bucket[b] = the rank that owns q = b << shift, for every b with b << shift < total;
  // the entries after those, up to bucket[2^bits] (a sentinel, so that bucket[b + 1] is readable
  // for every b < 2^bits) and one more that evens the count, hold m - 1, the rank that owns
  // total - 1.  A q of bucket b lies at a rank in [bucket[b], bucket[b + 1]].
  std::vector<uint16_t> bucket;
  uint32_t bits, shift;  // shift = bitlen(total - 1) - bits
};

static inline uint32_t wide16_fine_bitlen(uint32_t v) {
  uint32_t b = 0;
  while (v) ++b, v >>= 1;
  return b;
}

// bits: log2 of the bucket count, at most 16 (rc_wide16_fine_plan's dec_bits)
static inline Wide16FineTables wide16_fine_build_tables(uint32_t n, const uint32_t* c,
                                                        const uint32_t* cum, uint32_t total,
                                                        uint32_t bits) {
  Wide16FineTables t;
  const bool poison = n < 65536u;
  t.enc_clamp = poison ? n : 65535u;
  t.enc.resize(2 * (size_t)(n + (poison ? 1u : 0u)));
  for (uint32_t s = 0; s < n; ++s) {
    t.enc[2 * (size_t)s] = cum[s];
    t.enc[2 * (size_t)s + 1] = c[s];
  }
  if (poison) {
    t.enc[2 * (size_t)n] = 0xFFFFFFFFu;
    t.enc[2 * (size_t)n + 1] = 0u;
  }
  for (uint32_t s = 0; s < n; ++s)
    if (c[s]) {
      t.occ.push_back((uint16_t)s);
      t.rcum.push_back(cum[s]);
    }
  t.m = (uint32_t)t.occ.size();
  if (t.m & 1u) t.occ.push_back(0);
  t.rcum.push_back(total);
  t.rcum.push_back(total);
  t.bits = bits;
  t.shift = wide16_fine_bitlen(total - 1) - bits;
  const uint32_t nb = 1u << bits, last = (total - 1) >> t.shift;
  t.bucket.resize((size_t)nb + 2);
  uint32_t j = 0;
  for (uint32_t b = 0; b <= last; ++b) {
    const uint32_t q = b << t.shift;
    while (t.rcum[j + 1] <= q) ++j;  // (q < total = rcum[m]: j stays below m)
    t.bucket[b] = (uint16_t)j;
  }
  for (size_t b = (size_t)last + 1; b < t.bucket.size(); ++b) t.bucket[b] = (uint16_t)(t.m - 1);
  return t;
}

// FreqTable::find_index(q) for q < total through the tables, as the kernel goes: the bucket, the
// last rank of [bucket[b], bucket[b + 1]] whose rcum is <= q, its symbol.  *steps: the rcum reads
// of the search (0 when the bucket names one rank).
static inline uint32_t wide16_fine_lookup(const Wide16FineTables& t, uint32_t q,
                                          uint32_t* rank_out, uint32_t* steps) {
  const uint32_t b = q >> t.shift;
  uint32_t lo = t.bucket[b], hi = t.bucket[b + 1], n = 0;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (t.rcum[mid] <= q) lo = mid;
    else hi = mid - 1;
    ++n;
  }
  if (rank_out) *rank_out = lo;
  if (steps) *steps = n;
  return t.occ[lo];
}
