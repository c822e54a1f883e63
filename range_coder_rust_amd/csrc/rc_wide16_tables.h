// rc_wide16_tables.h — the device tables of a wide16 static model (rc_wide16.h), built on the
// host from a checked table (cum[0] = 0, cum[i + 1] = cum[i] + c[i], sum(c) = total, 1 <= n <=
// 65536, 256 <= total <= 65536).  Plain C++ with no device code and no HIP header, so that a
// stand-alone host program can include it (tests/native/wide16_tables_check.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "range_coder.h"

struct Wide16Tables {
  // encoder: (cum | flag << 24, c) per symbol, the wide coders' layout 0: a symbol with c = 0 is
  // (RC_F_ZERO_FREQ << 24, 1), and entry n, which a symbol >= n is clamped to, is the poison
  // entry (RC_F_BAD_SYMBOL << 24, 1).  n = 65536 has no poison entry: every 16-bit value is a
  // symbol.  2 words per entry.
  std::vector<uint32_t> enc;
  uint32_t enc_clamp;  // the index a symbol is clamped to: min(s, enc_clamp)
  // decoder: symof[q] = FreqTable::find_index(q) for q < total (the symbol s with
  // cum[s] <= q < cum[s] + c[s]; a symbol with c = 0 owns no entry), padded to a power of two with
  // its last entry (the kernel masks the index, so the padding names a symbol with c > 0 too)
  std::vector<uint16_t> symof;
  // decoder: cum[0 .. n + 1] with cum[n] = cum[n + 1] = total
  std::vector<uint32_t> row;
};

static inline uint32_t wide16_bitlen(uint32_t v) {
  uint32_t b = 0;
  while (v) ++b, v >>= 1;
  return b;
}

static inline Wide16Tables wide16_build_tables(uint32_t n, const uint32_t* c, const uint32_t* cum,
                                               uint32_t total) {
  Wide16Tables t;
  const bool poison = n < 65536u;
  t.enc_clamp = poison ? n : 65535u;
  t.enc.resize(2 * (size_t)(n + (poison ? 1u : 0u)));
  for (uint32_t s = 0; s < n; ++s) {
    t.enc[2 * (size_t)s] = c[s] ? cum[s] : RC_F_ZERO_FREQ << 24;
    t.enc[2 * (size_t)s + 1] = c[s] ? c[s] : 1u;
  }
  if (poison) {
    t.enc[2 * (size_t)n] = RC_F_BAD_SYMBOL << 24;
    t.enc[2 * (size_t)n + 1] = 1u;
  }
  t.symof.resize((size_t)1 << wide16_bitlen(total - 1));
  for (uint32_t s = 0; s < n; ++s)
    for (uint32_t q = cum[s]; q < cum[s] + c[s]; ++q) t.symof[q] = (uint16_t)s;
  for (size_t q = total; q < t.symof.size(); ++q) t.symof[q] = t.symof[total - 1];
  t.row.resize((size_t)n + 2);
  for (uint32_t s = 0; s < n + 2; ++s) t.row[s] = s < n ? cum[s] : total;
  return t;
}
