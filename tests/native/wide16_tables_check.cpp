// Host check of rc_wide16_tables.h (tests/test_wide16_tables.py builds it with
// -fsanitize=address,undefined and runs it): for each table, symof[q] against a brute-force
// FreqTable::find_index for every q < total, the padding up to the power of two, the encoder's
// entries and flags (the poison entry included, and its absence at n = 65536) and the cum row.
// Prints one line per table, or the first mismatch and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <cmath>

#include "../../range_coder_rust_amd/csrc/rc_wide16_tables.h"

#define FAIL(...)          \
  do {                     \
    printf(__VA_ARGS__);   \
    printf("\n");          \
    exit(1);               \
  } while (0)

// find_index as the reference searches (sample_impl.rs:27-45) for rfreq = q
static uint32_t find_index(const std::vector<uint32_t>& cum, uint32_t q) {
  uint32_t left = 0, right = (uint32_t)cum.size() - 1;
  while (left < right) {
    const uint32_t mid = (left + right) / 2;
    if (cum[mid + 1] <= q) left = mid + 1; else right = mid;
  }
  return left;
}
// ... and by its definition: the number of j in [1, n - 1] with cum[j] <= q
static uint32_t find_index_count(const std::vector<uint32_t>& cum, uint32_t q) {
  uint32_t s = 0;
  for (size_t j = 1; j < cum.size(); ++j) s += cum[j] <= q;
  return s;
}

static int n_tables = 0;
static void check(const char* name, const std::vector<uint32_t>& c, bool count_too) {
  const uint32_t n = (uint32_t)c.size();
  std::vector<uint32_t> cum(n);
  uint64_t acc = 0;
  for (uint32_t s = 0; s < n; ++s) cum[s] = (uint32_t)acc, acc += c[s];
  const uint32_t total = (uint32_t)acc;
  if (acc < 256 || acc > 65536) FAIL("%s: total %llu", name, (unsigned long long)acc);
  const Wide16Tables t = wide16_build_tables(n, c.data(), cum.data(), total);
  // q-to-symbol: one entry per q, a power of two of them, the padding names the last real entry
  size_t want = 1;
  while (want < total) want <<= 1;
  if (t.symof.size() != want) FAIL("%s: %zu symof entries, want %zu", name, t.symof.size(), want);
  for (uint32_t q = 0; q < total; ++q) {
    const uint32_t s = find_index(cum, q);
    if (t.symof[q] != s) FAIL("%s: symof[%u] = %u, find_index %u", name, q, t.symof[q], s);
    if (c[s] == 0 || cum[s] > q || q >= cum[s] + c[s]) FAIL("%s: q %u not inside %u", name, q, s);
    if (count_too && find_index_count(cum, q) != s) FAIL("%s: the count at q %u", name, q);
  }
  for (size_t q = total; q < want; ++q)
    if (t.symof[q] != t.symof[total - 1] || c[t.symof[q]] == 0) FAIL("%s: padding at %zu", name, q);
  // encoder entries
  const bool poison = n < 65536;
  if (t.enc.size() != 2 * (size_t)(n + (poison ? 1 : 0))) FAIL("%s: %zu entry words", name, t.enc.size());
  if (t.enc_clamp != (poison ? n : 65535u)) FAIL("%s: clamp %u", name, t.enc_clamp);
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t x = t.enc[2 * (size_t)s], y = t.enc[2 * (size_t)s + 1];
    if (c[s] ? (x != cum[s] || y != c[s] || (x >> 24)) : (x != RC_F_ZERO_FREQ << 24 || y != 1))
      FAIL("%s: entry %u = (%08x, %u)", name, s, x, y);
  }
  if (poison && (t.enc[2 * (size_t)n] != RC_F_BAD_SYMBOL << 24 || t.enc[2 * (size_t)n + 1] != 1))
    FAIL("%s: the poison entry", name);
  // cum row
  if (t.row.size() != (size_t)n + 2) FAIL("%s: row of %zu", name, t.row.size());
  for (uint32_t s = 0; s < n + 2; ++s)
    if (t.row[s] != (s < n ? cum[s] : total)) FAIL("%s: row[%u]", name, s);
  printf("%s: n %u total %u ok\n", name, n, total);
  ++n_tables;
}

int main() {
  {  // all ones at n = total = 65536: no poison entry, no padding
    check("ones", std::vector<uint32_t>(65536, 1), false);
  }
  {  // one symbol holds the whole total
    std::vector<uint32_t> c(1, 65536);
    check("one symbol", c, true);
  }
  {  // three symbols with c > 0 at indices 0, 30000 and 65535, zeros elsewhere
    std::vector<uint32_t> c(65536, 0);
    c[0] = 1000, c[30000] = 64000, c[65535] = 536;
    check("three symbols", c, false);
  }
  {  // symbol n - 1 with c = 0 (and a run of zeros in front of it)
    std::vector<uint32_t> c(5000, 0);
    for (uint32_t s = 0; s < 4000; ++s) c[s] = 1 + (s % 7 == 0 ? 9 : 0) + (s & 1);
    c[4990] = 300;
    check("last symbol empty", c, true);
  }
  {  // total 65535, not a power of two: one entry of padding
    std::vector<uint32_t> c(4097, 15);
    c[4096] = 65535 - 4096 * 15;
    check("total 65535", c, true);
  }
  {  // a seeded Zipf table over 20,000 symbols: zeros in its tail, a shuffled order
    const uint32_t n = 20000, total = 40000;
    std::vector<double> w(n);
    double sum = 0;
    for (uint32_t s = 0; s < n; ++s) sum += w[s] = 1.0 / std::pow(s + 1.0, 1.2);
    std::vector<uint32_t> c(n);
    uint64_t acc = 0;
    for (uint32_t s = 0; s < n; ++s) acc += c[s] = (uint32_t)(w[s] / sum * total);
    c[0] += total - (uint32_t)acc;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint32_t s = n - 1; s > 0; --s) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      const uint32_t j = (uint32_t)(x % (s + 1));
      const uint32_t tmp = c[s];
      c[s] = c[j], c[j] = tmp;
    }
    check("zipf 20000", c, false);
  }
  printf("%d tables ok\n", n_tables);
  return 0;
}
