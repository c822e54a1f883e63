// Host check of rc_wide16_fine_tables.h (tests/test_wide16_fine_tables.py builds it with
// -fsanitize=address,undefined and runs it): for each table and both bucket counts (2^15, 2^16),
// the way the kernel goes -- bucket, rank search, occupied symbol -- against a brute-force
// FreqTable::find_index at every bucket boundary and at rcum[j] - 1, rcum[j] and rcum[j] + c - 1
// of every rank (at every q < total when total <= 2^18); the ranks per bucket, the padding and the
// sentinel; the encoder's entries and the poison entry (and its absence at n = 65536).
// Prints one line per table, or the first mismatch and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include "../../range_coder_rust_amd/csrc/rc_wide16_fine_tables.h"

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
static void check_bits(const char* name, const std::vector<uint32_t>& c,
                       const std::vector<uint32_t>& cum, uint32_t total, uint32_t bits) {
  const uint32_t n = (uint32_t)c.size();
  const Wide16FineTables t = wide16_fine_build_tables(n, c.data(), cum.data(), total, bits);
  // ranks: the occupied symbols in order, their cum, the total twice
  uint32_t m = 0;
  for (uint32_t s = 0; s < n; ++s) {
    if (!c[s]) continue;
    if (m >= t.m || t.occ[m] != s || t.rcum[m] != cum[s]) FAIL("%s: rank %u", name, m);
    ++m;
  }
  if (m != t.m || t.occ.size() != (size_t)(m + (m & 1)) || t.rcum.size() != (size_t)m + 2 ||
      t.rcum[m] != total || t.rcum[m + 1] != total || t.rcum[0] != 0)
    FAIL("%s: %u ranks, tables of %zu and %zu", name, m, t.occ.size(), t.rcum.size());
  // buckets
  uint32_t bl = 0;
  while ((total - 1) >> bl) ++bl;
  if (t.bits != bits || t.shift != bl - bits) FAIL("%s: bits %u shift %u", name, t.bits, t.shift);
  const uint32_t nb = 1u << bits, last = (total - 1) >> t.shift;
  if (t.bucket.size() != (size_t)nb + 2) FAIL("%s: %zu buckets", name, t.bucket.size());
  if (last >= nb || last < nb / 2) FAIL("%s: last bucket %u of %u", name, last, nb);
  uint32_t widest = 0;
  for (uint32_t b = 0; b <= last; ++b) {
    const uint32_t j = t.bucket[b], q = b << t.shift;
    if (j >= m || t.rcum[j] > q || q >= t.rcum[j + 1]) FAIL("%s: bucket %u names rank %u", name, b, j);
    const uint32_t j1 = t.bucket[b + 1];
    if (j1 < j || j1 >= m) FAIL("%s: bucket %u's neighbour", name, b);
    if (j1 - j + 1 > widest) widest = j1 - j + 1;
    // the last q of the bucket lies at a rank of [j, j1]
    const uint64_t qe = (uint64_t)(b + 1) << t.shift;
    const uint32_t ql = qe < total ? (uint32_t)qe - 1 : total - 1;
    if (t.rcum[j1 + 1] <= ql) FAIL("%s: bucket %u ends past rank %u", name, b, j1);
  }
  if (widest > (1u << t.shift) + 1) FAIL("%s: %u ranks in a bucket, shift %u", name, widest, t.shift);
  for (size_t b = (size_t)last + 1; b < t.bucket.size(); ++b)  // the padding and the sentinel
    if (t.bucket[b] != m - 1) FAIL("%s: padding at %zu", name, b);
  // q -> symbol as the kernel goes
  uint32_t max_steps = 0;
  auto one = [&](uint32_t q, bool count_too) {
    uint32_t rank = 0, steps = 0;
    const uint32_t s = wide16_fine_lookup(t, q, &rank, &steps);
    const uint32_t want = find_index(cum, q);
    if (s != want) FAIL("%s: q %u gives %u, find_index %u", name, q, s, want);
    if (c[s] == 0 || cum[s] > q || q >= cum[s] + c[s]) FAIL("%s: q %u not inside %u", name, q, s);
    if (count_too && find_index_count(cum, q) != s) FAIL("%s: the count at q %u", name, q);
    if (steps > t.shift + 1) FAIL("%s: %u search steps at q %u, shift %u", name, steps, q, t.shift);
    if (steps > max_steps) max_steps = steps;
  };
  if (total <= (1u << 18)) {
    for (uint32_t q = 0; q < total; ++q) one(q, n <= 4096 && (q & 63) == 0);
  } else {
    for (uint32_t b = 0; b <= last; ++b) {
      one(b << t.shift, false);
      if (b) one((b << t.shift) - 1, false);
    }
    for (uint32_t j = 0; j < m; ++j) {
      if (t.rcum[j]) one(t.rcum[j] - 1, false);
      one(t.rcum[j], false);
      one(t.rcum[j + 1] - 1, false);
    }
    one(total - 1, false);
  }
  // encoder entries
  const bool poison = n < 65536;
  if (t.enc.size() != 2 * (size_t)(n + (poison ? 1 : 0))) FAIL("%s: %zu entry words", name, t.enc.size());
  if (t.enc_clamp != (poison ? n : 65535u)) FAIL("%s: clamp %u", name, t.enc_clamp);
  for (uint32_t s = 0; s < n; ++s)
    if (t.enc[2 * (size_t)s] != cum[s] || t.enc[2 * (size_t)s + 1] != c[s])
      FAIL("%s: entry %u", name, s);
  if (poison && (t.enc[2 * (size_t)n] != 0xFFFFFFFFu || t.enc[2 * (size_t)n + 1] != 0))
    FAIL("%s: the poison entry", name);
  printf("%s: n %u total %u ranks %u bits %u shift %u widest bucket %u, %u steps ok\n", name, n,
         total, m, bits, t.shift, widest, max_steps);
}

static void check(const char* name, const std::vector<uint32_t>& c) {
  std::vector<uint32_t> cum(c.size());
  uint64_t acc = 0;
  for (size_t s = 0; s < c.size(); ++s) cum[s] = (uint32_t)acc, acc += c[s];
  if (acc <= 65536 || acc > (1u << 24)) FAIL("%s: total %llu", name, (unsigned long long)acc);
  check_bits(name, c, cum, (uint32_t)acc, 15);
  check_bits(name, c, cum, (uint32_t)acc, 16);
  ++n_tables;
}

int main() {
  {  // dense: every symbol of the 16-bit alphabet at c = 1 and one heavy symbol, total 2^24
    std::vector<uint32_t> c(65536, 1);
    c[12345] = (1u << 24) - 65535;
    check("dense 2^24", c);
  }
  {  // the same alphabet at the smallest total: one symbol with c = 2
    std::vector<uint32_t> c(65536, 1);
    c[65535] = 2;
    check("dense 65537", c);
  }
  {  // 2,048 occupied symbols of c in 1..3 with a zero-frequency symbol between each pair, and
     // one heavy symbol far behind them, total 2^20
    std::vector<uint32_t> c(65536, 0);
    uint64_t acc = 0;
    for (uint32_t j = 0; j < 2048; ++j) acc += c[2 * j + 100] = 1 + j % 3;
    c[50000] = (1u << 20) - (uint32_t)acc;
    check("sparse 2^20", c);
  }
  {  // two occupied symbols 60,000 apart, total 2^24
    std::vector<uint32_t> c(65536, 0);
    c[3000] = 1;
    c[63000] = (1u << 24) - 1;
    check("two symbols 2^24", c);
  }
  {  // two occupied symbols 60,000 apart, the light one last, total 2^18 (every q checked)
    std::vector<uint32_t> c(63001, 0);
    c[3000] = (1u << 18) - 5;
    c[63000] = 5;
    check("two symbols 2^18", c);
  }
  {  // one symbol holds the whole total
    check("one symbol", std::vector<uint32_t>(1, 65537));
  }
  {  // total 2^24 - 3 over 65,535 symbols: a poison entry, a last bucket that is not full
    std::vector<uint32_t> c(65535, 200);
    for (uint32_t s = 0; s < 65535; s += 3) c[s] = 0;
    uint64_t acc = 0;
    for (uint32_t x : c) acc += x;
    c[65534] += (1u << 24) - 3 - (uint32_t)acc;
    check("total 2^24 - 3", c);
  }
  {  // a small alphabet at a total that is no power of two, every q checked, the count too
    std::vector<uint32_t> c(300, 0);
    uint64_t acc = 0;
    for (uint32_t s = 0; s < 299; ++s) acc += c[s] = (s % 5 == 0) ? 0 : 1 + (s * 37) % 600;
    c[299] = 100003 - (uint32_t)acc;
    check("300 symbols 100003", c);
  }
  printf("%d tables ok\n", n_tables);
  return 0;
}
