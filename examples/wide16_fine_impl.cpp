// A dense 16-bit alphabet through the C++ host API: int16-like samples around zero, a skewed
// table over all 65536 symbols with every symbol encodable and a total of 2^20, coded in one batch
// launch of a wide16 fine model (rc::Wide16FineModel), checked against the per-call rc::Encoder
// given the same table, then decoded back.  At a total of 2^16 the same alphabet leaves every
// symbol a frequency of one: that table is all ones and its code is 2 bytes per symbol, which is
// printed beside the fine model's size.
// Built by __graft_entry__.build(); run by tests/test_gpu_wide16_fine.py::test_cpp_wide16_fine_impl.
#include <cstdio>
#include <vector>

#include "range_coder.hpp"

// a fixed table as a PModel (the reference's trait: c_freq, cum_freq, total_freq)
struct Table : rc::PModel {
  std::vector<uint32_t> c, cum;
  uint32_t total = 0;
  uint32_t c_freq(size_t i) const override { return c[i]; }
  uint32_t cum_freq(size_t i) const override { return cum[i]; }
  uint32_t total_freq() const override { return total; }
  size_t alphabet_count() const override { return c.size(); }
};

int main() {
  // 4 chunks of 3000 two's-complement samples: sums of uniform draws, both signs, so the largest
  // symbol is 65535 and the alphabet is all of 2^16
  const size_t alphabet = 65536, chunks = 4, count = 3000;
  const uint32_t total = 1u << 20;
  std::vector<std::vector<uint16_t>> data(chunks, std::vector<uint16_t>(count));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  for (auto& ch : data)
    for (auto& s : ch) {
      int v = 0;
      for (int j = 0; j < 4; ++j) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v += (int)((x >> 40) & 0x3FF) - 512;
      }
      s = (uint16_t)(int16_t)v;
    }
  // every symbol gets 1, the rest of the total goes to the symbols that occur, by their counts
  std::vector<uint64_t> cnt(alphabet, 0);
  for (const auto& ch : data)
    for (uint16_t s : ch) cnt[s] += 1;
  Table table;
  table.c.assign(alphabet, 1);
  const uint64_t spare = total - alphabet, n_all = chunks * count;
  uint64_t given = 0;
  size_t top = 0;
  for (size_t s = 0; s < alphabet; ++s) {
    const uint64_t add = cnt[s] * spare / n_all;
    table.c[s] += (uint32_t)add;
    given += add;
    if (cnt[s] > cnt[top]) top = s;
  }
  table.c[top] += (uint32_t)(spare - given);
  table.cum.resize(alphabet);
  for (size_t s = 0; s < alphabet; ++s) {
    table.cum[s] = table.total;
    table.total += table.c[s];
  }
  std::printf("FREQ TABLE: %zu symbols, total %u\n", table.alphabet_count(), table.total_freq());

  // the reference's way: one call per symbol (chunk 0)
  rc::Encoder encoder;
  for (uint16_t s : data[0]) encoder.encode(table, s);
  const std::vector<uint8_t> want = encoder.finish();

  // the batch way: one launch over the chunks
  rc::Wide16FineModel fine(rc::Context::default_context(), table);
  const std::vector<std::vector<uint8_t>> codes = fine.encode_chunks(data);
  size_t bytes = 0;
  for (const auto& c : codes) bytes += c.size();
  std::printf("length : %zubyte for %zu symbols at total 2^20\n", bytes, chunks * count);
  std::printf("all ones at total 2^16: %zubyte (2 bytes per symbol and the flush)\n",
              chunks * (2 * count + 8));
  if (codes.at(0) != want) {
    std::printf("batch and per-call bytes differ: FAILED\n");
    return 1;
  }
  const auto back = fine.decode_chunks(codes, std::vector<uint64_t>(chunks, count));
  if (back != data) {
    std::printf("round trip FAILED\n");
    return 1;
  }
  std::printf("round trip ok\ntest passed\n");
  return 0;
}
