// The full 16-bit alphabet through the C++ host API: a FreqTable over all 65536 symbols, as the
// reference's FreqTable::new(alphabet_count) allows, counted from bf16-like data (the high bits
// of a few thousand float values), coded as 16-bit symbols in one batch launch of a wide16 static
// model (rc::Wide16Model, tables in device memory), checked against the per-call rc::Encoder given
// the same table, then decoded back.
// Built by __graft_entry__.build(); run by tests/test_gpu_wide16.py::test_cpp_wide16_impl.
#include <cstdio>
#include <cstring>
#include <vector>

#include "range_coder.hpp"

int main() {
  // 4 chunks of 3000 bf16 bit patterns: sums of uniform draws around zero, both signs
  const size_t alphabet = 65536, chunks = 4, count = 3000;
  std::vector<std::vector<uint16_t>> data(chunks, std::vector<uint16_t>(count));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  for (auto& ch : data)
    for (auto& s : ch) {
      float v = 0.f;
      for (int j = 0; j < 4; ++j) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v += (float)((x >> 40) & 0xFFFF) / 65536.f - 0.5f;
      }
      uint32_t bits;
      std::memcpy(&bits, &v, 4);
      s = (uint16_t)(bits >> 16);
    }
  data[0][7] = 65535;  // the last index is in use
  data[1][9] = 0;
  rc::FreqTable table(alphabet);
  for (const auto& ch : data)
    for (uint16_t s : ch) table.add_alphabet_freq(s);
  table.calc_cum();
  std::printf("FREQ TABLE: %zu symbols, total %u\n", table.alphabet_count(), table.total_freq());

  // the reference's way: one call per symbol (chunk 0)
  rc::Encoder encoder;
  for (uint16_t s : data[0]) encoder.encode(table, s);
  const std::vector<uint8_t> want = encoder.finish();

  // the batch way: one launch over the chunks
  rc::Wide16Model wide16(rc::Context::default_context(), table);
  const std::vector<std::vector<uint8_t>> codes = wide16.encode_chunks(data);
  size_t bytes = 0;
  for (const auto& c : codes) bytes += c.size();
  std::printf("length : %zubyte for %zu symbols\n", bytes, chunks * count);
  if (codes.at(0) != want) {
    std::printf("batch and per-call bytes differ: FAILED\n");
    return 1;
  }
  const auto back = wide16.decode_chunks(codes, std::vector<uint64_t>(chunks, count));
  if (back != data) {
    std::printf("round trip FAILED\n");
    return 1;
  }
  std::printf("round trip ok\ntest passed\n");
  return 0;
}
