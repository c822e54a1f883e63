// A wide alphabet through the C++ host API: examples/sample_impl.rs with a FreqTable of 1000
// symbols instead of 10 -- the reference's FreqTable::new(alphabet_count) takes any size and its
// PModel is indexed with usize.  The data are counted into the table, coded as 16-bit symbols in
// one batch launch of a wide static model (rc::WideModel), checked against the per-call
// rc::Encoder given the same table, then decoded back.
// Built by __graft_entry__.build(); run by tests/test_gpu_wide.py::test_cpp_wide_impl.
#include <cstdio>
#include <vector>

#include "range_coder.hpp"

int main() {
  // 3000 symbols over 1000 indexes, skewed towards the low ones (the product of two draws)
  const size_t alphabet = 1000, count = 3000;
  std::vector<uint16_t> test_data(count);
  uint64_t x = 0x2545F4914F6CDD1Dull;
  for (size_t i = 0; i < count; ++i) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t a = (x >> 33) % alphabet, b = (x >> 13) % alphabet;
    test_data[i] = (uint16_t)(a * b / alphabet);
  }
  test_data[7] = (uint16_t)(alphabet - 1);  // the last index is in use
  rc::FreqTable table(alphabet);
  for (uint16_t s : test_data) table.add_alphabet_freq(s);
  table.calc_cum();
  std::printf("FREQ TABLE: %zu symbols, total %u\n", table.alphabet_count(), table.total_freq());

  // the reference's way: one call per symbol
  rc::Encoder encoder;
  for (uint16_t s : test_data) encoder.encode(table, s);
  const std::vector<uint8_t> want = encoder.finish();

  // the batch way: one chunk of 16-bit symbols
  rc::WideModel wide(rc::Context::default_context(), table);
  const std::vector<uint8_t> code = wide.encode_chunks({test_data}).at(0);
  std::printf("output : 0x");
  for (size_t i = 0; i < 16 && i < code.size(); ++i) std::printf("%02x", code[i]);
  std::printf("...\nlength : %zubyte\n", code.size());
  if (code != want) {
    std::printf("batch and per-call bytes differ: FAILED\n");
    return 1;
  }
  const std::vector<uint16_t> back = wide.decode_chunks({code}, {count}).at(0);
  if (back != test_data) {
    std::printf("round trip FAILED\n");
    return 1;
  }
  std::printf("test passed\n");
  return 0;
}
