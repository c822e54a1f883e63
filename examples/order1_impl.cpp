// Order-1 context coding through the C++ host API: a short text coded with K FreqTables chosen by
// the class of the previous byte -- what the reference writes as
// encoder.encode(&models[class(data[i-1])], data[i]) -- in one batch launch of an order-1 set
// (rc::Order1Set), checked against the per-call rc::Encoder given the same tables, then decoded
// back with no side information: the decoder finds each table from the symbol it decoded last.
// The tables of a set share one total_freq in 256..65536: each starts with one count per symbol
// (every byte stays encodable in every class) and the text is counted until the total is 4096.
// Built by __graft_entry__.build(); run by tests/test_gpu_order1.py::test_cpp_order1_impl.
#include <cstdio>
#include <string>
#include <vector>

#include "range_coder.hpp"

// the class of a previous byte: space or punctuation, vowel, other letter, anything else
static uint8_t byte_class(uint8_t b) {
  if (b == ' ' || b == ',' || b == '.' || b == '\n') return 0;
  const uint8_t l = (uint8_t)(b | 0x20);
  if (l == 'a' || l == 'e' || l == 'i' || l == 'o' || l == 'u') return 1;
  if (l >= 'a' && l <= 'z') return 2;
  return 3;
}

int main() {
  const std::string text =
      "the quick brown fox jumps over the lazy dog, and the lazy dog, in no hurry at all, "
      "watches the quick brown fox jump over it again and again.\n";
  const std::vector<uint8_t> data(text.begin(), text.end());
  constexpr uint32_t K = 4, N = 128, TOTAL = 4096, FIRST = 0;
  std::vector<uint8_t> ctx_map(N);
  for (uint32_t s = 0; s < N; ++s) ctx_map[s] = byte_class((uint8_t)s);

  // K tables by previous-byte class: one count per symbol, then the text's pairs, round after
  // round, until each table holds TOTAL counts
  std::vector<rc::FreqTable> tables(K, rc::FreqTable(N));
  std::vector<uint32_t> filled(K, N);
  for (uint32_t j = 0; j < K; ++j)
    for (uint32_t s = 0; s < N; ++s) tables[j].add_alphabet_freq(s);
  for (bool grew = true; grew;) {
    grew = false;
    for (size_t i = 0; i < data.size(); ++i) {
      const uint32_t j = i ? ctx_map[data[i - 1]] : FIRST;
      if (filled[j] < TOTAL) {
        tables[j].add_alphabet_freq(data[i]);
        ++filled[j];
        grew = true;
      }
    }
  }
  for (uint32_t j = 0; j < K; ++j) {
    for (uint32_t s = 0; filled[j] < TOTAL; s = (s + 1) % N, ++filled[j])
      tables[j].add_alphabet_freq(s);  // (a class the text never enters: top it up evenly)
    tables[j].calc_cum();
  }
  std::vector<const rc::PModel*> models;
  for (const rc::FreqTable& t : tables) models.push_back(&t);
  std::printf("%u tables of %u symbols, total %u, %zu bytes of text\n", K, N,
              tables[0].total_freq(), data.size());

  // the reference's way: the model is an argument of every call
  rc::Encoder encoder;
  for (size_t i = 0; i < data.size(); ++i)
    encoder.encode(*models[i ? ctx_map[data[i - 1]] : FIRST], data[i]);
  const std::vector<uint8_t> want = encoder.finish();

  // the batch way: one chunk, no index stream
  rc::Order1Set set(rc::Context::default_context(), models, ctx_map, FIRST);
  const std::vector<uint8_t> code = set.encode_chunks({data}).at(0);
  std::printf("output : 0x");
  for (uint8_t b : code) std::printf("%02x", b);
  std::printf("\nlength : %zubyte\n", code.size());
  if (code != want) {
    std::printf("batch and per-call bytes differ: FAILED\n");
    return 1;
  }

  const std::vector<uint8_t> back = set.decode_chunks({code}, {data.size()}).at(0);
  if (back != data) {
    std::printf("round trip FAILED\n");
    return 1;
  }
  rc::Decoder decoder(code);  // and the per-call decoder reads the same stream
  uint32_t row = FIRST;
  for (size_t i = 0; i < data.size(); ++i) {
    const size_t s = decoder.decode(*models[row]);
    if (s != data[i]) {
      std::printf("per-call decode FAILED\n");
      return 1;
    }
    row = ctx_map[s];
  }
  std::printf("test passed\n");
  return 0;
}
