// A model chosen per symbol, through the C++ host API: the reference's sample data
// (examples/sample_impl.rs:74) coded with two FreqTables that alternate per symbol -- what the
// reference writes as encoder.encode(&models[i % 2], data[i]) -- in one batch launch of a static
// model set (rc::ModelSet), checked against the per-call rc::Encoder given the same two tables,
// then decoded back.  The tables of a set share one total_freq in 256..65536, so each symbol is
// counted 32 times: table 0 counts the symbols at even positions, table 1 those at odd ones.
// Built by __graft_entry__.build(); run by tests/test_gpu_indexed.py::test_cpp_model_set_impl.
#include <cstdio>
#include <vector>

#include "range_coder.hpp"

int main() {
  const std::vector<size_t> test_data = {2, 1, 1, 4, 1, 4, 2, 1, 0, 1, 5, 9, 8, 7, 6, 5};
  rc::FreqTable t0(10), t1(10);
  for (size_t i = 0; i < test_data.size(); ++i)
    for (int r = 0; r < 32; ++r) (i % 2 ? t1 : t0).add_alphabet_freq(test_data[i]);
  t0.calc_cum();
  t1.calc_cum();
  const rc::PModel* models[2] = {&t0, &t1};
  std::printf("FREQ TABLES (total %u)\n", t0.total_freq());
  for (size_t i = 0; i < t0.alphabet_count(); ++i)
    std::printf("index:%zu, c:%u/%u, cum:%u/%u\n", i, t0.c_freq(i), t1.c_freq(i), t0.cum_freq(i),
                t1.cum_freq(i));

  // the reference's way: the model is an argument of every call
  rc::Encoder encoder;
  for (size_t i = 0; i < test_data.size(); ++i) encoder.encode(*models[i % 2], test_data[i]);
  const std::vector<uint8_t> want = encoder.finish();

  // the batch way: one chunk, one model index per symbol
  rc::ModelSet set(rc::Context::default_context(), {&t0, &t1});
  rc::ModelSet::Chunk chunk;
  for (size_t i = 0; i < test_data.size(); ++i) {
    chunk.data.push_back((uint8_t)test_data[i]);
    chunk.idx.push_back((uint8_t)(i % 2));
  }
  const std::vector<uint8_t> code = set.encode_chunks({chunk}).at(0);
  std::printf("output : 0x");
  for (uint8_t b : code) std::printf("%02x", b);
  std::printf("\nlength : %zubyte\n", code.size());
  if (code != want) {
    std::printf("batch and per-call bytes differ: FAILED\n");
    return 1;
  }

  rc::ModelSet::Chunk stream;
  stream.data = code;
  stream.idx = chunk.idx;  // side information: the decoder knows each symbol's model
  const std::vector<uint8_t> back = set.decode_chunks({stream}).at(0);
  if (back != chunk.data) {
    std::printf("round trip FAILED\n");
    return 1;
  }
  rc::Decoder decoder(code);  // and the per-call decoder reads the same stream
  for (size_t i = 0; i < test_data.size(); ++i)
    if (decoder.decode(*models[i % 2]) != test_data[i]) {
      std::printf("per-call decode FAILED\n");
      return 1;
    }
  std::printf("test passed\n");
  return 0;
}
