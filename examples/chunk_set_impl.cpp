// A model chosen per chunk, through the C++ host API: the reference's sample data
// (examples/sample_impl.rs:74) in four chunks, coded in one batch launch of a static chunk set
// (rc::ChunkSet) of two FreqTables -- chunks 0 and 2 with table 0, chunks 1 and 3 with table 1 --
// and checked against the per-call rc::Encoder given each chunk's table, then decoded back.  The
// tables of a set share one total_freq in 256..65536, so each symbol is counted 32 times: table 0
// counts the data, table 1 its mirror image 9 - s.  rc::cost_table prices both tables.
// Built by __graft_entry__.build(); run by tests/test_gpu_chunk_set.py::test_cpp_chunk_set_impl.
#include <cstdio>
#include <vector>

#include "range_coder.hpp"

int main() {
  const std::vector<size_t> test_data = {2, 1, 1, 4, 1, 4, 2, 1, 0, 1, 5, 9, 8, 7, 6, 5};
  rc::FreqTable t0(10), t1(10);
  for (size_t s : test_data)
    for (int r = 0; r < 32; ++r) {
      t0.add_alphabet_freq(s);
      t1.add_alphabet_freq(9 - s);
    }
  t0.calc_cum();
  t1.calc_cum();
  const rc::PModel* models[2] = {&t0, &t1};
  std::printf("FREQ TABLES (total %u)\n", t0.total_freq());

  // a symbol that fills half the table costs one bit, one the table lacks has no cost
  std::vector<uint32_t> c0;
  for (size_t i = 0; i < t0.alphabet_count(); ++i) c0.push_back(t0.c_freq(i));
  const std::vector<uint32_t> cost = rc::cost_table(c0, t0.total_freq());
  for (size_t i = 0; i < cost.size(); ++i) {
    const bool none = cost[i] == RC_COST_NONE;
    if (none != (c0[i] == 0) || (c0[i] == t0.total_freq() / 2 && cost[i] != 65536u)) {
      std::printf("cost table FAILED at %zu\n", i);
      return 1;
    }
  }

  // four chunks: the data, its mirror, the data reversed, and an empty one
  std::vector<std::vector<uint8_t>> chunks(4);
  for (size_t s : test_data) {
    chunks[0].push_back((uint8_t)s);
    chunks[1].push_back((uint8_t)(9 - s));
  }
  chunks[2].assign(chunks[0].rbegin(), chunks[0].rend());
  const std::vector<uint8_t> class_of = {0, 1, 0, 1};

  rc::ChunkSet set(rc::Context::default_context(), {&t0, &t1});
  const std::vector<std::vector<uint8_t>> codes = set.encode_chunks(chunks, class_of);
  std::vector<uint64_t> counts;
  for (size_t k = 0; k < chunks.size(); ++k) {
    // the reference's way: the chunk's model is an argument of every call
    rc::Encoder encoder;
    for (uint8_t s : chunks[k]) encoder.encode(*models[class_of[k]], s);
    if (codes.at(k) != encoder.finish()) {
      std::printf("chunk %zu: batch and per-call bytes differ: FAILED\n", k);
      return 1;
    }
    std::printf("chunk %zu (table %u): %zu byte\n", k, (unsigned)class_of[k], codes[k].size());
    counts.push_back(chunks[k].size());
  }
  if (set.decode_chunks(codes, counts, class_of) != chunks) {
    std::printf("round trip FAILED\n");
    return 1;
  }
  std::printf("test passed\n");
  return 0;
}
