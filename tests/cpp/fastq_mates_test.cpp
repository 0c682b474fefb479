// A read library named as main.cpp names it (src/main.cpp:142-148: "r1.fq:r2.fq", "reads.fq:" or "interleaved.fq")
// through the C++ adapter: KmerDHT::add_reads_fname, then finish_updates, then a digest of the local KmerMap that the
// test compares with the Python adapter's table.
//   fastq_mates_test <k> <reads_fname>   prints "OK <rows> <sum of counts> <digest> <pairs> <rounds>"
#include <iostream>

#include "mhmkc_kcount.hpp"

using namespace mhm2;

// one row's 64-bit mix (tests/test_fastq_mates_cpp.py restates it); the digest is the sum over the rows
static uint64_t row_mix(const uint64_t *longs, int n_longs, uint16_t count, char left, char right) {
  uint64_t h = 0;
  for (int i = 0; i < n_longs; i++) {
    h = (h ^ longs[i]) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  h = (h ^ ((uint64_t)count | (uint64_t)(uint8_t)left << 16 | (uint64_t)(uint8_t)right << 24)) * 0xD6E8FEB86659FD93ull;
  return h ^ (h >> 32);
}

template <int MAX_K>
int run(int k, const std::string &reads_fname) {
  Kmer<MAX_K>::set_k(k);
  KmerDHT<MAX_K> dht(1000, 1 << 20, 100, false, true);
  dht.add_reads_fname(reads_fname);
  const mhmkc_fastq_mates_info_t mi = dht.inserter().fastq_mates_info();
  dht.finish_updates();
  uint64_t rows = 0, counts = 0, digest = 0;
  for (auto it = dht.local_kmers_begin(); it != dht.local_kmers_end(); ++it) {
    rows++;
    counts += it->second.count;
    digest += row_mix(it->first.get_longs(), Kmer<MAX_K>::N_LONGS, it->second.count, it->second.left, it->second.right);
  }
  std::cout << "OK " << rows << " " << counts << " " << digest << " " << mi.pairs << " " << mi.rounds << "\n";
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const int k = std::atoi(argv[1]);
  if (k < 32) return run<32>(k, argv[2]);
  if (k < 64) return run<64>(k, argv[2]);
  if (k < 96) return run<96>(k, argv[2]);
  return run<128>(k, argv[2]);
}
