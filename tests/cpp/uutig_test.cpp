// The two traversals of the C++ adapter after analyze_kmers, side by side: traverse_debruijn_graph over the host KmerMap
// and traverse_debruijn_graph_device (mhmkc_uutigs on the GPU, include/mhmkc_dbjg.hpp). Contig for contig: id, sequence
// (for even k either strand) and depth must be equal.
//   uutig_test <k> <seqqual.txt>      prints "OK <n_ctgs> <n_bases>" or the first mismatches; exit status 1 on any
#include <fstream>
#include <iostream>
#include <sstream>

#include "mhmkc_dbjg.hpp"

using namespace mhm2;

static std::string revcomp(const std::string &s) {
  std::string r(s.rbegin(), s.rend());
  for (char &c : r) c = dbjg_comp(c);
  return r;
}

template <int MAX_K>
int run(int k, const std::string &path) {
  using K = Kmer<MAX_K>;
  K::set_k(k);
  std::ifstream in(path);
  std::string line;
  PackedReads pr(33);
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string s, q;
    ss >> s >> q;
    pr.add_read("@r/1", s, q);
  }
  KmerDHT<MAX_K> dht(1000, 1 << 20, 100, false, true);
  Contigs ctgs;
  std::vector<PackedReads *> list{&pr};
  analyze_kmers<MAX_K>(k, 0, 33, list, 2, ctgs, dht, false);
  Contigs host, dev;
  traverse_debruijn_graph<MAX_K>((unsigned)k, dht, host);
  traverse_debruijn_graph_device<MAX_K>((unsigned)k, dht, dev);
  int bad = 0;
  auto fail = [&](const std::string &what) {
    if (bad++ < 10) std::cout << "MISMATCH " << what << "\n";
  };
  if (host.size() != dev.size()) fail("contigs: " + std::to_string(host.size()) + " vs " + std::to_string(dev.size()));
  uint64_t n_bases = 0;
  for (size_t c = 0; c < host.size() && c < dev.size(); c++) {
    const bool same = dev[c].seq == host[c].seq || (k % 2 == 0 && dev[c].seq == revcomp(host[c].seq));
    if (dev[c].id != host[c].id || !same || dev[c].depth != host[c].depth)
      fail("contig " + std::to_string(c) + ": id " + std::to_string(dev[c].id) + " depth " + std::to_string(dev[c].depth) +
           " vs " + std::to_string(host[c].depth) + " length " + std::to_string(dev[c].seq.size()) + " vs " +
           std::to_string(host[c].seq.size()));
    n_bases += dev[c].seq.size();
  }
  if (bad) {
    std::cout << "FAILED " << bad << "\n";
    return 1;
  }
  std::cout << "OK " << dev.size() << " " << n_bases << "\n";
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
