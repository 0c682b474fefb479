// The two shapes of print_stats / dump_contigs in the C++ adapter after analyze_kmers, side by side: the device path
// (HashTableInserter::uutigs_stats, HashTableInserter::dump_uutigs: mhmkc_uutigs_stats, mhmkc_uutigs_fasta,
// mhmkc_fasta_write) and the plain host loops over the Contigs vector (ctg_stats, print_stats, dump_contigs of
// include/mhmkc_kcount.hpp, src/contigs.cpp:92-180). The two files must be equal byte for byte, the integer figures
// equal, tot_depth within n 2^-52 sum|d| of the host's sequential sum, and the logged blocks equal line for line.
//   fasta_test <k> <seqqual.txt> <min_ctg_len> <out_dir>   prints "OK <n_ctgs written> <file bytes>" or the mismatches
#include <cmath>
#include <fstream>
#include <iostream>
#include <sstream>

#include "mhmkc_dbjg.hpp"

using namespace mhm2;

static std::string slurp(const std::string &path) {
  std::ifstream in(path, std::ios::binary);
  std::ostringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

template <int MAX_K>
int run(int k, const std::string &path, unsigned min_len, const std::string &dir) {
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
  Contigs none, ctgs;
  std::vector<PackedReads *> list{&pr};
  analyze_kmers<MAX_K>(k, 0, 33, list, 2, none, dht, false);
  traverse_debruijn_graph_device<MAX_K>((unsigned)k, dht, ctgs);
  int bad = 0;
  auto fail = [&](const std::string &what) {
    if (bad++ < 10) std::cout << "MISMATCH " << what << "\n";
  };
  // the file
  const std::string f_dev = dir + "/device.fasta", f_host = dir + "/host.fasta";
  const uint64_t n_all = dht.inserter().dump_uutigs(f_dev, min_len);
  dump_contigs(ctgs, f_host, min_len);
  const std::string t_dev = slurp(f_dev), t_host = slurp(f_host);
  if (t_dev != t_host) fail("files differ: " + std::to_string(t_dev.size()) + " vs " + std::to_string(t_host.size()) + " bytes");
  if (n_all != t_dev.size()) fail("n_bytes_all " + std::to_string(n_all) + " vs the file's " + std::to_string(t_dev.size()));
  // the figures
  mhmkc_ctg_stats mine{};
  const mhmkc_ctg_stats dev = dht.inserter().uutigs_stats(min_len, &mine), host = ctg_stats(ctgs, min_len);
  auto eq = [&](const char *name, uint64_t a, uint64_t b) {
    if (a != b) fail(std::string(name) + ": " + std::to_string(a) + " vs " + std::to_string(b));
  };
  eq("n_ctgs", dev.n_ctgs, host.n_ctgs);
  eq("tot_len", dev.tot_len, host.tot_len);
  eq("max_len", dev.max_len, host.max_len);
  eq("n_ns", dev.n_ns, host.n_ns);
  eq("n50", dev.n50, host.n50);
  eq("l50", dev.l50, host.l50);
  for (int i = 0; i < 5; i++) eq("len_sums", dev.len_sums[i], host.len_sums[i]);
  eq("mine.n_ctgs", mine.n_ctgs, dev.n_ctgs);
  double sum_abs = 0;
  for (const Contig &c : ctgs)
    if (c.seq.size() >= min_len) sum_abs += std::fabs(c.depth);
  // two floating sums of n values in different orders: each within (n - 1) 2^-53 sum|d| of the exact sum
  if (std::fabs(dev.tot_depth - host.tot_depth) > (double)host.n_ctgs * std::ldexp(1.0, -52) * sum_abs)
    fail("tot_depth " + std::to_string(dev.tot_depth) + " vs " + std::to_string(host.tot_depth));
  // the logged block: the integers decide every line but the average depth, which prints six significant digits
  std::ostringstream ps;
  print_stats(ctgs, min_len, ps);
  if (ps.str() != assembly_stats_text(dev, min_len)) fail("print_stats:\n" + ps.str() + "vs\n" + assembly_stats_text(dev, min_len));
  if (ps.str().find("Assembly statistics (contig lengths >= " + std::to_string(min_len) + ")\n    Number of contigs:       ") != 0)
    fail("the block's head:\n" + ps.str());
  if (bad) {
    std::cout << "FAILED " << bad << "\n";
    return 1;
  }
  std::cout << "OK " << dev.n_ctgs << " " << t_dev.size() << "\n" << ps.str();
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const int k = std::atoi(argv[1]);
  const unsigned min_len = (unsigned)std::atoi(argv[3]);
  if (k < 32) return run<32>(k, argv[2], min_len, argv[4]);
  if (k < 64) return run<64>(k, argv[2], min_len, argv[4]);
  if (k < 96) return run<96>(k, argv[2], min_len, argv[4]);
  return run<128>(k, argv[2], min_len, argv[4]);
}
