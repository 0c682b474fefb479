// Multi-k contigging at one rank with the contigs kept on the device between the rounds (src/contigging.cpp:93-158): the
// analyze_kmers overload that takes the previous round's KmerDHT (mhmkc_add_ctgs_from) against the existing route,
// traverse_debruijn_graph_device -> Contigs -> analyze_kmers(ctgs), round by round. Both routes start from the same
// first-k table; from then on each continues from its own previous round. Row for row the tables must be equal.
//   ctg_chain_test <seqqual.txt> <k1,k2,...>   prints "ROUND <k> <rows> <ctg_kmers>" per round after the first and "OK",
//                                              or the first mismatches; exit status 1 on any
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

#include "mhmkc_dbjg.hpp"

using namespace mhm2;

struct Chain {
  PackedReads *pr;
  std::vector<int> ks;
};

template <int MAX_K>
int compare(int k, KmerDHT<MAX_K> &a, KmerDHT<MAX_K> &b) {
  int bad = 0;
  if (a.get_local_num_kmers() != b.get_local_num_kmers()) {
    std::cout << "MISMATCH k " << k << ": " << a.get_local_num_kmers() << " vs " << b.get_local_num_kmers() << " rows\n";
    bad++;
  }
  for (auto it = a.local_kmers_begin(); it != a.local_kmers_end(); ++it) {
    KmerCounts *kc = b.get_local_kmer_counts(it->first);
    if (!kc || kc->count != it->second.count || kc->left != it->second.left || kc->right != it->second.right) {
      if (bad++ < 10)
        std::cout << "MISMATCH k " << k << ": " << it->first.to_string() << " " << it->second.count << " "
                  << it->second.left << " " << it->second.right << " vs "
                  << (kc ? std::to_string(kc->count) + " " + kc->left + " " + kc->right : std::string("absent")) << "\n";
    }
  }
  return bad;
}

template <int MAX_K, int PREV_MAX_K>
int round_k(const Chain &ch, size_t i, KmerDHT<PREV_MAX_K> &prev_a, KmerDHT<PREV_MAX_K> &prev_b);

// round i of the chain at the smallest MAX_K that holds its k (never below the previous round's)
template <int PREV_MAX_K>
int next_round(const Chain &ch, size_t i, KmerDHT<PREV_MAX_K> &prev_a, KmerDHT<PREV_MAX_K> &prev_b) {
  if (i >= ch.ks.size()) return 0;
  const int k = ch.ks[i];
  if (k <= ch.ks[i - 1]) die("the chain's k must grow from round to round");
  if constexpr (PREV_MAX_K <= 32)
    if (k < 32) return round_k<32, PREV_MAX_K>(ch, i, prev_a, prev_b);
  if constexpr (PREV_MAX_K <= 64)
    if (k < 64) return round_k<64, PREV_MAX_K>(ch, i, prev_a, prev_b);
  if constexpr (PREV_MAX_K <= 96)
    if (k < 96) return round_k<96, PREV_MAX_K>(ch, i, prev_a, prev_b);
  return round_k<128, PREV_MAX_K>(ch, i, prev_a, prev_b);
}

template <int MAX_K, int PREV_MAX_K>
int round_k(const Chain &ch, size_t i, KmerDHT<PREV_MAX_K> &prev_a, KmerDHT<PREV_MAX_K> &prev_b) {
  const int k = ch.ks[i], prev_k = ch.ks[i - 1];
  Contigs ctgs;  // the existing route: the previous round's uutigs through the host
  traverse_debruijn_graph_device<PREV_MAX_K>((unsigned)prev_k, prev_a, ctgs);
  Kmer<MAX_K>::set_k(k);
  std::vector<PackedReads *> list{ch.pr};
  KmerDHT<MAX_K> a(1000, 1 << 20, 100, false, true), b(1000, 1 << 20, 100, false, true);
  analyze_kmers<MAX_K>(k, prev_k, 33, list, 2, ctgs, a, false);
  analyze_kmers<MAX_K>(k, prev_k, 33, list, 2, prev_b, b, false);
  const int bad = compare<MAX_K>(k, a, b);
  const mhmkc_stats sa = a.inserter().stats(), sb = b.inserter().stats();
  if (bad || sa.ctg_kmers != sb.ctg_kmers) {
    std::cout << "FAILED k " << k << ": " << bad << " rows, ctg_kmers " << sa.ctg_kmers << " vs " << sb.ctg_kmers << "\n";
    return 1;
  }
  std::cout << "ROUND " << k << " " << b.get_local_num_kmers() << " " << sb.ctg_kmers << "\n";
  return next_round<MAX_K>(ch, i + 1, a, b);
}

template <int MAX_K>
int first_round(const Chain &ch) {
  const int k = ch.ks[0];
  Kmer<MAX_K>::set_k(k);
  std::vector<PackedReads *> list{ch.pr};
  Contigs none;
  KmerDHT<MAX_K> a(1000, 1 << 20, 100, false, true), b(1000, 1 << 20, 100, false, true);
  analyze_kmers<MAX_K>(k, 0, 33, list, 2, none, a, false);
  analyze_kmers<MAX_K>(k, 0, 33, list, 2, none, b, false);
  return next_round<MAX_K>(ch, 1, a, b);
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  PackedReads pr(33);
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string s, q;
    ss >> s >> q;
    pr.add_read("@r/1", s, q);
  }
  Chain ch{&pr, {}};
  std::stringstream kl(argv[2]);
  for (std::string x; std::getline(kl, x, ',');) ch.ks.push_back(std::atoi(x.c_str()));
  if (ch.ks.empty()) return 2;
  const int k = ch.ks[0];
  const int rc = k < 32 ? first_round<32>(ch) : k < 64 ? first_round<64>(ch) : k < 96 ? first_round<96>(ch) : first_round<128>(ch);
  if (rc == 0) std::cout << "OK\n";
  return rc;
}
