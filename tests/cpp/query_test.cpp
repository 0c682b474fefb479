// The query side of the C++ adapter (include/mhmkc_kcount.hpp) against the adapter's own KmerMap, after analyze_kmers:
//   KmerDHT::kmer_exists (forward and reverse-complement input), the batch KmerDHT::lookup (mhmkc_lookup on the GPU)
//   and HashTableInserter::dbjg_links (mhmkc_dbjg_links), whose rules are restated here over the KmerMap.
//   query_test <k> <seqqual.txt>      prints "OK <n_out> <queries>" or the first mismatches; exit status 1 on any
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <unordered_map>

#include "mhmkc_dbjg.hpp"

using namespace mhm2;

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
  int bad = 0;
  auto fail = [&](const std::string &what) {
    if (bad++ < 10) std::cout << "MISMATCH " << what << "\n";
  };

  // queries: every k-mer of the map, its reverse complement, and a one-base mutant of it
  std::mt19937_64 rng(k);
  std::vector<K> q;
  for (auto it = dht.local_kmers_begin(); it != dht.local_kmers_end(); ++it) {
    q.push_back(it->first);
    q.push_back(it->first.revcomp());
    std::string s = it->first.to_string();
    const size_t p = rng() % s.size();
    s[p] = "ACGT"[(std::string("ACGT").find(s[p]) + 1 + rng() % 3) % 4];
    q.push_back(K(s.c_str()));
  }
  for (int canon = 0; canon < 2; canon++) {
    std::vector<KmerCounts> out;
    std::vector<uint8_t> found;
    dht.lookup(q, canon != 0, out, found);
    if (out.size() != q.size() || found.size() != q.size()) fail("lookup sizes");
    for (size_t i = 0; i < q.size() && i < out.size(); i++) {
      K key = q[i];
      if (canon) {
        const K rc = key.revcomp();
        if (rc < key) key = rc;
      }
      KmerCounts *kc = dht.get_local_kmer_counts(key);
      if ((kc != nullptr) != (found[i] != 0)) {
        fail("lookup found " + q[i].to_string());
      } else if (kc && (kc->count != out[i].count || kc->left != out[i].left || kc->right != out[i].right)) {
        fail("lookup counts " + q[i].to_string());
      } else if (!kc && (out[i].count || out[i].left || out[i].right)) {
        fail("lookup miss not empty " + q[i].to_string());
      }
      if (canon && dht.kmer_exists(q[i]) != (found[i] != 0)) fail("kmer_exists " + q[i].to_string());
    }
  }
  // every k-mer of the map exists, forward and reverse-complemented
  for (auto it = dht.local_kmers_begin(); it != dht.local_kmers_end(); ++it)
    if (!dht.kmer_exists(it->first) || !dht.kmer_exists(it->first.revcomp())) fail("kmer_exists " + it->first.to_string());

  // the links: rows are those of mhmkc_fetch
  mhmkc_t h = dht.inserter().handle();
  uint64_t n = 0;
  check(mhmkc_device_output(h, nullptr, nullptr, nullptr, nullptr, &n), h, "mhmkc_device_output");
  if ((int64_t)n != dht.get_local_num_kmers()) fail("n_out");
  std::vector<uint64_t> keys(n * K::N_LONGS);
  check(mhmkc_fetch(h, keys.data(), nullptr, nullptr, nullptr), h, "mhmkc_fetch");
  std::vector<std::string> strs(n);
  std::unordered_map<std::string, uint32_t> row_of;
  for (uint64_t i = 0; i < n; i++) {
    strs[i] = K(&keys[i * K::N_LONGS]).to_string();
    row_of[strs[i]] = (uint32_t)i;
  }
  std::vector<uint32_t> next;
  std::vector<uint8_t> status;
  dht.inserter().dbjg_links(next, status);
  if (next.size() != 2 * n || status.size() != 2 * n) fail("links sizes");
  for (int d = 0; d < 2 && next.size() == 2 * n; d++) {
    for (uint64_t i = 0; i < n; i++) {
      KmerCounts *kc = dht.get_local_kmer_counts(K(strs[i].c_str()));
      uint32_t e_next = MHMKC_NO_ROW;
      uint8_t e_st;
      if (kc->left == 'X' || kc->right == 'X') {
        e_st = MHMKC_LINK_DEADEND;
      } else if (kc->left == 'F' || kc->right == 'F') {
        e_st = MHMKC_LINK_FORK;
      } else {
        DbjgKmer<MAX_K> kmer{strs[i]};
        DbjgKmer<MAX_K> nb = d ? kmer.forward_base(kc->right) : kmer.backward_base(kc->left);
        DbjgKmer<MAX_K> rc = nb.revcomp();
        const bool is_rc = rc.s < nb.s;
        KmerCounts *jc = dht.get_local_kmer_counts(K((is_rc ? rc : nb).s.c_str()));
        if (!jc) {
          e_st = MHMKC_LINK_DEADEND;
        } else {
          e_next = row_of.at((is_rc ? rc : nb).s);
          char l = jc->left, r = jc->right;
          if (l == 'X' || r == 'X') {
            e_st = MHMKC_LINK_DEADEND;
          } else if (l == 'F' || r == 'F') {
            e_st = MHMKC_LINK_FORK;
          } else {
            if (is_rc) {
              std::swap(l, r);
              l = dbjg_comp(l);
              r = dbjg_comp(r);
            }
            const bool ok = d ? l == kmer.front() : r == kmer.back();
            e_st = ok ? (uint8_t)(MHMKC_LINK_OK | (is_rc ? MHMKC_LINK_RC : 0)) : (uint8_t)MHMKC_LINK_CONFLICT;
          }
        }
      }
      if (next[d * n + i] != e_next || status[d * n + i] != e_st)
        fail("link " + strs[i] + " direction " + std::to_string(d) + ": " + std::to_string(next[d * n + i]) + "/" +
             std::to_string(status[d * n + i]) + " vs " + std::to_string(e_next) + "/" + std::to_string(e_st));
    }
  }
  if (bad) {
    std::cout << "FAILED " << bad << "\n";
    return 1;
  }
  std::cout << "OK " << n << " " << q.size() << "\n";
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
