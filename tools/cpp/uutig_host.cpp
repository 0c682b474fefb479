// The route to a round's uutigs that exists without mhmkc_uutigs, timed for tools/uutig_bench.py in its process: the
// hand-off of the finished table into the C++ adapter's KmerMap (include/mhmkc_kcount.hpp load_ordered, what bench.py
// --full reports as `kmermap`), then mhm2::traverse_debruijn_graph (include/mhmkc_dbjg.hpp) on one thread; and the
// comparison of its contigs with the device's. Not part of the library.
//   int mhmkc_uhost(mhmkc_t h, int k, int threads, int traverse, double *ms /*[4]*/, uint64_t *v /*[8]*/)
// ms: 0 hand-off (load_ordered into a KmerMap), 1 the traversal's own table (mhmkc_fetch + KmerDHT::load_table, not
//     part of the route: the adapter keeps its map private), 2 traverse_debruijn_graph, 3 mhmkc_uutigs_fetch.
// v:  0-2 the host's contigs, bases and digest, 3-5 the device's, 6 the contigs equal in id, strand and depth,
//     7 those equal as the other strand (even k). The digest is order-free: the sum over the contigs of a 64-bit hash
//     of the canonical sequence and the depth's bits. traverse = 0 skips the host traversal (v[0..2], v[6..7] = 0).
// Returns 0, or -1 on a library error.
#include <chrono>
#include <vector>

#include "mhmkc_dbjg.hpp"

static std::string revcomp(const std::string &s) {
  std::string r(s.rbegin(), s.rend());
  for (char &c : r) c = mhm2::dbjg_comp(c);
  return r;
}

static uint64_t ctg_hash(const std::string &seq, double depth) {
  const std::string rc = revcomp(seq);
  const std::string &c = rc < seq ? rc : seq;
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char ch : c) h = (h ^ ch) * 0x100000001b3ull;
  uint64_t d;
  static_assert(sizeof d == sizeof depth, "double");
  std::memcpy(&d, &depth, 8);
  h = (h ^ d) * 0xBF58476D1CE4E5B9ull;
  return h ^ (h >> 31);
}

template <int MAX_K>
static int run(mhmkc_t h, int k, int threads, int traverse, double *ms, uint64_t *v) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  mhm2::Kmer<MAX_K>::set_k(k);
  mhmkc_stats st;
  if (mhmkc_get_stats(h, &st) != MHMKC_OK) return -1;
  const uint64_t n = st.n_out;
  for (int i = 0; i < 4; i++) ms[i] = 0;
  for (int i = 0; i < 8; i++) v[i] = 0;
  {
    mhm2::KmerMap<MAX_K> map;
    const auto t0 = clk::now();
    mhm2::load_ordered<MAX_K>(h, map, n, threads, 4u << 20, nullptr);
    ms[0] = since(t0);
  }
  mhm2::Contigs host;
  if (traverse) {
    constexpr int nl = mhm2::Kmer<MAX_K>::N_LONGS;
    mhm2::RankInfo ri;
    ri.table_only = true;
    mhm2::KmerDHT<MAX_K> dht(1000, 1 << 20, 100, false, true, ri);
    {
      const auto t1 = clk::now();
      std::vector<uint64_t> keys(n * nl);
      std::vector<uint16_t> counts(n);
      std::vector<char> left(n), right(n);
      if (mhmkc_fetch(h, keys.data(), counts.data(), left.data(), right.data()) != MHMKC_OK) return -1;
      dht.load_table(keys.data(), counts.data(), left.data(), right.data(), n);
      ms[1] = since(t1);
    }
    const auto t2 = clk::now();
    mhm2::traverse_debruijn_graph<MAX_K>((unsigned)k, dht, host);
    ms[2] = since(t2);
  }
  uint64_t nc = 0, nb = 0;
  if (mhmkc_uutigs(h, &nc, &nb) != MHMKC_OK) return -1;
  std::vector<uint64_t> offs(nc + 1);
  std::vector<char> seqs(nb);
  std::vector<double> depths(nc);
  const auto t3 = clk::now();
  if (mhmkc_uutigs_fetch(h, offs.data(), seqs.data(), depths.data(), nullptr) != MHMKC_OK) return -1;
  ms[3] = since(t3);
  v[3] = nc;
  v[4] = nb;
  for (uint64_t c = 0; c < nc; c++) {
    const std::string s(seqs.data() + offs[c], seqs.data() + offs[c + 1]);
    v[5] += ctg_hash(s, depths[c]);
    if (traverse && c < host.size() && host[c].depth == depths[c]) {
      if (host[c].seq == s)
        v[6]++;
      else if (host[c].seq == revcomp(s))
        v[7]++;
    }
  }
  v[0] = host.size();
  for (auto &c : host) {
    v[1] += c.seq.size();
    v[2] += ctg_hash(c.seq, c.depth);
  }
  return 0;
}

extern "C" int mhmkc_uhost_abi(void) { return MHMKC_ABI_VERSION; }

extern "C" int mhmkc_uhost(mhmkc_t h, int k, int threads, int traverse, double *ms, uint64_t *v) {
  if (threads < 1 || !ms || !v) return -1;
  switch (k / 32 + 1) {
    case 1: return run<32>(h, k, threads, traverse, ms, v);
    case 2: return run<64>(h, k, threads, traverse, ms, v);
    case 3: return run<96>(h, k, threads, traverse, ms, v);
    case 4: return run<128>(h, k, threads, traverse, ms, v);
  }
  return -1;
}
