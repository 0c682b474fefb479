// The route that exists without the device queries, timed for tools/query_bench.py in its process: the hand-off of the
// finished table into the C++ adapter's KmerMap (include/mhmkc_kcount.hpp load_ordered, what bench.py --full reports as
// `kmermap`), then KmerMap::find on n keys with `threads` host threads (KmerDHT::get_local_kmer_counts, one per key).
// Not part of the library.
//   int mhmkc_qfind(mhmkc_t h, int k, int threads, const uint64_t *keys, uint64_t n, int runs, double *handoff_ms,
//                   double *find_ms /*[runs]*/, uint64_t *hits)
// keys: n * N_LONGS words, looked up as given (the caller passes canonical forms where it wants kmer_exists' answer).
// Returns 0, or -1 on a library error.
#include <chrono>
#include <thread>
#include <vector>

#include "mhmkc_kcount.hpp"

template <int MAX_K>
static int run(mhmkc_t h, int k, int threads, const uint64_t *keys, uint64_t n, int runs, double *handoff_ms,
               double *find_ms, uint64_t *hits) {
  using clk = std::chrono::steady_clock;
  mhm2::Kmer<MAX_K>::set_k(k);
  mhmkc_stats st;
  if (mhmkc_get_stats(h, &st) != MHMKC_OK) return -1;
  mhm2::KmerMap<MAX_K> map;
  const auto t0 = clk::now();
  mhm2::load_ordered<MAX_K>(h, map, st.n_out, threads, 4u << 20, nullptr);
  if (handoff_ms) *handoff_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  constexpr int nl = mhm2::Kmer<MAX_K>::N_LONGS;
  const mhm2::KmerMap<MAX_K> &cmap = map;
  for (int r = 0; r < runs; r++) {
    std::vector<uint64_t> part((size_t)threads, 0);
    std::vector<std::thread> th;
    const auto t1 = clk::now();
    for (int t = 0; t < threads; t++)
      th.emplace_back([&, t] {
        const uint64_t a = n * (uint64_t)t / threads, b = n * (uint64_t)(t + 1) / threads;
        uint64_t c = 0;
        for (uint64_t i = a; i < b; i++) c += cmap.find(mhm2::Kmer<MAX_K>(keys + i * nl)) != cmap.end();
        part[(size_t)t] = c;
      });
    for (auto &x : th) x.join();
    find_ms[r] = std::chrono::duration<double, std::milli>(clk::now() - t1).count();
    uint64_t c = 0;
    for (uint64_t v : part) c += v;
    if (hits) *hits = c;
  }
  return 0;
}

extern "C" int mhmkc_qfind_abi(void) { return MHMKC_ABI_VERSION; }

extern "C" int mhmkc_qfind(mhmkc_t h, int k, int threads, const uint64_t *keys, uint64_t n, int runs, double *handoff_ms,
                           double *find_ms, uint64_t *hits) {
  if (threads < 1 || runs < 1) return -1;
  switch (k / 32 + 1) {
    case 1: return run<32>(h, k, threads, keys, n, runs, handoff_ms, find_ms, hits);
    case 2: return run<64>(h, k, threads, keys, n, runs, handoff_ms, find_ms, hits);
    case 3: return run<96>(h, k, threads, keys, n, runs, handoff_ms, find_ms, hits);
    case 4: return run<128>(h, k, threads, keys, n, runs, handoff_ms, find_ms, hits);
  }
  return -1;
}
