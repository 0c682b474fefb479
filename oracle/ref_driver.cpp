// C ABI over the reference's own kcount code, built single-rank (TEST INFRASTRUCTURE ONLY, oracle/Makefile `ref`).
//
// This file is linked with the reference's unmodified kmer.cpp, kcount.cpp, kcount_cpu.cpp, kmer_dht.cpp,
// packed_reads.cpp, contigs.cpp, utils.cpp and hash_funcs.c, compiled against the one-rank stand-in headers of
// oracle/ref_standin. It holds no kcount logic: it turns arrays into the reference's PackedReads and Contigs, calls
// the reference's functions, and copies their results out. tests/oracle_lib.py binds it.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <type_traits>
#include <vector>

#include "upcxx_utils.hpp"
#include "contigs.hpp"
#include "kcount.hpp"
#include "kmer.hpp"
#include "kmer_dht.hpp"
#include "packed_reads.hpp"

namespace {

std::string last_error;

template <int N>
using max_k = std::integral_constant<int, N>;

// The reference picks MAX_K = (k / 32 + 1) * 32 (main.cpp), so n_longs = k / 32 + 1 words per key.
template <typename F>
auto dispatch(int k, int n_longs, F &&f) -> decltype(f(max_k<32>{})) {
  if (k < 1 || n_longs != k / 32 + 1) throw std::invalid_argument("n_longs must be k / 32 + 1, 1 <= k <= 127");
  switch (n_longs) {
    case 1: return f(max_k<32>{});
    case 2: return f(max_k<64>{});
    case 3: return f(max_k<96>{});
    case 4: return f(max_k<128>{});
  }
  throw std::invalid_argument("k beyond MAX_BUILD_KMER");
}

// Runs body; on an exception (the stand-in's DIE among them) records the message and returns fail.
template <typename R, typename F>
R guarded(R fail, F &&body) {
  try {
    return body();
  } catch (const std::exception &e) {
    last_error = e.what();
  } catch (...) {
    last_error = "unknown exception";
  }
  return fail;
}

// Kmer::get_minimizer_fast asserts m <= k (kmer.cpp); the Release build, which this is, has no asserts and its
// unsigned k - m loop bound runs off the key. The reference defines nothing there, so the driver refuses to ask.
void check_minimizer_len(int m, int k) {
  if (m > k || m > 28) throw std::domain_error("minimizer length above k (or 28): undefined in the reference");
}

struct WorldSize {
  explicit WorldSize(int n) { upcxx::standin::world_size = n; }
  ~WorldSize() { upcxx::standin::world_size = 1; }
};

struct RefTable {
  int n_longs = 0;
  std::vector<uint64_t> keys;
  std::vector<uint16_t> counts;
  std::vector<uint8_t> left, right;
  int64_t warnings = 0, dropped = 0;
};

// The sum of the counts behind every "Number dropped <count> (..%)" line of flush_inserts (kcount_cpu.cpp), the
// only place the CPU table's drop count leaves HashTableInserter.
int64_t dropped_in_log() {
  static const std::string tag = "Number dropped ";
  const std::string &log = upcxx_utils::standin::log_text;
  int64_t n = 0;
  for (size_t p = log.find(tag); p != std::string::npos; p = log.find(tag, p + 1)) n += atoll(log.c_str() + p + tag.size());
  return n;
}

}  // namespace

extern "C" {

const char *ref_last_error() { return last_error.c_str(); }

// what this build was compiled with (the reference makes both compile-time)
void ref_build_params(int *qual_cutoff, double *dyn_min_depth) {
  *qual_cutoff = KCOUNT_QUAL_CUTOFF;
  *dyn_min_depth = DYN_MIN_DEPTH;
}

int ref_kmer_from_string(const char *s, int k, int n_longs, uint64_t *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      K::set_k(k);
      K km;
      km.set_kmer(s);
      memcpy(out, km.get_longs(), n_longs * sizeof(uint64_t));
      return 0;
    });
  });
}

int ref_kmer_to_string(const uint64_t *longs, int k, int n_longs, char *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      K::set_k(k);
      K(longs).to_string(out);
      return 0;
    });
  });
}

// Kmer::get_kmers over seq: the k-mers in order, n_longs words each; returns how many (or -1).
int64_t ref_get_kmers(const char *seq, int64_t len, int k, int n_longs, uint64_t *out, int64_t cap) {
  return guarded((int64_t)-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) -> int64_t {
      using K = Kmer<decltype(mk)::value>;
      K::set_k(k);
      std::vector<K> kmers;
      K::get_kmers(k, std::string(seq, len), kmers);
      if ((int64_t)kmers.size() > cap) throw std::length_error("get_kmers: output too small");
      for (size_t i = 0; i < kmers.size(); i++) memcpy(out + i * n_longs, kmers[i].get_longs(), n_longs * sizeof(uint64_t));
      return kmers.size();
    });
  });
}

int ref_kmer_revcomp(const uint64_t *longs, int k, int n_longs, uint64_t *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      K::set_k(k);
      K rc = K(longs).revcomp();
      memcpy(out, rc.get_longs(), n_longs * sizeof(uint64_t));
      return 0;
    });
  });
}

// operator<: 1 if a < b, 0 if not, -1 on error
int ref_kmer_less(const uint64_t *a, const uint64_t *b, int k, int n_longs) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      K::set_k(k);
      return K(a) < K(b) ? 1 : 0;
    });
  });
}

int ref_kmer_hash(const uint64_t *longs, int k, int n_longs, uint64_t *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      K::set_k(k);
      *out = K(longs).hash();
      return 0;
    });
  });
}

int ref_get_minimizer_fast(const uint64_t *longs, int k, int n_longs, int m, int least_complement, uint64_t *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      check_minimizer_len(m, k);
      K::set_k(k);
      *out = K(longs).get_minimizer_fast(m, least_complement != 0);
      return 0;
    });
  });
}

int ref_minimizer_hash_fast(const uint64_t *longs, int k, int n_longs, int m, uint64_t *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      using K = Kmer<decltype(mk)::value>;
      check_minimizer_len(m, k);
      K::set_k(k);
      *out = K(longs).minimizer_hash_fast(m);
      return 0;
    });
  });
}

// KmerDHT::get_kmer_target_rank of n keys in a world of `world` ranks, and the minimizer length the KmerDHT
// constructor chose for k (returned; -1 on error).
int ref_kmer_target_ranks(const uint64_t *keys, uint64_t n, int k, int n_longs, int world, int32_t *out) {
  return guarded(-1, [&] {
    return dispatch(k, n_longs, [&](auto mk) {
      constexpr int MAX_K = decltype(mk)::value;
      using K = Kmer<MAX_K>;
      if (world < 1) throw std::invalid_argument("world must be at least 1");
      K::set_k(k);
      WorldSize ws(world);
      upcxx::dist_object<KmerDHT<MAX_K>> dht(upcxx::world(), (uint64_t)1024, 1 << 20, 100, false, false);
      check_minimizer_len(dht->get_minimizer_len(), k);
      for (uint64_t i = 0; i < n; i++) out[i] = dht->get_kmer_target_rank(K(keys + i * n_longs));
      return dht->get_minimizer_len();
    });
  });
}

// The reference's analyze_kmers over reads (PackedRead bytes: base code | quality << 3, n_reads + 1 offsets) and
// contigs (ASCII back to back, n_ctgs + 1 offsets, one depth each): a handle to its final table, or NULL.
void *ref_analyze_kmers(int k, int n_longs, int qual_offset, int dmin_thres, int world, const uint8_t *bytes,
                        const uint64_t *offs, uint64_t n_reads, const char *ctg_blob, const uint64_t *ctg_offs,
                        const uint16_t *ctg_depths, uint64_t n_ctgs) {
  return guarded((void *)nullptr, [&] {
    return dispatch(k, n_longs, [&](auto mk) -> void * {
      constexpr int MAX_K = decltype(mk)::value;
      using K = Kmer<MAX_K>;
      if (world < 1) throw std::invalid_argument("world must be at least 1");
      K::set_k(k);
      WorldSize ws(world);
      upcxx_utils::standin::log_text.clear();
      upcxx_utils::standin::num_warnings = 0;

      uint64_t windows = 0;
      PackedReads reads(qual_offset, "");
      std::string seq, quals;
      for (uint64_t r = 0; r < n_reads; r++) {
        uint64_t lo = offs[r], len = offs[r + 1] - lo;
        if (len > UINT16_MAX) throw std::length_error("read longer than PackedRead's 16-bit length");
        seq.resize(len);
        quals.resize(len);
        for (uint64_t i = 0; i < len; i++) {
          unsigned code = bytes[lo + i] & 7;
          if (code > 4) throw std::invalid_argument("base code above 4 in a PackedRead byte");
          seq[i] = "ACGTN"[code];
          quals[i] = (char)(qual_offset + (bytes[lo + i] >> 3));
        }
        reads.add_read("@r" + std::to_string(r) + "/1", seq, quals);
        if (len >= (uint64_t)k) windows += len - k + 1;
      }
      Contigs ctgs;
      for (uint64_t c = 0; c < n_ctgs; c++) {
        uint64_t lo = ctg_offs[c], len = ctg_offs[c + 1] - lo;
        ctgs.add_contig({.id = (int64_t)c, .seq = std::string(ctg_blob + lo, len), .depth = (double)ctg_depths[c]});
        if (len >= (uint64_t)k) windows += len - k + 1;
      }

      // HashTableInserter::init allocates 3 slots per requested element, so no insert meets the 100-probe limit
      uint64_t my_num_kmers = windows + 1024;
      std::vector<PackedReads *> reads_list{&reads};
      upcxx::dist_object<KmerDHT<MAX_K>> dht(upcxx::world(), my_num_kmers, 1 << 20, 100, false, false);
      check_minimizer_len(dht->get_minimizer_len(), k);
      analyze_kmers<MAX_K>(k, 0, qual_offset, reads_list, dmin_thres, ctgs, dht, false);

      auto t = new RefTable;
      t->n_longs = n_longs;
      for (auto it = dht->local_kmers_begin(); it != dht->local_kmers_end(); ++it) {
        const uint64_t *l = it->first.get_longs();
        t->keys.insert(t->keys.end(), l, l + n_longs);
        t->counts.push_back(it->second.count);
        t->left.push_back((uint8_t)it->second.left);
        t->right.push_back((uint8_t)it->second.right);
      }
      t->warnings = upcxx_utils::standin::num_warnings;
      t->dropped = dropped_in_log();
      return t;
    });
  });
}

uint64_t ref_table_size(void *h) { return ((RefTable *)h)->counts.size(); }

// counters[0] = the stand-in's WARN/SWARN count, counters[1] = inserts the CPU table dropped
void ref_table_counters(void *h, int64_t *counters) {
  counters[0] = ((RefTable *)h)->warnings;
  counters[1] = ((RefTable *)h)->dropped;
}

void ref_table_fetch(void *h, uint64_t *keys, uint16_t *counts, uint8_t *left, uint8_t *right) {
  auto t = (RefTable *)h;
  size_t n = t->counts.size();
  if (!n) return;
  memcpy(keys, t->keys.data(), n * t->n_longs * sizeof(uint64_t));
  memcpy(counts, t->counts.data(), n * sizeof(uint16_t));
  memcpy(left, t->left.data(), n);
  memcpy(right, t->right.data(), n);
}

void ref_table_free(void *h) { delete (RefTable *)h; }

}  // extern "C"
