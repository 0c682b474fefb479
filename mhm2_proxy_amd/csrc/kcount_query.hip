// Queries on the finished table, on gfx950: a device index over the output rows, batched point lookups
// (KmerDHT::get_local_kmer_counts / kmer_exists, src/kcount/kmer_dht.cpp:198-219) and the de Bruijn links of every
// row (the lookup of get_next_step, src/dbjg_traversal.cpp:165-239, done once for all rows). DESIGN.md §3.11.
//
// The index is an open-addressing table in HBM with one 8-byte slot per entry, row | tag << 32: the row is the
// index into the output arrays (mhmkc_fetch order), the tag the low 32 bits of mhmkc_map_hash of the key, the home
// slot the hash's top bits. An empty slot is all ones (no row is 0xFFFFFFFF). Keys are distinct and never removed,
// so an insert is one 64-bit compare-and-swap per probe and a lookup reads one slot per probe; the key words
// themselves are read only where the tag matches. The host guarantees capacity > rows, so every probe chain ends at
// an empty slot.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"
#include "kcount_query_dev.hpp"
#include "kmer_ops.hpp"

namespace mhm {

namespace {

constexpr int Q_THREADS = 256;
constexpr unsigned long long SLOT_EMPTY = QSLOT_EMPTY;
constexpr uint32_t NO_ROW = Q_NO_ROW;

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

template <int NL>
__global__ __launch_bounds__(Q_THREADS) void k_query_build(const uint64_t *keys, uint64_t n, int nlo, QueryIndex ix) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t w[NL];
    load_key<NL>(keys, i, nlo, w);
    const uint64_t h = key_hash<NL>(w, nlo);
    const unsigned long long v = (unsigned long long)(uint32_t)i | (unsigned long long)(uint32_t)h << 32;
    uint64_t s = h >> ix.shift;
    // (capacity > n: a free slot exists for every row, so the chain ends)
    while (atomicCAS(&ix.slots[s], SLOT_EMPTY, v) != SLOT_EMPTY) s = (s + 1) & ix.mask;
  }
}

template <int NL>
__global__ __launch_bounds__(Q_THREADS) void k_query_lookup(const uint64_t *q, uint64_t n, int canonicalize, int k, int nlo,
                                                            QueryIndex ix, OutRows t, uint32_t *rows, uint16_t *counts,
                                                            char *left, char *right) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t w[NL];
    load_key<NL>(q, i, nlo, w);
    query_key<NL>(w, k, canonicalize);
    const uint32_t row = find_row<NL>(w, nlo, ix, t.keys);
    const bool hit = row != NO_ROW;
    if (rows) rows[i] = row;
    if (counts) counts[i] = hit ? t.counts[row] : (uint16_t)0;
    if (left) left[i] = hit ? t.left[row] : (char)0;
    if (right) right[i] = hit ? t.right[row] : (char)0;
  }
}

// Entry d * n + i: row i's neighbour in direction d (0 LEFT, 1 RIGHT) in row i's stored orientation, with the checks of
// get_next_step in its order, without the visited state.
template <int NL>
__global__ __launch_bounds__(Q_THREADS) void k_dbjg_links(OutRows t, uint64_t n, int k, int nlo, QueryIndex ix,
                                                          uint32_t *next, uint8_t *status) {
  const uint64_t total = 2 * n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const bool right_dirn = e >= n;
    const uint64_t i = right_dirn ? e - n : e;
    uint32_t nx = NO_ROW;
    uint8_t st;
    uint64_t key[NL];
    bool is_rc;
    uint32_t back_check;
    if (link_neighbour<NL>(t, i, right_dirn, k, nlo, key, is_rc, back_check, st)) {
      const uint32_t j = find_row<NL>(key, nlo, ix, t.keys);
      if (j == NO_ROW) {
        st = MHMKC_LINK_DEADEND;
      } else {
        nx = j;
        st = link_verdict(t.left[j], t.right[j], is_rc, right_dirn, back_check);
      }
    }
    next[e] = nx;
    status[e] = st;
  }
}

}  // namespace

hipError_t preload_query_kernels() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, (const void *)k_query_lookup<1>);
}

static bool index_ok(const QueryIndex &ix, uint64_t n_rows) {
  return ix.slots && ix.mask + 1 > n_rows && !((ix.mask + 1) & ix.mask) && ix.shift >= 1 && ix.shift <= 63 &&
         (ix.mask >> (64 - ix.shift)) == 0 && ix.n_rows == n_rows && n_rows < 0xffffffffull;
}

hipError_t launch_query_build(const uint64_t *keys, uint64_t n, int nl, int nlo, const QueryIndex &ix, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!index_ok(ix, n) || nlo < nl) return hipErrorInvalidValue;
  switch (nl) {
    case 1: k_query_build<1><<<grid_for(n), Q_THREADS, 0, s>>>(keys, n, nlo, ix); break;
    case 2: k_query_build<2><<<grid_for(n), Q_THREADS, 0, s>>>(keys, n, nlo, ix); break;
    case 3: k_query_build<3><<<grid_for(n), Q_THREADS, 0, s>>>(keys, n, nlo, ix); break;
    case 4: k_query_build<4><<<grid_for(n), Q_THREADS, 0, s>>>(keys, n, nlo, ix); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_query_lookup(const uint64_t *q, uint64_t n, bool canonicalize, int k, int nl, int nlo,
                               const QueryIndex &ix, const OutRows &t, uint32_t *rows, uint16_t *counts, char *left,
                               char *right, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!index_ok(ix, ix.n_rows) || nlo < nl || k / 32 + 1 != nl || k % 32 == 0) return hipErrorInvalidValue;
  const int c = canonicalize ? 1 : 0;
  switch (nl) {
    case 1: k_query_lookup<1><<<grid_for(n), Q_THREADS, 0, s>>>(q, n, c, k, nlo, ix, t, rows, counts, left, right); break;
    case 2: k_query_lookup<2><<<grid_for(n), Q_THREADS, 0, s>>>(q, n, c, k, nlo, ix, t, rows, counts, left, right); break;
    case 3: k_query_lookup<3><<<grid_for(n), Q_THREADS, 0, s>>>(q, n, c, k, nlo, ix, t, rows, counts, left, right); break;
    case 4: k_query_lookup<4><<<grid_for(n), Q_THREADS, 0, s>>>(q, n, c, k, nlo, ix, t, rows, counts, left, right); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_dbjg_links(const OutRows &t, uint64_t n, int k, int nl, int nlo, const QueryIndex &ix, uint32_t *next,
                             uint8_t *status, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!index_ok(ix, n) || nlo < nl || k / 32 + 1 != nl || k % 32 == 0) return hipErrorInvalidValue;
  switch (nl) {
    case 1: k_dbjg_links<1><<<grid_for(2 * n), Q_THREADS, 0, s>>>(t, n, k, nlo, ix, next, status); break;
    case 2: k_dbjg_links<2><<<grid_for(2 * n), Q_THREADS, 0, s>>>(t, n, k, nlo, ix, next, status); break;
    case 3: k_dbjg_links<3><<<grid_for(2 * n), Q_THREADS, 0, s>>>(t, n, k, nlo, ix, next, status); break;
    case 4: k_dbjg_links<4><<<grid_for(2 * n), Q_THREADS, 0, s>>>(t, n, k, nlo, ix, next, status); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mhm
