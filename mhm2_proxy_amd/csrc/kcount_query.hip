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
#include "kmer_ops.hpp"

namespace mhm {

namespace {

constexpr int Q_THREADS = 256;
constexpr unsigned long long SLOT_EMPTY = ~0ull;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

// mhmkc_map_hash of a key whose first NL words are w and whose other nlo - NL words are zero (the output rows'
// layout for n_longs > k/32 + 1)
template <int NL>
__device__ __forceinline__ uint64_t key_hash(const uint64_t *w, int nlo) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    h = (h ^ w[i]) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 31;
  }
  for (int i = NL; i < nlo; i++) {
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 31;
  }
  h *= 0x94D049BB133111EBull;
  return h ^ (h >> 29);
}

template <int NL>
__device__ __forceinline__ void load_key(const uint64_t *keys, uint64_t i, int nlo, uint64_t *w) {
#pragma unroll
  for (int j = 0; j < NL; j++) w[j] = keys[i * (uint64_t)nlo + j];
}

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

// The row holding key w (NL words, the unused bits zero), or NO_ROW.
template <int NL>
__device__ __forceinline__ uint32_t find_row(const uint64_t *w, int nlo, const QueryIndex &ix, const uint64_t *keys) {
  const uint64_t h = key_hash<NL>(w, nlo);
  const uint32_t tag = (uint32_t)h;
  uint64_t s = h >> ix.shift;
  for (uint64_t probes = 0; probes <= ix.mask; probes++) {
    const unsigned long long v = ix.slots[s];
    const uint32_t row = (uint32_t)v;
    if (row == NO_ROW) return NO_ROW;
    if ((uint32_t)(v >> 32) == tag && (uint64_t)row < ix.n_rows) {
      bool eq = true;
#pragma unroll
      for (int j = 0; j < NL; j++) eq &= keys[(uint64_t)row * nlo + j] == w[j];
      if (eq) return row;
    }
    s = (s + 1) & ix.mask;
  }
  return NO_ROW;
}

template <int NL>
__global__ __launch_bounds__(Q_THREADS) void k_query_lookup(const uint64_t *q, uint64_t n, int canonicalize, int k, int nlo,
                                                            QueryIndex ix, OutRows t, uint32_t *rows, uint16_t *counts,
                                                            char *left, char *right) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t w[NL];
    load_key<NL>(q, i, nlo, w);
    w[NL - 1] &= top_mask(k - 32 * (NL - 1));
    if (canonicalize) {
      uint64_t rc[NL];
      revcomp<NL>(w, rc, k);
      if (kmer_less<NL>(rc, w)) {
#pragma unroll
        for (int j = 0; j < NL; j++) w[j] = rc[j];
      }
    }
    const uint32_t row = find_row<NL>(w, nlo, ix, t.keys);
    const bool hit = row != NO_ROW;
    if (rows) rows[i] = row;
    if (counts) counts[i] = hit ? t.counts[row] : (uint16_t)0;
    if (left) left[i] = hit ? t.left[row] : (char)0;
    if (right) right[i] = hit ? t.right[row] : (char)0;
  }
}

__device__ __forceinline__ uint32_t base_code(char c) {  // set_kmer's bit trick (src/kmer.cpp:274-296)
  const uint32_t x = ((uint32_t)c & 4u) >> 1;
  return x + ((x ^ ((uint32_t)c & 2u)) >> 1);
}
__device__ __forceinline__ char base_char(uint32_t code) { return (char)((0x54474341u >> (8 * code)) & 0xffu); }
__device__ __forceinline__ char comp_char(char c) { return base_char(3u - base_code(c)); }

// Entry d * n + i: row i's neighbour in direction d (0 LEFT, 1 RIGHT) in row i's stored orientation, with the checks of
// get_next_step in its order, without the visited state.
template <int NL>
__global__ __launch_bounds__(Q_THREADS) void k_dbjg_links(OutRows t, uint64_t n, int k, int nlo, QueryIndex ix,
                                                          uint32_t *next, uint8_t *status) {
  const uint64_t total = 2 * n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const bool right_dirn = e >= n;
    const uint64_t i = right_dirn ? e - n : e;
    const char l = t.left[i], r = t.right[i];
    uint32_t nx = NO_ROW;
    uint8_t st;
    if (l == 'X' || r == 'X') {
      st = MHMKC_LINK_DEADEND;
    } else if (l == 'F' || r == 'F') {
      st = MHMKC_LINK_FORK;
    } else {
      uint64_t w[NL], nb[NL], rc[NL];
      load_key<NL>(t.keys, i, nlo, w);
      const int kl = k - 32 * (NL - 1);  // bases in the last word
      uint32_t back_check;               // the base the neighbour's extension must lead back to
      if (right_dirn) {                  // forward_base(right), back-check against front()
#pragma unroll
        for (int j = 0; j < NL; j++) nb[j] = (w[j] << 2) | (j + 1 < NL ? w[j + 1] >> 62 : 0ull);
        nb[NL - 1] |= (uint64_t)base_code(r) << (64 - 2 * kl);
        back_check = (uint32_t)(w[0] >> 62);
      } else {  // backward_base(left), back-check against back()
#pragma unroll
        for (int j = NL - 1; j >= 0; j--) nb[j] = (w[j] >> 2) | (j > 0 ? w[j - 1] << 62 : 0ull);
        nb[0] |= (uint64_t)base_code(l) << 62;
        nb[NL - 1] &= top_mask(kl);
        back_check = (uint32_t)(w[NL - 1] >> (64 - 2 * kl)) & 3u;
      }
      revcomp<NL>(nb, rc, k);
      const bool is_rc = kmer_less<NL>(rc, nb);
      const uint32_t j = find_row<NL>(is_rc ? rc : nb, nlo, ix, t.keys);
      if (j == NO_ROW) {
        st = MHMKC_LINK_DEADEND;
      } else {
        nx = j;
        char jl = t.left[j], jr = t.right[j];
        if (jl == 'X' || jr == 'X') {
          st = MHMKC_LINK_DEADEND;
        } else if (jl == 'F' || jr == 'F') {
          st = MHMKC_LINK_FORK;
        } else {
          if (is_rc) {
            const char tmp = jl;
            jl = comp_char(jr);
            jr = comp_char(tmp);
          }
          const char want = base_char(back_check);
          const bool ok = right_dirn ? jl == want : jr == want;
          st = ok ? (uint8_t)(MHMKC_LINK_OK | (is_rc ? MHMKC_LINK_RC : 0)) : (uint8_t)MHMKC_LINK_CONFLICT;
        }
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
