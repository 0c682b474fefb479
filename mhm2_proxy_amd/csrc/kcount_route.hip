// Queries answered by the rank that owns the key, on gfx950: the reference's traversal computes
// get_kmer_target_rank of a neighbour and asks that rank by rpc (src/dbjg_traversal.cpp:228-236,260-274,
// src/kcount/kmer_dht.cpp:193-219). Here a batch of queries is grouped by owner, the groups travel between the ranks,
// every owner probes its own index (kcount_query.hip) and the 8-byte replies travel back to the place their queries
// hold in the asker's layout.
//
// A round serves m queries of one rank. The queries come from one of two sources: a batch of keys (mhmkc_lookup_ranks)
// or the entries [e0, e0 + m) of the rank's 2 * n_rows link entries, whose query is the neighbour of the entry's row
// (mhmkc_dbjg_links_ranks; an entry that its own row ends asks nothing). Both kernels that need a query's key, the
// route and the pack, recompute it from the source: the round keeps one byte (the owner) and one word (the place) per
// query besides the send layout and the replies.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"
#include "kcount_query_dev.hpp"
#include "kmer_ops.hpp"

namespace mhm {

namespace {

constexpr int R_THREADS = 256;
constexpr uint8_t NO_DEST = 0xFF;  // an entry that asks nothing
constexpr uint32_t NO_POS = 0xFFFFFFFFu;

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

// The key of query i of the round: false when the entry asks nothing.
template <int NL, bool LINKS>
__device__ __forceinline__ bool route_key(const RouteSource &src, uint64_t i, int k, int nlo, uint64_t *w) {
  if (LINKS) {
    const uint64_t e = src.e0 + i;
    const bool right_dirn = e >= src.n_rows;
    bool is_rc;
    uint32_t back_check;
    uint8_t st;
    return link_neighbour<NL>(src.t, right_dirn ? e - src.n_rows : e, right_dirn, k, nlo, w, is_rc, back_check, st);
  }
  load_key<NL>(src.q, i, nlo, w);
  query_key<NL>(w, k, src.canonicalize);
  return true;
}

// dest[i] = the owner of query i (NO_DEST: none); hist[r] += the queries of owner r, through an LDS histogram: one global
// add per owner and workgroup
template <int NL, bool LINKS>
__global__ __launch_bounds__(R_THREADS) void k_route(RouteSource src, uint64_t m, int k, int nlo, int mlen, int G,
                                                     uint8_t *dest, unsigned long long *hist) {
  __shared__ unsigned int lh[256];
  for (int i = threadIdx.x; i < G; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t w[NL];
    uint8_t d = NO_DEST;
    if (route_key<NL, LINKS>(src, i, k, nlo, w)) {
      d = (uint8_t)(quick_hash(minimizer_fast(w, k, mlen)) % (uint64_t)G);
      atomicAdd(&lh[d], 1u);
    }
    dest[i] = d;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < G; i += blockDim.x)
    if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

// The queries laid out by owner, NL words each, owner r's from cursor[r] on (cursor = the owners' first places; the order
// inside an owner's group is free): each workgroup reserves one run per owner and tile with one atomic and ranks its
// queries in LDS, as k_owner_scatter does. pos[i] = the place of query i, where its reply will lie (NO_POS: none).
template <int NL, bool LINKS>
__global__ __launch_bounds__(R_THREADS) void k_route_pack(RouteSource src, uint64_t m, int k, int nlo, const uint8_t *dest,
                                                          int G, unsigned long long *cursor, uint64_t *send, uint32_t *pos) {
  __shared__ unsigned int lc[256];
  __shared__ unsigned long long lb[256];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < m; i0 += stride) {
    for (int i = threadIdx.x; i < G; i += blockDim.x) lc[i] = 0;
    __syncthreads();
    const uint64_t i = i0 + threadIdx.x;
    uint32_t d = NO_DEST, rk = 0;
    if (i < m) {
      d = dest[i];
      if (d < (uint32_t)G) rk = atomicAdd(&lc[d], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < G; j += blockDim.x) lb[j] = lc[j] ? atomicAdd(&cursor[j], (unsigned long long)lc[j]) : 0ull;
    __syncthreads();
    if (i < m) {
      uint32_t p = NO_POS;
      if (d < (uint32_t)G) {
        const uint64_t o = lb[d] + rk;
        uint64_t w[NL];
        if (o < m && route_key<NL, LINKS>(src, i, k, nlo, w)) {  // (the layout holds m places)
          p = (uint32_t)o;
#pragma unroll
          for (int j = 0; j < NL; j++) send[o * NL + j] = w[j];
        }
      }
      pos[i] = p;
    }
    __syncthreads();
  }
}

// One reply per received key: row | count << 32 | left << 48 | right << 56, a miss MHMKC_NO_ROW and zeros. A rank
// without rows has no index and misses everything.
template <int NL>
__global__ __launch_bounds__(R_THREADS) void k_route_answer(const uint64_t *keys, uint64_t n, int nlo, QueryIndex ix,
                                                            OutRows t, unsigned long long *reply) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    unsigned long long r = Q_NO_ROW;
    if (ix.n_rows) {
      uint64_t w[NL];
      load_key<NL>(keys, i, NL, w);
      const uint32_t row = find_row<NL>(w, nlo, ix, t.keys);
      if (row != Q_NO_ROW)
        r = (unsigned long long)row | (unsigned long long)t.counts[row] << 32 |
            (unsigned long long)(uint8_t)t.left[row] << 48 | (unsigned long long)(uint8_t)t.right[row] << 56;
    }
    reply[i] = r;
  }
}

// The reply of query i, checked: its place lies inside the layout, and its row inside the owner's announced rows.
// Anything else reads as a miss (a bad peer gives wrong answers, never a fault).
__device__ __forceinline__ unsigned long long checked_reply(const unsigned long long *reply, uint32_t p, uint64_t layout,
                                                            uint32_t d, int G, const unsigned long long *n_rows_of) {
  if (p == NO_POS || (uint64_t)p >= layout || d >= (uint32_t)G) return Q_NO_ROW;
  const unsigned long long r = reply[p];
  return (r & 0xFFFFFFFFull) < n_rows_of[d] && (uint32_t)r != Q_NO_ROW ? r : (unsigned long long)Q_NO_ROW;
}

__global__ __launch_bounds__(R_THREADS) void k_route_unpack(const unsigned long long *reply, const uint32_t *pos,
                                                            const uint8_t *dest, uint64_t m, uint64_t layout, int G,
                                                            const unsigned long long *n_rows_of, uint8_t *ranks,
                                                            uint32_t *rows, uint16_t *counts, char *left, char *right) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = dest[i];
    const unsigned long long r = checked_reply(reply, pos[i], layout, d, G, n_rows_of);
    if (ranks) ranks[i] = (uint8_t)d;
    if (rows) rows[i] = (uint32_t)r;
    if (counts) counts[i] = (uint16_t)(r >> 32);
    if (left) left[i] = (char)(r >> 48);
    if (right) right[i] = (char)(r >> 56);
  }
}

// Entries [e0, e0 + m) of the links: steps 1 and 2 recomputed from the row (is_rc and the back-check are not stored),
// step 3 from the neighbour's reply.
template <int NL>
__global__ __launch_bounds__(R_THREADS) void k_route_verdict(RouteSource src, uint64_t m, int k, int nlo,
                                                             const unsigned long long *reply, const uint32_t *pos,
                                                             const uint8_t *dest, uint64_t layout, int G,
                                                             const unsigned long long *n_rows_of, uint8_t *next_rank,
                                                             uint32_t *next_row, uint8_t *status) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e = src.e0 + i;
    const bool right_dirn = e >= src.n_rows;
    uint64_t key[NL];
    bool is_rc;
    uint32_t back_check;
    uint8_t st, nr = MHMKC_NO_RANK;
    uint32_t nx = Q_NO_ROW;
    if (link_neighbour<NL>(src.t, right_dirn ? e - src.n_rows : e, right_dirn, k, nlo, key, is_rc, back_check, st)) {
      const uint32_t d = dest[i];
      const unsigned long long r = checked_reply(reply, pos[i], layout, d, G, n_rows_of);
      if ((uint32_t)r == Q_NO_ROW) {
        st = MHMKC_LINK_DEADEND;
      } else {
        nr = (uint8_t)d;
        nx = (uint32_t)r;
        st = link_verdict((char)(r >> 48), (char)(r >> 56), is_rc, right_dirn, back_check);
      }
    }
    next_rank[e] = nr;
    next_row[e] = nx;
    status[e] = st;
  }
}

// one rank: rank 0 wherever the single-rank links name a row
__global__ __launch_bounds__(R_THREADS) void k_route_rank0(const uint32_t *next, uint64_t n, uint8_t *next_rank) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    next_rank[i] = next[i] == Q_NO_ROW ? (uint8_t)MHMKC_NO_RANK : (uint8_t)0;
}

bool shape_ok(int k, int nl, int nlo, int mlen, int G) {
  return nl >= 1 && nl <= 4 && nlo >= nl && k / 32 + 1 == nl && k % 32 != 0 && mlen >= 1 && mlen <= 28 && mlen <= k &&
         G >= 1 && G <= 255;
}

// a round's m queries have 32-bit places; link entries lie inside the rank's 2 * n_rows
bool source_ok(const RouteSource &src, uint64_t m) {
  return m < 0xffffffffull && (src.links ? src.e0 + m <= 2 * src.n_rows && src.t.keys && src.t.left && src.t.right : src.q != nullptr);
}

bool index_ok(const QueryIndex &ix) {
  return !ix.n_rows || (ix.slots && ix.mask + 1 > ix.n_rows && !((ix.mask + 1) & ix.mask) && ix.shift >= 1 &&
                        ix.shift <= 63 && (ix.mask >> (64 - ix.shift)) == 0 && ix.n_rows < 0xffffffffull);
}

}  // namespace

// (the code object of this file is loaded at create, as the other query kernels')
hipError_t preload_route_kernels() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, (const void *)k_route_unpack);
}

#define ROUTE_SWITCH(KERNEL, ...)                                                              \
  switch (nl) {                                                                                \
    case 1: KERNEL(1, __VA_ARGS__); break;                                                     \
    case 2: KERNEL(2, __VA_ARGS__); break;                                                     \
    case 3: KERNEL(3, __VA_ARGS__); break;                                                     \
    case 4: KERNEL(4, __VA_ARGS__); break;                                                     \
    default: return hipErrorInvalidValue;                                                      \
  }

hipError_t launch_route(const RouteSource &src, uint64_t m, int k, int nl, int nlo, int mlen, int n_ranks, uint8_t *dest,
                        unsigned long long *hist, hipStream_t s) {
  if (!m) return hipSuccess;
  if (!shape_ok(k, nl, nlo, mlen, n_ranks) || !source_ok(src, m)) return hipErrorInvalidValue;
#define K_ROUTE(NLV, ...)                                                                                    \
  if (src.links) k_route<NLV, true><<<grid_for(m), R_THREADS, 0, s>>>(__VA_ARGS__);                         \
  else k_route<NLV, false><<<grid_for(m), R_THREADS, 0, s>>>(__VA_ARGS__)
  ROUTE_SWITCH(K_ROUTE, src, m, k, nlo, mlen, n_ranks, dest, hist)
#undef K_ROUTE
  return hipGetLastError();
}

hipError_t launch_route_pack(const RouteSource &src, uint64_t m, int k, int nl, int nlo, const uint8_t *dest, int n_ranks,
                             unsigned long long *cursor, uint64_t *send, uint32_t *pos, hipStream_t s) {
  if (!m) return hipSuccess;
  if (!shape_ok(k, nl, nlo, 1, n_ranks) || !source_ok(src, m)) return hipErrorInvalidValue;
#define K_PACK(NLV, ...)                                                                                     \
  if (src.links) k_route_pack<NLV, true><<<grid_for(m), R_THREADS, 0, s>>>(__VA_ARGS__);                    \
  else k_route_pack<NLV, false><<<grid_for(m), R_THREADS, 0, s>>>(__VA_ARGS__)
  ROUTE_SWITCH(K_PACK, src, m, k, nlo, dest, n_ranks, cursor, send, pos)
#undef K_PACK
  return hipGetLastError();
}

hipError_t launch_route_answer(const uint64_t *keys, uint64_t n, int k, int nl, int nlo, const QueryIndex &ix,
                               const OutRows &t, unsigned long long *reply, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!shape_ok(k, nl, nlo, 1, 1) || !index_ok(ix)) return hipErrorInvalidValue;
#define K_ANSWER(NLV, ...) k_route_answer<NLV><<<grid_for(n), R_THREADS, 0, s>>>(__VA_ARGS__)
  ROUTE_SWITCH(K_ANSWER, keys, n, nlo, ix, t, reply)
#undef K_ANSWER
  return hipGetLastError();
}

hipError_t launch_route_unpack(const unsigned long long *reply, const uint32_t *pos, const uint8_t *dest, uint64_t m,
                               uint64_t layout, int n_ranks, const unsigned long long *n_rows_of, uint8_t *ranks,
                               uint32_t *rows, uint16_t *counts, char *left, char *right, hipStream_t s) {
  if (!m) return hipSuccess;
  if (n_ranks < 1 || n_ranks > 255) return hipErrorInvalidValue;
  k_route_unpack<<<grid_for(m), R_THREADS, 0, s>>>(reply, pos, dest, m, layout, n_ranks, n_rows_of, ranks, rows, counts,
                                                   left, right);
  return hipGetLastError();
}

hipError_t launch_route_verdict(const RouteSource &src, uint64_t m, int k, int nl, int nlo,
                                const unsigned long long *reply, const uint32_t *pos, const uint8_t *dest, uint64_t layout,
                                int n_ranks, const unsigned long long *n_rows_of, uint8_t *next_rank, uint32_t *next_row,
                                uint8_t *status, hipStream_t s) {
  if (!m) return hipSuccess;
  if (!shape_ok(k, nl, nlo, 1, n_ranks) || !src.links || !source_ok(src, m)) return hipErrorInvalidValue;
#define K_VERDICT(NLV, ...) k_route_verdict<NLV><<<grid_for(m), R_THREADS, 0, s>>>(__VA_ARGS__)
  ROUTE_SWITCH(K_VERDICT, src, m, k, nlo, reply, pos, dest, layout, n_ranks, n_rows_of, next_rank, next_row, status)
#undef K_VERDICT
  return hipGetLastError();
}

#undef ROUTE_SWITCH

hipError_t launch_route_rank0(const uint32_t *next, uint64_t n, uint8_t *next_rank, hipStream_t s) {
  if (!n) return hipSuccess;
  k_route_rank0<<<grid_for(n), R_THREADS, 0, s>>>(next, n, next_rank);
  return hipGetLastError();
}

}  // namespace mhm
