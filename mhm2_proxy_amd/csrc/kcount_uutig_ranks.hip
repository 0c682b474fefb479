// The uutigs of a table that lies on several ranks (mhmkc_uutigs_ranks; traverse_debruijn_graph at rank_n() > 1,
// src/dbjg_traversal.cpp:291-335,517-567,569-596), the replicated build of DESIGN.md §3.12b: every rank receives the other
// ranks' rows, ranks the union with the kernels of kcount_uutig.hip, and keeps what is its own. The kernels here are that
// last step. A contig of the union belongs to the rank that holds its start row; the union's rows lie in rank order, rank
// r's at [base[r], base[r + 1]), so the owner is a search in base. The union's contigs are in start-key order, so a stable
// sort of them by owner puts every rank's contigs together, in start-key order, after those of the lower ranks: a contig's
// place in that order is its global id (reduce_prefix, dbjg_traversal.cpp:581-587), and a rank's contigs are one span of it.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"

namespace mhm {

namespace {

// 256 threads, grid-stride, no LDS, no scratch (the registers of each kernel: DESIGN.md §3.12b)
constexpr int R_THREADS = 256;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

// the rank whose rows hold union row s: the last r with base[r] <= s (base[0] = 0; ranks without rows are skipped)
__device__ __forceinline__ uint32_t owner_of(const uint64_t *base, int g, uint64_t s) {
  int lo = 0, hi = g;  // base[lo] <= s < base[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= s) lo = mid;
    else hi = mid;
  }
  return (uint32_t)lo;
}

// Stage 1: the owner of every contig of the union, as the sort key, and the contig as its value
__global__ __launch_bounds__(R_THREADS) void k_ur_owner(const uint32_t *starts, uint64_t n_ctgs, const uint64_t *base, int g,
                                                         uint32_t *owner, uint32_t *ctg) {
  const uint64_t n_rows = base[g];
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = starts[c];
    // (a start outside the union cannot come from k_uutig_starts; it goes to the last rank + 1, which nobody keeps)
    owner[c] = s < n_rows ? owner_of(base, g, s) : (uint32_t)g;
    ctg[c] = (uint32_t)c;
  }
}

// Stage 2: place p of the sorted order holds contig order[p] of rank owner[p]: the contig's global id is p, and the first
// place of every rank that has one is where the owner changes
__global__ __launch_bounds__(R_THREADS) void k_ur_ids(const uint32_t *owner, const uint32_t *order, uint64_t n_ctgs, int g,
                                                       uint32_t *gid, uint64_t *first) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_ctgs; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = owner[p], c = order[p];
    if (c < n_ctgs) gid[c] = (uint32_t)p;
    if (r <= (uint32_t)g && (p == 0 || owner[p - 1] != r)) first[r] = p;
  }
}

// Stage 3: this rank's contigs are places [first_me, first_me + n_mine): their k-mers, depths and lengths
__global__ __launch_bounds__(R_THREADS) void k_ur_take(const uint32_t *order, uint64_t first_me, uint64_t n_mine,
                                                        uint64_t n_ctgs, const uint64_t *uoff, const double *udepths,
                                                        const uint32_t *unk, uint32_t *n_kmers, double *depths,
                                                        uint64_t *lens) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= n_mine; j += (uint64_t)gridDim.x * blockDim.x) {
    if (j == n_mine) {
      lens[j] = 0;
      continue;
    }
    const uint64_t c = first_me + j < n_ctgs ? order[first_me + j] : n_ctgs;
    if (c >= n_ctgs) {
      n_kmers[j] = 0;
      depths[j] = 0;
      lens[j] = 0;
      continue;
    }
    n_kmers[j] = unk[c];
    depths[j] = udepths[c];
    lens[j] = uoff[c + 1] - uoff[c];
  }
}

// Stage 4: their bases, one per thread: base x of this rank lies in its contig j with offsets[j] <= x < offsets[j + 1]
__global__ __launch_bounds__(R_THREADS) void k_ur_seqs(const uint32_t *order, uint64_t first_me, uint64_t n_mine,
                                                        uint64_t n_ctgs, const uint64_t *uoff, const char *useq,
                                                        uint64_t u_bases, const uint64_t *offsets, uint64_t n_bases,
                                                        char *seqs) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_bases; x += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo = 0, hi = n_mine;  // offsets[lo] <= x < offsets[hi]
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (offsets[mid] <= x) lo = mid;
      else hi = mid;
    }
    const uint64_t c = first_me + lo < n_ctgs ? order[first_me + lo] : n_ctgs;
    if (c >= n_ctgs) continue;
    const uint64_t at = uoff[c] + (x - offsets[lo]);
    if (at < u_bases && at < uoff[c + 1]) seqs[x] = useq[at];
  }
}

// Stage 5: this rank's rows are rows [base_me, base_me + n_me) of the union; a row's contig becomes its global id
__global__ __launch_bounds__(R_THREADS) void k_ur_rows(const uint32_t *urow_ctg, const uint32_t *urow_pos,
                                                        const uint8_t *urow_rc, uint64_t n_rows, uint64_t base_me,
                                                        uint64_t n_me, const uint32_t *gid, uint64_t n_ctgs,
                                                        uint32_t *row_ctg, uint32_t *row_pos, uint8_t *row_rc) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_me; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t u = base_me + i;
    if (u >= n_rows) continue;
    const uint64_t c = urow_ctg[u];
    const bool in = c < n_ctgs;
    row_ctg[i] = in ? gid[c] : NO_ROW;
    row_pos[i] = in ? urow_pos[u] : 0u;
    row_rc[i] = in ? urow_rc[u] : (uint8_t)0;
  }
}

size_t ranks_sort_tmp(uint64_t n_ctgs, uint64_t n_mine) {
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)std::max<uint64_t>(n_ctgs, 1), 0, 8);
  (void)rocprim::exclusive_scan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0,
                                (size_t)(n_mine + 1), rocprim::plus<uint64_t>());
  return std::max(a, b);
}

size_t ranks_al(uint64_t n) { return (size_t)((n + 64) / 64 * 64); }

}  // namespace

size_t uutig_ranks_scratch_bytes(uint64_t n_ctgs) {
  // owner, ctg, owner sorted, order, gid (u32 each), lens (u64), the sort's and the scan's scratch (a rank has at most all
  // the contigs)
  return ranks_al(n_ctgs) * (5 * 4 + 8) + ranks_sort_tmp(n_ctgs, n_ctgs) + 512;
}

hipError_t launch_uutig_ranks_ids(const uint32_t *starts, uint64_t n_ctgs, const uint64_t *base, int g, void *scratch,
                                  size_t scratch_bytes, const uint32_t **order, const uint32_t **gid, uint64_t *first,
                                  hipStream_t s) {
  if (g < 1 || g > 255 || scratch_bytes < uutig_ranks_scratch_bytes(n_ctgs)) return hipErrorInvalidValue;
  const size_t a = ranks_al(n_ctgs);
  uint32_t *owner = (uint32_t *)scratch, *ctg = owner + a, *owner2 = ctg + a, *ord = owner2 + a, *id = ord + a;
  void *tmp = (char *)scratch + a * 28;
  size_t tb = scratch_bytes - a * 28;
  *order = ord;
  *gid = id;
  hipError_t e;
  if ((e = hipMemsetAsync(first, 0xFF, 8 * (size_t)(g + 1), s)) != hipSuccess) return e;
  if (!n_ctgs) return hipSuccess;
  k_ur_owner<<<grid_for(n_ctgs), R_THREADS, 0, s>>>(starts, n_ctgs, base, g, owner, ctg);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // one stable pass over the 8 bits of the owner: within a rank the contigs keep their start-key order
  if ((e = rocprim::radix_sort_pairs(tmp, tb, owner, owner2, ctg, ord, (size_t)n_ctgs, 0, 8, s)) != hipSuccess) return e;
  k_ur_ids<<<grid_for(n_ctgs), R_THREADS, 0, s>>>(owner2, ord, n_ctgs, g, id, first);
  return hipGetLastError();
}

hipError_t launch_uutig_ranks_take(const uint32_t *order, uint64_t first_me, uint64_t n_mine, uint64_t n_ctgs,
                                   const uint64_t *uoff, const double *udepths, const uint32_t *unk, void *scratch,
                                   size_t scratch_bytes, uint32_t *n_kmers, double *depths, uint64_t *offsets,
                                   hipStream_t s) {
  if (n_mine > n_ctgs || first_me + n_mine > n_ctgs || scratch_bytes < uutig_ranks_scratch_bytes(n_ctgs))
    return hipErrorInvalidValue;
  const size_t a = ranks_al(n_ctgs);
  uint64_t *lens = (uint64_t *)((char *)scratch + a * 20);
  void *tmp = (char *)scratch + a * 28;
  size_t tb = scratch_bytes - a * 28;
  k_ur_take<<<grid_for(n_mine + 1), R_THREADS, 0, s>>>(order, first_me, n_mine, n_ctgs, uoff, udepths, unk, n_kmers, depths,
                                                        lens);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return rocprim::exclusive_scan(tmp, tb, lens, offsets, (uint64_t)0, (size_t)(n_mine + 1), rocprim::plus<uint64_t>(), s);
}

hipError_t launch_uutig_ranks_seqs(const uint32_t *order, uint64_t first_me, uint64_t n_mine, uint64_t n_ctgs,
                                   const uint64_t *uoff, const char *useq, uint64_t u_bases, const uint64_t *offsets,
                                   uint64_t n_bases, char *seqs, hipStream_t s) {
  if (!n_bases || !n_mine) return hipSuccess;
  if (first_me + n_mine > n_ctgs || n_bases > u_bases) return hipErrorInvalidValue;
  k_ur_seqs<<<grid_for(n_bases), R_THREADS, 0, s>>>(order, first_me, n_mine, n_ctgs, uoff, useq, u_bases, offsets, n_bases,
                                                     seqs);
  return hipGetLastError();
}

hipError_t launch_uutig_ranks_rows(const uint32_t *urow_ctg, const uint32_t *urow_pos, const uint8_t *urow_rc,
                                   uint64_t n_rows, uint64_t base_me, uint64_t n_me, const uint32_t *gid, uint64_t n_ctgs,
                                   uint32_t *row_ctg, uint32_t *row_pos, uint8_t *row_rc, hipStream_t s) {
  if (!n_me) return hipSuccess;
  if (base_me + n_me > n_rows) return hipErrorInvalidValue;
  k_ur_rows<<<grid_for(n_me), R_THREADS, 0, s>>>(urow_ctg, urow_pos, urow_rc, n_rows, base_me, n_me, gid, n_ctgs, row_ctg,
                                                 row_pos, row_rc);
  return hipGetLastError();
}

}  // namespace mhm
