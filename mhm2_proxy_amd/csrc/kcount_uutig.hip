// The unitigs of the finished table from its de Bruijn links, on gfx950: the traversal of one contigging round
// (traverse_debruijn_graph, src/dbjg_traversal.cpp:165-289,301-307,404-407,539-541,569-596) at one rank, as list
// ranking over the link arrays of mhmkc_dbjg_links instead of a walk with a visited array. DESIGN.md §3.12.
//
// Every row has two ports, 2 * row + d (d: 0 LEFT, 1 RIGHT, in the row's stored orientation). A port is linked when
// its link is OK, enters another port than itself and that port's link leads back (the walker's get_next_step seen
// from both sides, dbjg_traversal.cpp:165-239); every other port is an end. Under linked ports the rows with two
// ACGT extensions form simple paths and simple cycles, each one uutig. A port's state is 32 bytes: the port travel
// has reached from it (or, once `done`, the end port), the rows passed on the way, the sum of their counts and the
// smallest key among them (its first word and its row; equal first words fall back to the rows' full keys). One
// pointer-jumping round doubles the reach of every port that is not done; a port that is done is read (32 coalesced
// bytes) and skipped. The two state buffers alternate as source and destination, so a round never reads what it writes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"
#include "kmer_ops.hpp"

namespace mhm {

namespace {

// 256 threads, no LDS, ~40 VGPRs: 8 waves per SIMD stay resident, which is what hides the dependent HBM reads
// (one 32-byte state per jump) of these kernels
constexpr int U_THREADS = 256;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
constexpr uint64_t PORT_MASK = (1ull << 40) - 1;
constexpr uint64_t DONE = 1ull << 63;
constexpr int ROUND_SHIFT = 48;

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

__device__ __forceinline__ bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// The mutual-link rule for port (i, d): false for an end; otherwise entry = the port travel enters and succ = the port
// it leaves the neighbour through. Every index read from memory is checked against n before it is used.
__device__ __forceinline__ bool port_link(const uint32_t *next, const uint8_t *status, uint64_t n, uint64_t i, uint32_t d,
                                          uint64_t &succ, uint64_t &entry) {
  const uint8_t st = status[d * n + i];
  if ((st & 0x7f) != MHMKC_LINK_OK) return false;
  const uint64_t j = next[d * n + i];
  if (j >= n) return false;
  const uint32_t e = d ^ (uint32_t)(st >> 7) ^ 1u;
  if (j == i && e == d) return false;  // a hairpin: the neighbour is the row's own reverse complement
  const uint8_t st2 = status[e * n + j];
  if ((st2 & 0x7f) != MHMKC_LINK_OK) return false;
  const uint32_t e2 = e ^ (uint32_t)(st2 >> 7) ^ 1u;
  if ((uint64_t)next[e * n + j] != i || e2 != d) return false;  // not mutual (rows that are their own reverse complement)
  entry = 2 * j + e;
  succ = 2 * j + (e ^ 1u);
  return true;
}

// Kmer::operator< (src/kmer.cpp:265-272) on (first word, row): the other words are read only when the first are equal
template <int NL>
__device__ __forceinline__ bool key_before(uint64_t aw, uint32_t ar, uint64_t bw, uint32_t br, const uint64_t *keys,
                                           uint64_t n, int nlo) {
  if (aw != bw) return aw < bw;
  if (NL == 1 || ar == br || ar >= n || br >= n) return false;
#pragma unroll
  for (int j = 1; j < NL; j++) {
    const uint64_t x = keys[(uint64_t)ar * nlo + j], y = keys[(uint64_t)br * nlo + j];
    if (x != y) return x < y;
  }
  return false;
}

// Stage 1, the port successor: the first state of every port (or of the listed ports). With cut != null the listed
// ports lie on cycles whose state in cut names the cycle's start (minrow): the start's port 1 and the port entering
// it become ends, which opens the cycle where the host walker's left walk closes it (dbjg_traversal.cpp:262-289).
__global__ __launch_bounds__(U_THREADS) void k_uutig_init(OutRows t, uint64_t n, int nlo, const uint32_t *next,
                                                           const uint8_t *status, const uint64_t *list, uint64_t n_items,
                                                           const UutigPort *cut, uint32_t round, UutigPort *st) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_items; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = list ? list[x] : x;
    if (p >= 2 * n) continue;
    const uint64_t i = p >> 1;
    uint64_t succ = 0, entry = 0;
    bool linked = port_link(next, status, n, i, (uint32_t)(p & 1), succ, entry);
    if (cut && linked) {
      const uint64_t cp = 2 * (uint64_t)cut[p].minrow + 1;
      if (p == cp || entry == cp) linked = false;
    }
    UutigPort a;
    a.sum = t.counts[i];
    a.minw0 = t.keys[i * (uint64_t)nlo];
    a.minrow = (uint32_t)i;
    a.dist = linked ? 1u : 0u;
    a.link = (linked ? succ : (p | DONE)) | (uint64_t)(round & 0xffu) << ROUND_SHIFT;
    st[p] = a;
  }
}

// Stage 2, one round of pointer jumping: src's state of [p, q) joined with its state of [q, ...). A port that was done
// by round - 1 is copied once, so that both buffers hold its last state, and is only read from then on.
template <int NL>
__global__ __launch_bounds__(U_THREADS) void k_uutig_jump(const UutigPort *src, UutigPort *dst, uint64_t n_ports,
                                                           const uint64_t *list, uint64_t n_items, const uint64_t *keys,
                                                           int nlo, uint32_t round, unsigned long long *active) {
  unsigned mine = 0;
  const uint64_t n = n_ports >> 1;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_items; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = list ? list[x] : x;
    if (p >= n_ports) continue;
    UutigPort a = src[p];
    if (a.link & DONE) {
      if (((a.link >> ROUND_SHIFT) & 0xffu) == ((round - 1) & 0xffu)) dst[p] = a;
      continue;
    }
    const uint64_t q = a.link & PORT_MASK;
    if (q >= n_ports) continue;
    const UutigPort b = src[q];
    a.dist += b.dist;
    a.sum += b.sum;
    if (key_before<NL>(b.minw0, b.minrow, a.minw0, a.minrow, keys, n, nlo)) {
      a.minw0 = b.minw0;
      a.minrow = b.minrow;
    }
    a.link = (b.link & (PORT_MASK | DONE)) | (uint64_t)(round & 0xffu) << ROUND_SHIFT;
    dst[p] = a;
    mine += (b.link & DONE) ? 0u : 1u;
  }
  // ports still on their way after this round, one atomic per wave
  for (int o = warpSize / 2; o > 0; o >>= 1) mine += __shfl_down(mine, o);
  if ((threadIdx.x & (warpSize - 1)) == 0 && mine) atomicAdd(active, (unsigned long long)mine);
}

// Stage 3: the ports that are not done when ranking stops lie on cycles
__global__ __launch_bounds__(U_THREADS) void k_uutig_active(const UutigPort *st, uint64_t n_ports, uint64_t *list,
                                                             uint64_t cap, unsigned long long *n_list) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_ports; p += (uint64_t)gridDim.x * blockDim.x) {
    if (st[p].link & DONE) continue;
    const unsigned long long at = atomicAdd(n_list, 1ull);
    if (at < cap) list[at] = p;
  }
}

// Stage 4a: every walkable row learns its component's start (kept in row_pos until k_uutig_place); the starts are
// collected (traverse_debruijn_graph starts one walk per component, dbjg_traversal.cpp:539-541)
template <int NL>
__global__ __launch_bounds__(U_THREADS) void k_uutig_starts(OutRows t, uint64_t n, int nlo, const UutigPort *st,
                                                             uint32_t *row_ctg, uint32_t *row_pos, uint8_t *row_rc,
                                                             uint32_t *starts, unsigned long long *n_starts) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    row_ctg[i] = NO_ROW;
    row_rc[i] = 0;
    if (!is_base(t.left[i]) || !is_base(t.right[i])) {
      row_pos[i] = 0;
      continue;
    }
    const UutigPort a = st[2 * i], b = st[2 * i + 1];
    const uint32_t s = key_before<NL>(b.minw0, b.minrow, a.minw0, a.minrow, t.keys, n, nlo) ? b.minrow : a.minrow;
    row_pos[i] = s;
    if ((uint64_t)s == i) {
      const unsigned long long at = atomicAdd(n_starts, 1ull);
      if (at < n) starts[at] = s;
    }
  }
}

__global__ __launch_bounds__(U_THREADS) void k_uutig_sort_word(const uint64_t *keys, uint64_t n, int nlo, int w,
                                                                const uint32_t *rows, uint64_t n_ctgs, uint64_t *word) {
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = rows[c];
    word[c] = r < n ? keys[r * nlo + w] : ~0ull;
  }
}

// Stage 4b: contig c is the component with the c-th smallest start (the id traverse_debruijn_graph assigns): its
// k-mers, its length for the scan of the offsets, and its depth, the start counted by both walks
// (dbjg_traversal.cpp:224) over len - k + 2 = m + 1
__global__ __launch_bounds__(U_THREADS) void k_uutig_ctgs(const uint32_t *sorted, uint64_t n_ctgs, uint64_t n, int k,
                                                           const UutigPort *st, uint32_t *row_ctg, uint32_t *n_kmers,
                                                           double *depths, uint64_t *lens) {
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    if (c == n_ctgs) {
      lens[c] = 0;
      continue;
    }
    const uint64_t s = sorted[c];
    if (s >= n) {
      n_kmers[c] = 0;
      depths[c] = 0;
      lens[c] = 0;
      continue;
    }
    const UutigPort a = st[2 * s], b = st[2 * s + 1];
    const uint64_t m = (uint64_t)a.dist + b.dist + 1;
    const uint64_t sum = a.sum + b.sum;  // each chain holds the start's count: the component's sum and the start once more
    n_kmers[c] = (uint32_t)m;
    depths[c] = (double)sum / (double)(m + 1);
    lens[c] = m + (uint64_t)k - 1;
    row_ctg[s] = (uint32_t)c;
  }
}

// Stage 5a: a row lies as its start does when their left chains end at the same port; its position is its distance
// from that end
__global__ __launch_bounds__(U_THREADS) void k_uutig_place(OutRows t, uint64_t n, const UutigPort *st, uint32_t *row_ctg,
                                                            uint32_t *row_pos, uint8_t *row_rc) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!is_base(t.left[i]) || !is_base(t.right[i])) continue;
    const uint64_t s = row_pos[i];
    if (s >= n) continue;
    const uint64_t end0 = st[2 * s].link & PORT_MASK;
    const UutigPort a = st[2 * i], b = st[2 * i + 1];
    const bool rc = (a.link & PORT_MASK) != end0;
    if (s != i) row_ctg[i] = row_ctg[s];  // (the starts' entries were written by k_uutig_ctgs and are not written here)
    row_pos[i] = rc ? b.dist : a.dist;
    row_rc[i] = rc ? 1 : 0;
  }
}

// Stage 5b: every row writes the first base of its k-mer in walk orientation, the last row of a contig all k
template <int NL>
__global__ __launch_bounds__(U_THREADS) void k_uutig_bases(const uint64_t *keys, uint64_t n, int k, int nlo,
                                                            const uint32_t *row_ctg, const uint32_t *row_pos,
                                                            const uint8_t *row_rc, const uint64_t *offsets,
                                                            const uint32_t *n_kmers, uint64_t n_ctgs, uint64_t n_bases,
                                                            char *seqs) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c = row_ctg[i];
    if (c >= n_ctgs) continue;
    const uint64_t pos = row_pos[i], m = n_kmers[c];
    if (pos >= m) continue;
    const int nb = pos + 1 == m ? k : 1;
    const uint64_t at = offsets[c] + pos;
    if (at + (uint64_t)nb > n_bases) continue;
    uint64_t w[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) w[j] = keys[i * (uint64_t)nlo + j];
    const bool rc = row_rc[i] != 0;
    for (int b = 0; b < nb; b++) {
      const int x = rc ? k - 1 - b : b;
      uint32_t code = 0;
#pragma unroll
      for (int j = 0; j < NL; j++)
        if (j == x >> 5) code = (uint32_t)(w[j] >> (2 * (31 - (x & 31)))) & 3u;
      if (rc) code = 3u - code;
      seqs[at + b] = (char)((0x54474341u >> (8 * code)) & 0xffu);
    }
  }
}

}  // namespace

hipError_t launch_uutig_init(const OutRows &t, uint64_t n, int nlo, const uint32_t *next, const uint8_t *status,
                             const uint64_t *list, uint64_t n_items, const UutigPort *cut, uint32_t round, UutigPort *st,
                             hipStream_t s) {
  if (!n || !n_items) return hipSuccess;
  if (n >= 0xffffffffull || nlo < 1) return hipErrorInvalidValue;
  k_uutig_init<<<grid_for(n_items), U_THREADS, 0, s>>>(t, n, nlo, next, status, list, n_items, cut, round, st);
  return hipGetLastError();
}

hipError_t launch_uutig_jump(const UutigPort *src, UutigPort *dst, uint64_t n, const uint64_t *list, uint64_t n_items,
                             const uint64_t *keys, int nl, int nlo, uint32_t round, unsigned long long *active,
                             hipStream_t s) {
  if (!n || !n_items) return hipSuccess;
  if (n >= 0xffffffffull || nlo < nl) return hipErrorInvalidValue;
  const unsigned g = grid_for(n_items);
  switch (nl) {
    case 1: k_uutig_jump<1><<<g, U_THREADS, 0, s>>>(src, dst, 2 * n, list, n_items, keys, nlo, round, active); break;
    case 2: k_uutig_jump<2><<<g, U_THREADS, 0, s>>>(src, dst, 2 * n, list, n_items, keys, nlo, round, active); break;
    case 3: k_uutig_jump<3><<<g, U_THREADS, 0, s>>>(src, dst, 2 * n, list, n_items, keys, nlo, round, active); break;
    case 4: k_uutig_jump<4><<<g, U_THREADS, 0, s>>>(src, dst, 2 * n, list, n_items, keys, nlo, round, active); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_uutig_active(const UutigPort *st, uint64_t n, uint64_t *list, uint64_t cap, unsigned long long *n_list,
                               hipStream_t s) {
  if (!n) return hipSuccess;
  k_uutig_active<<<grid_for(2 * n), U_THREADS, 0, s>>>(st, 2 * n, list, cap, n_list);
  return hipGetLastError();
}

hipError_t launch_uutig_starts(const OutRows &t, uint64_t n, int nl, int nlo, const UutigPort *st, uint32_t *row_ctg,
                               uint32_t *row_pos, uint8_t *row_rc, uint32_t *starts, unsigned long long *n_starts,
                               hipStream_t s) {
  if (!n) return hipSuccess;
  if (nlo < nl) return hipErrorInvalidValue;
  const unsigned g = grid_for(n);
  switch (nl) {
    case 1: k_uutig_starts<1><<<g, U_THREADS, 0, s>>>(t, n, nlo, st, row_ctg, row_pos, row_rc, starts, n_starts); break;
    case 2: k_uutig_starts<2><<<g, U_THREADS, 0, s>>>(t, n, nlo, st, row_ctg, row_pos, row_rc, starts, n_starts); break;
    case 3: k_uutig_starts<3><<<g, U_THREADS, 0, s>>>(t, n, nlo, st, row_ctg, row_pos, row_rc, starts, n_starts); break;
    case 4: k_uutig_starts<4><<<g, U_THREADS, 0, s>>>(t, n, nlo, st, row_ctg, row_pos, row_rc, starts, n_starts); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

static size_t uutig_sort_tmp(uint64_t n_ctgs) {
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)n_ctgs);
  (void)rocprim::exclusive_scan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0,
                                (size_t)(n_ctgs + 1), rocprim::plus<uint64_t>());
  return std::max(a, b);
}

size_t uutig_table_scratch_bytes(uint64_t n_ctgs) {
  const size_t a = (n_ctgs + 64) / 64 * 64;
  return a * (4 + 8 + 8 + 8) + uutig_sort_tmp(n_ctgs) + 512;
}

hipError_t launch_uutig_table(const OutRows &t, uint64_t n, int k, int nl, int nlo, const UutigPort *st, uint32_t *starts,
                              uint64_t n_ctgs, void *scratch, size_t scratch_bytes, uint32_t *row_ctg, uint32_t *n_kmers,
                              double *depths, uint64_t *offsets, hipStream_t s) {
  if (!n || nlo < nl || nl < 1 || nl > 4 || scratch_bytes < uutig_table_scratch_bytes(n_ctgs)) return hipErrorInvalidValue;
  const size_t a = (n_ctgs + 64) / 64 * 64;
  uint64_t *word = (uint64_t *)scratch, *word2 = word + a, *lens = word2 + a;
  uint32_t *rows2 = (uint32_t *)(lens + a);
  void *tmp = rows2 + a;
  size_t tb = scratch_bytes - a * 28;
  uint32_t *cur = starts, *alt = rows2;
  hipError_t e;
  if (n_ctgs) {
    // least significant word first, each pass stable: the starts end up in Kmer::operator< order
    for (int w = nl - 1; w >= 0; w--) {
      k_uutig_sort_word<<<grid_for(n_ctgs), U_THREADS, 0, s>>>(t.keys, n, nlo, w, cur, n_ctgs, word);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = rocprim::radix_sort_pairs(tmp, tb, word, word2, cur, alt, (size_t)n_ctgs, 0, 64, s)) != hipSuccess) return e;
      std::swap(cur, alt);
    }
    if (cur != starts &&
        (e = hipMemcpyAsync(starts, cur, n_ctgs * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess)
      return e;
  }
  k_uutig_ctgs<<<grid_for(n_ctgs + 1), U_THREADS, 0, s>>>(starts, n_ctgs, n, k, st, row_ctg, n_kmers, depths, lens);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return rocprim::exclusive_scan(tmp, tb, lens, offsets, (uint64_t)0, (size_t)(n_ctgs + 1), rocprim::plus<uint64_t>(), s);
}

hipError_t launch_uutig_place(const OutRows &t, uint64_t n, const UutigPort *st, uint32_t *row_ctg, uint32_t *row_pos,
                              uint8_t *row_rc, hipStream_t s) {
  if (!n) return hipSuccess;
  k_uutig_place<<<grid_for(n), U_THREADS, 0, s>>>(t, n, st, row_ctg, row_pos, row_rc);
  return hipGetLastError();
}

hipError_t launch_uutig_bases(const OutRows &t, uint64_t n, int k, int nl, int nlo, const uint32_t *row_ctg,
                              const uint32_t *row_pos, const uint8_t *row_rc, const uint64_t *offsets,
                              const uint32_t *n_kmers, uint64_t n_ctgs, uint64_t n_bases, char *seqs, hipStream_t s) {
  if (!n || !n_ctgs) return hipSuccess;
  if (nlo < nl || k / 32 + 1 != nl || k % 32 == 0) return hipErrorInvalidValue;
  const unsigned g = grid_for(n);
  switch (nl) {
    case 1: k_uutig_bases<1><<<g, U_THREADS, 0, s>>>(t.keys, n, k, nlo, row_ctg, row_pos, row_rc, offsets, n_kmers, n_ctgs, n_bases, seqs); break;
    case 2: k_uutig_bases<2><<<g, U_THREADS, 0, s>>>(t.keys, n, k, nlo, row_ctg, row_pos, row_rc, offsets, n_kmers, n_ctgs, n_bases, seqs); break;
    case 3: k_uutig_bases<3><<<g, U_THREADS, 0, s>>>(t.keys, n, k, nlo, row_ctg, row_pos, row_rc, offsets, n_kmers, n_ctgs, n_bases, seqs); break;
    case 4: k_uutig_bases<4><<<g, U_THREADS, 0, s>>>(t.keys, n, k, nlo, row_ctg, row_pos, row_rc, offsets, n_kmers, n_ctgs, n_bases, seqs); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mhm
