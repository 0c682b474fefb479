// The contigs of several ranks gathered on the device, on gfx950: the multi-rank contig pass's input
// when a rank of the round holds its contigs in HBM (mhmkc_add_ctgs_device, mhmkc_add_ctgs_from).
//
// Reference: add_ctg_kmers (src/kcount/kcount.cpp:100-138) runs on every rank over that rank's contigs and the supermers
// reach the k-mers' owners; here every rank extracts the contigs of all ranks and keeps its range, so the contigs are
// gathered, in rank order. A rank's contigs lie in the contig pass's layout (PackedRead bytes, byte offsets, u16 depths;
// kcount_ctgin.hip). They cross the wire as
//   u32 lengths       k_ctgx_lens   one lane per contig;
//   u16 depths        as they are;
//   bases as nibbles  k_ctgx_pack   16 bytes per lane and turn into 8 (ctg_nib8; a contig byte takes ten values),
// and are put together on the receiving rank by
//   k_ctgx_windows    one lane per gathered contig: its length as u64 and its counted windows;
//   exclusive_scan    twice (rocPRIM): the byte offsets and the window prefix of the gathered set;
//   k_ctgx_check      the peers' lengths against the sizes they announced, into the mailbox (CtgxBox);
//   k_expand_nibbles  (kcount_kernels.hip) every rank's nibbles to their place, launched by the host per rank.
// Lengths from a peer are data: they are summed and compared, never used as an address before the host has read the
// mailbox, and the expansion is placed by the announced sizes alone.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "kcount_launch.hpp"
#include "kmer_ops.hpp"

namespace mhm {

namespace {

constexpr int X_THREADS = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

unsigned capped_grid(uint64_t want) {
  uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(want, 16384));
  if (ctgx_grid_cap && ctgx_grid_cap < g) g = ctgx_grid_cap;
  return (unsigned)g;
}

__global__ void k_ctgx_begin(CtgxBox *box) {
  box->bad_rank = box->long_ctg = ~0ull;
  box->windows = 0;
}

// lens[i] = the bytes of contig i of this rank; a length that does not fit is named in the mailbox
__global__ __launch_bounds__(X_THREADS) void k_ctgx_lens(const uint64_t *__restrict__ offs, uint64_t n,
                                                          uint32_t *__restrict__ lens, CtgxBox *box) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t L = offs[i + 1] - offs[i];
    if (L > 0xffffffffull) atomicMin(&box->long_ctg, (unsigned long long)i);
    lens[i] = (uint32_t)L;
  }
}

// PackedRead bytes -> nibbles (ctg_nib8). src and dst are the starts of their buffers (16- and 8-byte aligned): every
// lane loads one dwordx4 and stores one dwordx2. The last n & 15 bytes go one pair per lane of the first workgroup; the
// high half of an odd last byte is zero.
__global__ __launch_bounds__(X_THREADS) void k_ctgx_pack(const uint8_t *__restrict__ src, uint64_t n,
                                                          uint8_t *__restrict__ dst) {
  const uint64_t nvec = n >> 4;
  const uint64_t tail0 = nvec << 4;
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const uint64_t i = tail0 + 2 * (uint64_t)threadIdx.x;
    if (i < n) {
      const uint32_t lo = src[i] & 15u;
      const uint32_t hi = i + 1 < n ? src[i + 1] & 15u : 0u;
      dst[i >> 1] = (uint8_t)(lo | (hi << 4));
    }
  }
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (uint64_t)gridDim.x * blockDim.x) {
    const u32x4 x = *(const u32x4 *)(src + (v << 4));
    u32x2 o;
    o.x = ctg_nib8(x.x, x.y);
    o.y = ctg_nib8(x.z, x.w);
    *(u32x2 *)(dst + (v << 3)) = o;
  }
}

// len64[i] = lens[i], cnt[i] = the counted windows of a contig of that length (add_ctg_kmers skips contigs shorter than
// k + 2; the first and the last k-mer are not counted), both 0 at i = n: the scans' last outputs are the totals.
__global__ __launch_bounds__(X_THREADS) void k_ctgx_windows(const uint32_t *__restrict__ lens, uint64_t n, uint64_t k,
                                                             unsigned long long *__restrict__ len64,
                                                             unsigned long long *__restrict__ cnt) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t L = i < n ? lens[i] : 0;
    len64[i] = L;
    cnt[i] = L >= k + 2 ? L - k - 1 : 0;
  }
}

// tab = [first contig of rank r | first byte of rank r], r = 0..g, from the sizes the ranks announced. Rank r's
// lengths must sum to its bytes: offs[first contig of r + 1] - offs[first contig of r]. The lowest rank that fails is
// named; the window total goes to the mailbox for the host to compare.
__global__ void k_ctgx_check(const uint64_t *__restrict__ offs, const uint64_t *__restrict__ win,
                             const uint64_t *__restrict__ tab, int g, uint64_t n, CtgxBox *box) {
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r == 0) box->windows = win[n];
  if (r >= g) return;
  const uint64_t c0 = tab[r], c1 = tab[r + 1];
  const uint64_t b0 = tab[g + 1 + r], b1 = tab[g + 1 + r + 1];
  if (c0 > c1 || c1 > n || offs[c1] - offs[c0] != b1 - b0 || offs[c0] != b0) atomicMin(&box->bad_rank, (unsigned long long)r);
}

size_t scan_tmp_bytes(uint64_t n_items) {
  size_t a = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull,
                                (size_t)n_items, rocprim::plus<unsigned long long>());
  return a;
}

}  // namespace

hipError_t launch_ctgx_begin(CtgxBox *box, hipStream_t s) {
  k_ctgx_begin<<<1, 1, 0, s>>>(box);
  return hipGetLastError();
}

hipError_t launch_ctgx_pack(const uint64_t *offs, uint64_t n_ctgs, const uint8_t *bytes, uint64_t n_bytes, uint32_t *lens,
                            uint8_t *nib, CtgxBox *box, hipStream_t s) {
  hipError_t e;
  if (n_ctgs) {
    k_ctgx_lens<<<capped_grid(std::min<uint64_t>(4096, (n_ctgs + X_THREADS - 1) / X_THREADS)), X_THREADS, 0, s>>>(
        offs, n_ctgs, lens, box);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_bytes) {
    if (((uintptr_t)bytes & 15) || ((uintptr_t)nib & 7)) return hipErrorInvalidValue;
    // two vectors per lane at the full grid, as k_ctg_pack
    k_ctgx_pack<<<capped_grid(((n_bytes >> 4) + 2 * X_THREADS - 1) / (2 * X_THREADS)), X_THREADS, 0, s>>>(bytes, n_bytes, nib);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

size_t ctgx_tmp_bytes(uint64_t n_all) { return 2 * align256((n_all + 1) * 8) + align256(scan_tmp_bytes(n_all + 1)); }

hipError_t launch_ctgx_assemble(const uint32_t *lens, uint64_t n_all, int k, const uint64_t *tab, int g, uint64_t *offs,
                                uint64_t *win, void *tmp, size_t tmp_bytes, CtgxBox *box, hipStream_t s) {
  if (tmp_bytes < ctgx_tmp_bytes(n_all) || g < 1) return hipErrorInvalidValue;
  hipError_t e;
  const size_t plane = align256((n_all + 1) * 8);
  unsigned long long *len64 = (unsigned long long *)tmp;
  unsigned long long *cnt = (unsigned long long *)((char *)tmp + plane);
  void *stmp = (char *)tmp + 2 * plane;
  size_t sb = tmp_bytes - 2 * plane;
  k_ctgx_windows<<<capped_grid(std::min<uint64_t>(4096, (n_all + 1 + X_THREADS - 1) / X_THREADS)), X_THREADS, 0, s>>>(
      lens, n_all, (uint64_t)k, len64, cnt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = rocprim::exclusive_scan(stmp, sb, len64, (unsigned long long *)offs, 0ull, (size_t)(n_all + 1),
                                   rocprim::plus<unsigned long long>(), s)) != hipSuccess ||
      (e = rocprim::exclusive_scan(stmp, sb, cnt, (unsigned long long *)win, 0ull, (size_t)(n_all + 1),
                                   rocprim::plus<unsigned long long>(), s)) != hipSuccess)
    return e;
  k_ctgx_check<<<(unsigned)((g + X_THREADS - 1) / X_THREADS), X_THREADS, 0, s>>>(offs, win, tab, g, n_all, box);
  return hipGetLastError();
}

}  // namespace mhm
