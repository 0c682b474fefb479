// Contigs that are already on the device, made into the contig pass's input on gfx950.
//
// Reference: a contigging round hands its uutigs to the next k as `ctgs` (src/contigging.cpp:93-158), and
// add_ctg_kmers (src/kcount/kcount.cpp:100-138) gives every contig of length >= k+2 to process_seq with
// Contig::get_uint16_t_depth() (src/contigs.hpp:65). Here the uutigs lie in HBM as ASCII bases, u64 offsets and f64
// depths (kcount_uutig.hip); the contig pass (kcount_ctg.hip) reads PackedRead bytes, byte offsets, a prefix of the
// counted windows and u16 depths. Three steps turn the one into the other, appended to what the round already holds:
//   k_ctgin_contigs  one lane per contig: length, monotonicity, counted windows, depth, rebased offset;
//   exclusive_scan   the window prefix, started from the round's windows so far (rocPRIM);
//   k_ctg_pack       the bases, 16 per lane and turn.
// Whatever is wrong with the input is named in a mailbox (CtgInBox) that the host reads once, after the three.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "kcount_launch.hpp"
#include "kmer_ops.hpp"

namespace mhm {

namespace {

constexpr int G_THREADS = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__global__ void k_ctgin_begin(CtgInBox *box) {
  box->bad_pos = box->bad_off = box->bad_depth = ~0ull;
  box->windows = box->first_off = box->last_off = 0;
}

// cnt[i] = the counted windows of contig i (add_ctg_kmers skips contigs shorter than k + 2; the first and the last
// k-mer of a contig have no extension on one side and are not counted), cnt[n] = 0: the scan's last output is the total.
__global__ __launch_bounds__(G_THREADS) void k_ctgin_contigs(const uint64_t *offs, const void *depths, bool depth_f64,
                                                              uint64_t n, uint64_t k, uint64_t b0, uint64_t *out_offs,
                                                              unsigned long long *cnt, uint16_t *out_depth, CtgInBox *box) {
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0) {
    box->first_off = offs[0];
    box->last_off = offs[n];
    out_offs[0] = b0;
    cnt[n] = 0;
  }
  for (uint64_t i = t0; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o0 = offs[i], o1 = offs[i + 1];
    if (o1 < o0) atomicMin(&box->bad_off, (unsigned long long)i);
    const uint64_t L = o1 < o0 ? 0 : o1 - o0;
    cnt[i] = L >= k + 2 ? L - k - 1 : 0;
    out_offs[i + 1] = b0 + o1;
    uint16_t d;
    if (depth_f64) {
      bool ok;
      d = ctg_depth_u16(((const double *)depths)[i], &ok);
      if (!ok) atomicMin(&box->bad_depth, (unsigned long long)i);
    } else {
      d = ((const uint16_t *)depths)[i];
    }
    out_depth[i] = d;
  }
}

__global__ void k_ctgin_end(const uint64_t *win_total, CtgInBox *box) { box->windows = *win_total; }

__device__ __forceinline__ void pack_note_bad(const uint32_t bad[4], uint64_t p, unsigned long long *bad_pos) {
#pragma unroll
  for (int w = 0; w < 4; w++)
    if (bad[w]) {  // the lowest flagged lane of the first flagged word: little-endian, the first such byte
      atomicMin(bad_pos, (unsigned long long)(p + 4 * w + ((__ffs(bad[w]) - 1) >> 3)));
      return;
    }
}

// ASCII -> PackedRead bytes (ctg_pack4). The destination decides the split: up to 15 head bytes bring it to a 16-byte
// boundary, then every lane loads 16 bytes (at whatever address the source then has: global loads need no alignment
// on gfx950, and the compiler emits one global_load_dwordx4 for the copy below), converts them in four dwords and stores
// 16 aligned bytes; up to 15 tail bytes are left. Head and tail are one byte per lane of the first workgroup.
__global__ __launch_bounds__(G_THREADS) void k_ctg_pack(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                         uint64_t n, unsigned long long *bad_pos) {
  const uint64_t head = min((uint64_t)((16 - ((uintptr_t)dst & 15)) & 15), n);
  const uint64_t nvec = (n - head) >> 4;
  const uint64_t tail0 = head + (nvec << 4);
  if (blockIdx.x == 0 && threadIdx.x < 32) {
    const bool is_head = threadIdx.x < 16;
    const uint64_t i = is_head ? threadIdx.x : tail0 + (threadIdx.x - 16);
    if (is_head ? i < head : i < n) {
      uint32_t bad;
      const uint32_t o = ctg_pack4(src[i], &bad);
      if (bad & 0x80u) atomicMin(bad_pos, (unsigned long long)i);
      dst[i] = (uint8_t)o;
    }
  }
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = head + (v << 4);
    u32x4 x;
    __builtin_memcpy(&x, src + p, 16);
    uint32_t bad[4];
    u32x4 o;
    o.x = ctg_pack4(x.x, &bad[0]);
    o.y = ctg_pack4(x.y, &bad[1]);
    o.z = ctg_pack4(x.z, &bad[2]);
    o.w = ctg_pack4(x.w, &bad[3]);
    if (bad[0] | bad[1] | bad[2] | bad[3]) pack_note_bad(bad, p, bad_pos);
    *(u32x4 *)(dst + p) = o;
  }
}

size_t scan_tmp_bytes(uint64_t n_items) {
  size_t a = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull,
                                (size_t)n_items, rocprim::plus<unsigned long long>());
  return a;
}

}  // namespace

size_t ctgin_tmp_bytes(uint64_t n_ctgs) { return align256((n_ctgs + 1) * 8) + align256(scan_tmp_bytes(n_ctgs + 1)); }

hipError_t launch_ctgin(const char *seqs, const uint64_t *offs, const void *depths, bool depth_f64, uint64_t n_ctgs,
                        uint64_t n_bases, int k, uint64_t b0, uint64_t w0, uint8_t *out_bytes, uint64_t *out_offs,
                        uint64_t *out_win, uint16_t *out_depth, void *tmp, size_t tmp_bytes, CtgInBox *box, hipStream_t s) {
  if (tmp_bytes < ctgin_tmp_bytes(n_ctgs)) return hipErrorInvalidValue;
  hipError_t e;
  k_ctgin_begin<<<1, 1, 0, s>>>(box);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  unsigned long long *cnt = (unsigned long long *)tmp;
  const unsigned cg = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(4096, (n_ctgs + G_THREADS - 1) / G_THREADS));
  k_ctgin_contigs<<<cg, G_THREADS, 0, s>>>(offs, depths, depth_f64, n_ctgs, (uint64_t)k, b0, out_offs, cnt, out_depth, box);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t sb = tmp_bytes - align256((n_ctgs + 1) * 8);
  // out_win[i] = w0 + the windows of the batch's contigs before i; out_win[n_ctgs] = the round's windows with the batch
  if ((e = rocprim::exclusive_scan((char *)tmp + align256((n_ctgs + 1) * 8), sb, cnt, (unsigned long long *)out_win,
                                   (unsigned long long)w0, (size_t)(n_ctgs + 1), rocprim::plus<unsigned long long>(), s)) !=
      hipSuccess)
    return e;
  k_ctgin_end<<<1, 1, 0, s>>>(out_win + n_ctgs, box);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (n_bases) {
    // two 16-byte vectors per lane at the full grid: enough loads in flight per CU, few enough workgroups to launch
    const uint64_t want = ((n_bases >> 4) + 2 * G_THREADS - 1) / (2 * G_THREADS);
    uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(want, 16384));
    if (ctg_pack_grid_cap && ctg_pack_grid_cap < g) g = ctg_pack_grid_cap;
    k_ctg_pack<<<(unsigned)g, G_THREADS, 0, s>>>((const uint8_t *)seqs, out_bytes, n_bases, &box->bad_pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mhm
