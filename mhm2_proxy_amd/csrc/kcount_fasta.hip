// What the reference does with its Contigs at the end of every round, on device-resident contigs:
// Contigs::print_stats (src/contigs.cpp:92-164) and the text of Contigs::dump_contigs (src/contigs.cpp:166-180).
//
// The contigs come as mhmkc_add_ctgs_device takes them: ASCII bases back to back, n_ctgs + 1 u64 offsets, one double depth
// per contig. Nothing here trusts an offset it read: the table kernels check that the offsets start at 0 and never fall,
// the host reads their verdict before any kernel that follows an offset into the bases runs, and those kernels still
// compare every index with the array's size before they use it.
//
// Statistics. k_fa_stats takes the contig table in chunks of FA_CHUNK contigs, whatever the grid: a chunk's depths are
// added in one fixed order (four per thread in index order, then a tree over the 256 threads), the chunks' sums are added
// in chunk order by the host, so tot_depth depends on the inputs alone. The integer figures are sums and a maximum, which
// no order changes. k_fa_ns counts the 'N' bytes of the counted contigs, 16 bytes per lane. N50 / L50: the counted
// lengths (u32; 0 for a contig that is not counted) sorted in descending order, their running sums, and the one place
// where the running sum first reaches half of the total.
//
// Text. Per contig the record's length (0 when it is filtered out), an exclusive scan for the records' places, then
// k_fa_copy writes the text in aligned 16-byte units of the destination (a unit inside one contig's bases is one shifted
// pair of aligned 16-byte loads and one 16-byte store; a unit that touches a record's edge is put together byte by byte,
// with zeros where a header lies), and k_fa_headers writes the headers and the closing newlines over those zeros.
// to_string(double) is "%f": the depth times 10^6 as a 73-bit integer m 10^6 2^-s, shifted and rounded to nearest, ties
// to even, in integers (fa_micro).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"

namespace mhm {

namespace {

constexpr int FA_THREADS = 256;
constexpr uint64_t FA_CHUNK = FASTA_STATS_CHUNK;  // contigs per chunk of k_fa_stats: 4 per thread

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

// the first offending contig c is kept as ~c under atomicMax (0: none)
__device__ __forceinline__ void fa_flag(unsigned long long *slot, uint64_t c) { atomicMax(slot, ~(unsigned long long)c); }

template <class T, class Op>
__device__ __forceinline__ T fa_block_reduce(T v, T *lds, Op op) {
  const int t = threadIdx.x;
  __syncthreads();
  lds[t] = v;
  __syncthreads();
  for (int w = FA_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) lds[t] = op(lds[t], lds[t + w]);
    __syncthreads();
  }
  return lds[0];
}

struct FaAddU {
  __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; }
};
struct FaMaxU {
  __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; }
};
struct FaAddD {
  __device__ double operator()(double a, double b) const { return a + b; }
};

// One pass over the contig table: length, filter, class sums, maximum, depth; lens[c] for the N50 sort
__global__ __launch_bounds__(FA_THREADS) void k_fa_stats(const uint64_t *offs, const double *depths, uint64_t n_ctgs,
                                                          uint32_t min_len, uint32_t *lens, double *partial,
                                                          CtgStatsBox *box) {
  __shared__ unsigned long long lds_u[FA_THREADS];
  __shared__ double lds_d[FA_THREADS];
  const uint64_t n_chunks = (n_ctgs + FA_CHUNK - 1) / FA_CHUNK;
  const int t = threadIdx.x;
  if (blockIdx.x == 0 && t == 0) {
    if (offs[0] != 0) fa_flag(&box->bad_off, 0);
    box->n_bases = offs[n_ctgs];
  }
  for (uint64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    unsigned long long cnt = 0, tot = 0, mx = 0, cls[5] = {0, 0, 0, 0, 0};
    double dsum = 0;
    for (int j = 0; j < 4; j++) {
      const uint64_t c = ch * FA_CHUNK + (uint64_t)j * FA_THREADS + t;
      if (c >= n_ctgs) continue;
      const uint64_t a = offs[c], b = offs[c + 1];
      if (b < a) {
        fa_flag(&box->bad_off, c);
        lens[c] = 0;
        continue;
      }
      const uint64_t len = b - a;
      const bool counted = len >= min_len;
      if (counted && len > 0xFFFFFFFFull) fa_flag(&box->bad_len, c);
      lens[c] = counted ? (uint32_t)len : 0u;
      if (!counted) continue;
      cnt++;
      tot += len;
      mx = len > mx ? len : mx;
      cls[0] += len >= 1000 ? len : 0;
      cls[1] += len >= 5000 ? len : 0;
      cls[2] += len >= 10000 ? len : 0;
      cls[3] += len >= 25000 ? len : 0;
      cls[4] += len >= 50000 ? len : 0;
      dsum += depths[c];
    }
    const double d = fa_block_reduce(dsum, lds_d, FaAddD());
    if (t == 0) partial[ch] = d;
    cnt = fa_block_reduce(cnt, lds_u, FaAddU());
    tot = fa_block_reduce(tot, lds_u, FaAddU());
    mx = fa_block_reduce(mx, lds_u, FaMaxU());
    for (int i = 0; i < 5; i++) cls[i] = fa_block_reduce(cls[i], lds_u, FaAddU());
    if (t == 0 && cnt) {
      atomicAdd(&box->n_ctgs, cnt);
      atomicAdd(&box->tot_len, tot);
      atomicMax(&box->max_len, mx);
      for (int i = 0; i < 5; i++)
        if (cls[i]) atomicAdd(&box->len_sums[i], cls[i]);
    }
  }
}

// the largest c in [0, n) with off[c] <= p, given off[0] <= p (off: n + 1 entries)
__device__ __forceinline__ uint64_t fa_find(const uint64_t *off, uint64_t n, uint64_t p) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t fa_word(const uint4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// One pass over the bases: the 'N' bytes of the counted contigs. A lane takes one aligned 16-byte unit of the array
// (the first and the last may hold bytes outside it, which are skipped) and finds the contig of its first byte in the
// offsets; with min_len <= 1 every byte of the array lies in a counted contig and no offset is read.
__global__ __launch_bounds__(FA_THREADS) void k_fa_ns(const char *seqs, const uint64_t *offs, uint64_t n_ctgs,
                                                       uint64_t n_bases, uint32_t min_len, CtgStatsBox *box) {
  __shared__ unsigned long long lds_u[FA_THREADS];
  const uint64_t mis = (uint64_t)(uintptr_t)seqs & 15;
  const uint4 *units = (const uint4 *)(seqs - mis);
  const uint64_t n_units = (n_bases + mis + 15) / 16;
  unsigned long long ns = 0;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 v = units[u];
    const uint64_t first = u * 16 < mis ? 0 : u * 16 - mis;  // the unit's first byte inside the array
    uint64_t c = 0, end = n_bases;
    bool ok = true;
    if (min_len > 1) {
      c = fa_find(offs, n_ctgs, first);
      const uint64_t a = offs[c];
      end = offs[c + 1];
      ok = end >= a && end - a >= min_len;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint64_t at = u * 16 + i;
      if (at < mis || at - mis >= n_bases) continue;
      const uint64_t p = at - mis;
      while (p >= end && c + 1 < n_ctgs) {
        c++;
        const uint64_t a = end;
        end = offs[c + 1];
        ok = end >= a && end - a >= min_len;
      }
      const uint32_t byte = (fa_word(v, i >> 2) >> (8 * (i & 3))) & 0xFF;
      ns += (ok && p < end && byte == 'N') ? 1 : 0;
    }
  }
  ns = fa_block_reduce(ns, lds_u, FaAddU());
  if (threadIdx.x == 0 && ns) atomicAdd(&box->n_ns, ns);
}

struct FaWiden {
  __device__ uint64_t operator()(uint32_t v) const { return v; }
};

// sorted: the lengths in descending order, run: their running sums. The one place i with run[i] >= half > run[i - 1],
// half = ceil(tot / 2), is the last of the L50 leading contigs.
__global__ __launch_bounds__(FA_THREADS) void k_fa_n50(const uint32_t *sorted, const uint64_t *run, uint64_t n,
                                                        uint64_t n_counted, uint64_t tot, unsigned long long *out) {
  const uint64_t half = tot / 2 + (tot & 1);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n && i < n_counted;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (run[i] >= half && (i == 0 || run[i - 1] < half)) {
      out[0] = sorted[i];
      out[1] = i + 1;
    }
  }
}

// depth * 10^6 rounded to nearest, ties to even: what "%f" prints, without its point. bits: a finite double >= 0 below 2^32.
__device__ __forceinline__ uint64_t fa_micro(uint64_t bits) {
  const uint32_t e = (uint32_t)(bits >> 52) & 0x7FF;
  const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
  const uint64_t m = e ? frac | (1ull << 52) : frac;
  const uint32_t s = e ? 1075u - e : 1074u;  // x = m 2^-s; x < 2^32 gives s >= 21
  const uint64_t lo = m * 1000000ull, hi = __umul64hi(m, 1000000ull);  // the product is below 2^73
  if (s >= 74) return 0;  // below one half of 10^-6
  uint64_t q;
  bool above, tie;
  if (s < 64) {
    q = (lo >> s) | (hi << (64 - s));
    const uint64_t rem = lo & ((1ull << s) - 1), h = 1ull << (s - 1);
    above = rem > h;
    tie = rem == h;
  } else if (s == 64) {
    q = hi;
    above = lo > (1ull << 63);
    tie = lo == (1ull << 63);
  } else {
    const uint32_t r = s - 64;  // 1 .. 9
    q = hi >> r;
    const uint64_t rem_hi = hi & ((1ull << r) - 1), h_hi = 1ull << (r - 1);
    above = rem_hi > h_hi || (rem_hi == h_hi && lo != 0);
    tie = rem_hi == h_hi && lo == 0;
  }
  return q + ((above || (tie && (q & 1))) ? 1 : 0);
}

__device__ __forceinline__ uint32_t fa_digits(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) {
    v /= 10;
    d++;
  }
  return d;
}

__device__ __forceinline__ bool fa_depth_ok(uint64_t bits) {
  // the sign bit clear, finite, below 2^32 (0x41F0000000000000)
  return bits < 0x41F0000000000000ull;
}

// ">Contig" id " " integer part "." six digits "\n": 7 + digits(id) + 1 + digits(ip) + 7 + 1
__device__ __forceinline__ uint32_t fa_header_len(uint64_t id, uint64_t micro) {
  return 7 + fa_digits(id) + 1 + fa_digits(micro / 1000000ull) + 7 + 1;
}

// Per contig: the checks and the record's length (header, bases, newline; 0 when filtered out). rec[n_ctgs] = 0.
__global__ __launch_bounds__(FA_THREADS) void k_fa_table(const uint64_t *offs, const double *depths, uint64_t n_ctgs,
                                                          uint64_t first_id, uint32_t min_len, uint64_t *rec, FastaBox *box) {
  __shared__ unsigned long long lds_u[FA_THREADS];
  unsigned long long written = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (offs[0] != 0) fa_flag(&box->bad_off, 0);
    box->n_bases = offs[n_ctgs];
  }
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    if (c == n_ctgs) {
      rec[c] = 0;
      continue;
    }
    const uint64_t a = offs[c], b = offs[c + 1];
    uint64_t r = 0;
    if (b < a) {
      fa_flag(&box->bad_off, c);
    } else if (b - a >= min_len) {
      const uint64_t bits = (uint64_t)__double_as_longlong(depths[c]);
      if (!fa_depth_ok(bits)) {
        fa_flag(&box->bad_depth, c);
      } else {
        r = fa_header_len(first_id + c, fa_micro(bits)) + (b - a) + 1;
        written++;
      }
    }
    rec[c] = r;
  }
  written = fa_block_reduce(written, lds_u, FaAddU());
  if (threadIdx.x == 0 && written) atomicAdd(&box->n_written, written);
}

__global__ void k_fa_total(const uint64_t *dst, uint64_t n_ctgs, FastaBox *box) {
  if (blockIdx.x == 0 && threadIdx.x == 0) box->n_bytes = dst[n_ctgs];
}

// 16 bytes from byte `at` of seqs, all inside the array: the two aligned units that hold them, shifted together. Neither
// aligned load touches a 16-byte unit without a byte of the array in it.
__device__ __forceinline__ uint4 fa_load16(const char *seqs, uint64_t at) {
  const uintptr_t adr = (uintptr_t)seqs + at;
  const uint32_t sh = (uint32_t)(adr & 15);
  const uint4 *p = (const uint4 *)(adr - sh);
  const uint4 v0 = p[0];
  if (sh == 0) return v0;
  const uint4 v1 = p[1];
  const uint64_t q0 = v0.x | ((uint64_t)v0.y << 32), q1 = v0.z | ((uint64_t)v0.w << 32);
  const uint64_t q2 = v1.x | ((uint64_t)v1.y << 32), q3 = v1.z | ((uint64_t)v1.w << 32);
  const uint64_t a = sh >= 8 ? q1 : q0, b = sh >= 8 ? q2 : q1, c = sh >= 8 ? q3 : q2;
  const uint32_t bits = 8 * (sh & 7);
  const uint64_t o0 = bits ? (a >> bits) | (b << (64 - bits)) : a;
  const uint64_t o1 = bits ? (b >> bits) | (c << (64 - bits)) : b;
  return make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
}

// where contig c's bases lie in the text: [seq0, seq0 + len) inside its record [d0, d1); len 0 for a contig without a
// record or with offsets that do not fit it
struct FaRec {
  uint64_t d1, s0, seq0, len;
};
__device__ __forceinline__ FaRec fa_rec(const uint64_t *soff, const uint64_t *doff, uint64_t c, uint64_t n_bases) {
  FaRec r;
  const uint64_t d0 = doff[c], s0 = soff[c], s1 = soff[c + 1];
  r.d1 = doff[c + 1];
  r.s0 = s0;
  uint64_t len = s1 >= s0 && s1 <= n_bases ? s1 - s0 : 0;
  if (r.d1 <= d0 || r.d1 - d0 <= len) len = 0;
  r.len = len;
  r.seq0 = r.d1 - 1 - len;
  return r;
}

// The bases into the text, one aligned 16-byte unit of the text per lane (the text's buffer is 16-byte aligned and holds
// whole units). Header bytes and newlines are written as zeros here and filled in by k_fa_headers, which runs after.
__global__ __launch_bounds__(FA_THREADS) void k_fa_copy(const char *seqs, const uint64_t *soff, uint64_t n_ctgs,
                                                         uint64_t n_bases, const uint64_t *doff, uint64_t n_bytes,
                                                         char *text) {
  const uint64_t n_units = (n_bytes + 15) / 16;
  uint4 *out = (uint4 *)text;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t pos0 = u * 16;
    uint64_t c = fa_find(doff, n_ctgs, pos0);
    FaRec r = fa_rec(soff, doff, c, n_bases);
    if (pos0 >= r.seq0 && pos0 + 16 <= r.seq0 + r.len) {  // the whole unit inside the contig's bases
      out[u] = fa_load16(seqs, r.s0 + (pos0 - r.seq0));
      continue;
    }
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint64_t pos = pos0 + i;
      while (pos >= r.d1 && c + 1 < n_ctgs) {
        c++;
        r = fa_rec(soff, doff, c, n_bases);
      }
      uint32_t byte = 0;
      if (pos < n_bytes && pos >= r.seq0 && pos - r.seq0 < r.len) {
        const uint64_t at = r.s0 + (pos - r.seq0);
        if (at < n_bases) byte = (uint8_t)seqs[at];
      }
      const uint32_t sh = byte << (8 * (i & 3));
      if ((i >> 2) == 0) w0 |= sh;
      else if ((i >> 2) == 1) w1 |= sh;
      else if ((i >> 2) == 2) w2 |= sh;
      else w3 |= sh;
    }
    out[u] = make_uint4(w0, w1, w2, w3);
  }
}

__device__ __forceinline__ void fa_put_dec(char *p, uint64_t v, uint32_t nd) {
  for (uint32_t j = nd; j-- > 0;) {
    p[j] = (char)('0' + v % 10);
    v /= 10;
  }
}

// The header of every record and the newline that closes it
__global__ __launch_bounds__(FA_THREADS) void k_fa_headers(const uint64_t *soff, const double *depths, uint64_t n_ctgs,
                                                            uint64_t first_id, const uint64_t *doff, uint64_t n_bytes,
                                                            char *text) {
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t d0 = doff[c], d1 = doff[c + 1];
    if (d1 <= d0 || d1 > n_bytes) continue;
    const uint64_t bits = (uint64_t)__double_as_longlong(depths[c]);
    if (!fa_depth_ok(bits)) continue;
    const uint64_t id = first_id + c, micro = fa_micro(bits), ip = micro / 1000000ull;
    const uint32_t nid = fa_digits(id), nip = fa_digits(ip);
    const uint64_t hdr = 7 + nid + 1 + nip + 7 + 1;
    if (d1 - d0 < hdr + 1) continue;
    char *p = text + d0;
    p[0] = '>', p[1] = 'C', p[2] = 'o', p[3] = 'n', p[4] = 't', p[5] = 'i', p[6] = 'g';
    fa_put_dec(p + 7, id, nid);
    p += 7 + nid;
    *p++ = ' ';
    fa_put_dec(p, ip, nip);
    p += nip;
    *p++ = '.';
    fa_put_dec(p, micro % 1000000ull, 6);
    p[6] = '\n';
    text[d1 - 1] = '\n';
  }
}

size_t fa_al(uint64_t n, size_t sz) { return (size_t)((n * sz + 255) / 256 * 256); }

size_t fa_sort_tmp(uint64_t n) {
  size_t a = 0, b = 0;
  const size_t m = (size_t)std::max<uint64_t>(n, 1);
  (void)rocprim::radix_sort_keys_desc(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, m, 0, 32);
  (void)rocprim::inclusive_scan(nullptr, b, rocprim::make_transform_iterator((const uint32_t *)nullptr, FaWiden()),
                                (uint64_t *)nullptr, m, rocprim::plus<uint64_t>());
  return std::max(a, b) + 256;
}

size_t fa_scan_tmp(uint64_t n) {
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)(n + 1),
                                rocprim::plus<uint64_t>());
  return b + 256;
}

}  // namespace

// lens u32 [n], sorted u32 [n], running sums u64 [n], rocprim's scratch
size_t ctg_n50_scratch_bytes(uint64_t n) { return 2 * fa_al(n + 1, 4) + fa_al(n + 1, 8) + fa_sort_tmp(n); }

uint32_t *ctg_n50_lens(void *scratch) { return (uint32_t *)scratch; }
const uint32_t *ctg_n50_sorted(const void *scratch, uint64_t n) { return (const uint32_t *)((const char *)scratch + fa_al(n + 1, 4)); }

hipError_t launch_ctg_n50(uint64_t n, uint64_t n_counted, uint64_t tot_len, void *scratch, size_t scratch_bytes,
                          unsigned long long *out, hipStream_t s) {
  if (scratch_bytes < ctg_n50_scratch_bytes(n)) return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(out, 0, 16, s)) != hipSuccess) return e;
  if (!n || !n_counted) return hipSuccess;
  uint32_t *lens = (uint32_t *)scratch;
  uint32_t *sorted = (uint32_t *)((char *)scratch + fa_al(n + 1, 4));
  uint64_t *run = (uint64_t *)((char *)scratch + 2 * fa_al(n + 1, 4));
  void *tmp = (char *)scratch + 2 * fa_al(n + 1, 4) + fa_al(n + 1, 8);
  size_t tb = scratch_bytes - (2 * fa_al(n + 1, 4) + fa_al(n + 1, 8));
  if ((e = rocprim::radix_sort_keys_desc(tmp, tb, (const uint32_t *)lens, sorted, (size_t)n, 0, 32, s)) != hipSuccess) return e;
  if ((e = rocprim::inclusive_scan(tmp, tb, rocprim::make_transform_iterator((const uint32_t *)sorted, FaWiden()), run,
                                   (size_t)n, rocprim::plus<uint64_t>(), s)) != hipSuccess)
    return e;
  k_fa_n50<<<grid_for(std::min(n, n_counted)), FA_THREADS, 0, s>>>(sorted, run, n, n_counted, tot_len, out);
  return hipGetLastError();
}

hipError_t launch_ctg_stats_table(const uint64_t *offs, const double *depths, uint64_t n_ctgs, uint32_t min_len,
                                  uint32_t *lens, double *partial, CtgStatsBox *box, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemsetAsync(box, 0, sizeof(CtgStatsBox), s)) != hipSuccess) return e;
  const uint64_t n_chunks = (n_ctgs + FA_CHUNK - 1) / FA_CHUNK;
  // (every chunk's sum is the same whichever workgroup takes it: the grid only has to be positive)
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, grid_for(n_chunks * FA_THREADS)));
  k_fa_stats<<<grid, FA_THREADS, 0, s>>>(offs, depths, n_ctgs, min_len, lens, partial, box);
  return hipGetLastError();
}

hipError_t launch_ctg_stats_ns(const char *seqs, const uint64_t *offs, uint64_t n_ctgs, uint64_t n_bases, uint32_t min_len,
                               CtgStatsBox *box, hipStream_t s) {
  if (!n_bases || !n_ctgs) return hipSuccess;
  k_fa_ns<<<grid_for((n_bases + 31) / 16), FA_THREADS, 0, s>>>(seqs, offs, n_ctgs, n_bases, min_len, box);
  return hipGetLastError();
}

// rec u64 [n + 1], dst u64 [n + 1], rocprim's scratch
size_t fasta_scratch_bytes(uint64_t n_ctgs) { return 2 * fa_al(n_ctgs + 1, 8) + fa_scan_tmp(n_ctgs); }

hipError_t launch_fasta_table(const uint64_t *offs, const double *depths, uint64_t n_ctgs, uint64_t first_id,
                              uint32_t min_len, void *scratch, size_t scratch_bytes, FastaBox *box, const uint64_t **dst_off,
                              hipStream_t s) {
  if (scratch_bytes < fasta_scratch_bytes(n_ctgs)) return hipErrorInvalidValue;
  uint64_t *rec = (uint64_t *)scratch;
  uint64_t *dst = (uint64_t *)((char *)scratch + fa_al(n_ctgs + 1, 8));
  void *tmp = (char *)scratch + 2 * fa_al(n_ctgs + 1, 8);
  size_t tb = scratch_bytes - 2 * fa_al(n_ctgs + 1, 8);
  *dst_off = dst;
  hipError_t e;
  if ((e = hipMemsetAsync(box, 0, sizeof(FastaBox), s)) != hipSuccess) return e;
  k_fa_table<<<grid_for(n_ctgs + 1), FA_THREADS, 0, s>>>(offs, depths, n_ctgs, first_id, min_len, rec, box);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = rocprim::exclusive_scan(tmp, tb, (const uint64_t *)rec, dst, (uint64_t)0, (size_t)(n_ctgs + 1),
                                   rocprim::plus<uint64_t>(), s)) != hipSuccess)
    return e;
  k_fa_total<<<1, 64, 0, s>>>(dst, n_ctgs, box);
  return hipGetLastError();
}

hipError_t launch_fasta_copy(const char *seqs, const uint64_t *offs, uint64_t n_ctgs, uint64_t n_bases,
                             const uint64_t *dst_off, uint64_t n_bytes, char *text, hipStream_t s) {
  if (!n_bytes || !n_ctgs) return hipSuccess;
  if (((uintptr_t)text & 15) != 0) return hipErrorInvalidValue;
  k_fa_copy<<<grid_for((n_bytes + 15) / 16), FA_THREADS, 0, s>>>(seqs, offs, n_ctgs, n_bases, dst_off, n_bytes, text);
  return hipGetLastError();
}

hipError_t launch_fasta_headers(const uint64_t *offs, const double *depths, uint64_t n_ctgs, uint64_t first_id,
                                const uint64_t *dst_off, uint64_t n_bytes, char *text, hipStream_t s) {
  if (!n_bytes || !n_ctgs) return hipSuccess;
  k_fa_headers<<<grid_for(n_ctgs), FA_THREADS, 0, s>>>(offs, depths, n_ctgs, first_id, dst_off, n_bytes, text);
  return hipGetLastError();
}

}  // namespace mhm
