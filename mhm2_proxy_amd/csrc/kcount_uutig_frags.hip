// The uutigs of the union of all ranks' tables from rank-local fragments, on gfx950 (mhmkc_uutigs_frags, DESIGN.md
// §3.12c): traverse_debruijn_graph walks inside a rank and connect_frags joins what crosses ranks
// (src/dbjg_traversal.cpp:291-335,517-567). Here a rank ranks its own rows with the kernels of kcount_uutig.hip over
// links whose cross-rank neighbours are ends; what that leaves between cross-linked ports is a fragment. The open
// fragments of all ranks, one record each, are the rows of a second, replicated graph that the same pointer jumping
// ranks with weighted states: a port's dist counts the rows of the fragments passed, its sum their counts.
//
// The kernels keep the style of kcount_uutig.hip: 256 threads, grid-stride, no LDS, and every index read from memory
// is checked against its bound before it is used.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"

namespace mhm {

namespace {

constexpr int U_THREADS = 256;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
constexpr uint64_t PORT_MASK = (1ull << 40) - 1;
constexpr uint64_t DONE = 1ull << 63;
constexpr int ROUND_SHIFT = 48;
constexpr int RW = UFRAG_REST_WORDS;

inline unsigned grid_for(uint64_t n) { return query_grid_for(n); }

__device__ __forceinline__ bool link_ok(uint8_t st) { return (st & 0x7f) == MHMKC_LINK_OK; }

// ---- stage 1: the claims

// A routed link entry x = d * n + i that is OK and names a row of another rank sends that rank one claim
__device__ __forceinline__ bool claims(const uint8_t *rl_rank, const uint8_t *rl_status, uint64_t x, int me, int g,
                                       uint32_t &to) {
  if (!link_ok(rl_status[x])) return false;
  to = rl_rank[x];
  return (int)to != me && (int)to < g;
}

__global__ __launch_bounds__(U_THREADS) void k_ufrag_claim_count(uint64_t n, int me, int g, const uint8_t *rl_rank,
                                                                  const uint8_t *rl_status, unsigned long long *hist) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < 2 * n; x += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t to;
    if (claims(rl_rank, rl_status, x, me, g, to)) atomicAdd(&hist[to], 1ull);
  }
}

// claim = {the claiming row, the row it enters, d | e << 1}: port (row, d) of the sender enters port (row, e) of the receiver
__global__ __launch_bounds__(U_THREADS) void k_ufrag_claim_pack(uint64_t n, int me, int g, const uint32_t *rl_row,
                                                                 const uint8_t *rl_rank, const uint8_t *rl_status,
                                                                 unsigned long long *cursor, uint64_t cap, uint32_t *send) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < 2 * n; x += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t to;
    if (!claims(rl_rank, rl_status, x, me, g, to)) continue;
    const uint32_t d = x >= n ? 1u : 0u;
    const uint64_t i = x - d * n;
    const uint32_t e = d ^ (uint32_t)(rl_status[x] >> 7) ^ 1u;
    const unsigned long long at = atomicAdd(&cursor[to], 1ull);
    if (at >= cap) continue;
    send[3 * at] = (uint32_t)i;
    send[3 * at + 1] = rl_row[x];
    send[3 * at + 2] = d | e << 1;
  }
}

// A received claim of rank `from` cross-links own port (j, e) iff that port's own link is OK, names the claiming row of
// that rank and enters it through the claiming direction: port_link's rule (kcount_uutig.hip) with its two halves on
// two ranks. xlink is indexed by port, 2 * row + direction.
__global__ __launch_bounds__(U_THREADS) void k_ufrag_claim_match(const uint32_t *recv, uint64_t n_recv, uint32_t from,
                                                                  uint64_t n, const uint32_t *rl_row, const uint8_t *rl_rank,
                                                                  const uint8_t *rl_status, uint8_t *xlink,
                                                                  unsigned long long *n_links) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_recv; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t fi = recv[3 * r], fl = recv[3 * r + 2];
    const uint64_t j = recv[3 * r + 1];
    if (j >= n) continue;
    const uint32_t d = fl & 1u, e = (fl >> 1) & 1u;
    const uint64_t x = e * n + j;
    const uint8_t st = rl_status[x];
    if (!link_ok(st) || rl_rank[x] != from || rl_row[x] != fi) continue;
    if ((e ^ (uint32_t)(st >> 7) ^ 1u) != d) continue;
    xlink[2 * j + e] = 1;
    atomicAdd(n_links, 1ull);
  }
}

// ---- stage 2: the links of the rank's own table: a neighbour on this rank stays, every other OK link becomes an end
__global__ __launch_bounds__(U_THREADS) void k_ufrag_local_links(uint64_t n, int me, const uint32_t *rl_row,
                                                                  const uint8_t *rl_rank, const uint8_t *rl_status,
                                                                  uint32_t *next, uint8_t *status) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < 2 * n; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint8_t st = rl_status[x];
    const bool own = link_ok(st) && (int)rl_rank[x] == me;
    next[x] = own ? rl_row[x] : NO_ROW;
    status[x] = own ? st : (link_ok(st) ? (uint8_t)MHMKC_LINK_DEADEND : st);
  }
}

// whether port (i, 1) is linked under the local links (port_link of kcount_uutig.hip, for d = 1)
__device__ __forceinline__ bool right_linked(const uint32_t *next, const uint8_t *status, uint64_t n, uint64_t i) {
  const uint32_t d = 1;
  const uint8_t st = status[d * n + i];
  if (!link_ok(st)) return false;
  const uint64_t j = next[d * n + i];
  if (j >= n) return false;
  const uint32_t e = d ^ (uint32_t)(st >> 7) ^ 1u;
  if (j == i && e == d) return false;
  const uint8_t st2 = status[e * n + j];
  if (!link_ok(st2)) return false;
  return (uint64_t)next[e * n + j] == i && (e ^ (uint32_t)(st2 >> 7) ^ 1u) == d;
}

// Every fragment (start row starts[t]) learns whether one of its two end ports is cross-linked. A closed fragment is a
// contig of the union and its start joins the rank's contig starts; an open one takes a place among the rank's records.
__global__ __launch_bounds__(U_THREADS) void k_ufrag_classify(const uint32_t *starts, uint64_t n_frag, uint64_t n,
                                                               const UutigPort *st, const uint8_t *xlink,
                                                               const uint32_t *next, const uint8_t *status,
                                                               uint32_t *row_ctg, uint32_t *lf_open, uint32_t *cstarts,
                                                               unsigned long long *ctr) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_frag; t += (uint64_t)gridDim.x * blockDim.x) {
    lf_open[t] = NO_ROW;
    const uint64_t s = starts[t];
    if (s >= n) {
      atomicAdd(&ctr[UFRAG_C_BAD], 1ull);
      continue;
    }
    const uint64_t e0 = st[2 * s].link & PORT_MASK, e1 = st[2 * s + 1].link & PORT_MASK;
    if (e0 >= 2 * n || e1 >= 2 * n) {
      atomicAdd(&ctr[UFRAG_C_BAD], 1ull);
      continue;
    }
    row_ctg[s] = (uint32_t)t;
    if (xlink[e0] | xlink[e1]) {
      lf_open[t] = (uint32_t)atomicAdd(&ctr[UFRAG_C_OPEN], 1ull);
    } else {
      const unsigned long long at = atomicAdd(&ctr[UFRAG_C_STARTS], 1ull);
      if (at < n) cstarts[at] = (uint32_t)s;
      atomicAdd(&ctr[UFRAG_C_CLOSED], 1ull);
      // a cycle was opened at its start's port 1: that port is an end although its local link is mutual
      if (e1 == 2 * s + 1 && right_linked(next, status, n, s)) atomicAdd(&ctr[UFRAG_C_CYCLES], 1ull);
    }
  }
}

// ---- stage 3: the record of every open fragment, written at its place among all ranks' records
__global__ __launch_bounds__(U_THREADS) void k_ufrag_emit(OutRows t, uint64_t n, int nl, int nlo, const uint32_t *starts,
                                                           uint64_t n_frag, const UutigPort *st, const uint8_t *xlink,
                                                           const uint32_t *rl_row, const uint8_t *rl_rank,
                                                           const uint8_t *rl_status, const uint32_t *lf_open, uint32_t me,
                                                           uint64_t n_open, uint64_t *keys, uint64_t *rest) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_frag; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o = lf_open[x];
    const uint64_t s = starts[x];
    if (o >= n_open || s >= n) continue;
    const UutigPort a = st[2 * s], b = st[2 * s + 1];
    const uint64_t e[2] = {a.link & PORT_MASK, b.link & PORT_MASK};
    if (e[0] >= 2 * n || e[1] >= 2 * n) continue;
    uint64_t prow[2] = {NO_ROW, NO_ROW}, prank[2] = {0xff, 0xff}, pdir[2] = {0, 0}, has[2] = {0, 0};
    for (int y = 0; y < 2; y++) {
      if (!xlink[e[y]]) continue;
      const uint64_t j = e[y] >> 1, d = e[y] & 1, le = d * n + j;
      has[y] = 1;
      prow[y] = rl_row[le];
      prank[y] = rl_rank[le];
      pdir[y] = d ^ (uint64_t)(rl_status[le] >> 7) ^ 1u;
    }
    for (int j = 0; j < nl; j++) keys[o * nl + j] = t.keys[s * (uint64_t)nlo + j];
    uint64_t *r = rest + o * RW;
    r[0] = a.sum + b.sum - t.counts[s];
    r[1] = s | ((uint64_t)a.dist + b.dist + 1) << 32;
    r[2] = (e[0] >> 1) | (e[1] >> 1) << 32;
    r[3] = prow[0] | prow[1] << 32;
    r[4] = (uint64_t)t.counts[s] | (uint64_t)me << 16 | prank[0] << 24 | prank[1] << 32 | (e[0] & 1) << 40 |
           (e[1] & 1) << 41 | pdir[0] << 42 | pdir[1] << 43 | has[0] << 44 | has[1] << 45;
    r[5] = a.dist;
  }
}

// the fields of a record
__device__ __forceinline__ uint64_t f_sum(const uint64_t *rest, uint64_t f) { return rest[f * RW]; }
__device__ __forceinline__ uint64_t f_start(const uint64_t *rest, uint64_t f) { return rest[f * RW + 1] & 0xffffffffull; }
__device__ __forceinline__ uint64_t f_rows(const uint64_t *rest, uint64_t f) { return rest[f * RW + 1] >> 32; }
__device__ __forceinline__ uint64_t f_rank(const uint64_t *rest, uint64_t f) { return (rest[f * RW + 4] >> 16) & 0xff; }
__device__ __forceinline__ uint64_t f_lp(const uint64_t *rest, uint64_t f) { return rest[f * RW + 5] & 0xffffffffull; }
__device__ __forceinline__ bool f_has(const uint64_t *rest, uint64_t f, int y) { return (rest[f * RW + 4] >> (44 + y)) & 1; }
// a port as one word: rank << 33 | row << 1 | direction
__device__ __forceinline__ uint64_t f_end(const uint64_t *rest, uint64_t f, int y) {
  const uint64_t fl = rest[f * RW + 4], row = (rest[f * RW + 2] >> (32 * y)) & 0xffffffffull;
  return ((fl >> 16) & 0xff) << 33 | row << 1 | ((fl >> (40 + y)) & 1);
}
__device__ __forceinline__ uint64_t f_peer(const uint64_t *rest, uint64_t f, int y) {
  const uint64_t fl = rest[f * RW + 4], row = (rest[f * RW + 3] >> (32 * y)) & 0xffffffffull;
  return ((fl >> (24 + 8 * y)) & 0xff) << 33 | row << 1 | ((fl >> (42 + y)) & 1);
}

// ---- stage 4: the fragment graph

__global__ __launch_bounds__(U_THREADS) void k_ufrag_port_keys(const uint64_t *rest, uint64_t nf, uint64_t *pk,
                                                                uint64_t *pv) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < 2 * nf; p += (uint64_t)gridDim.x * blockDim.x) {
    pk[p] = f_end(rest, p >> 1, (int)(p & 1));
    pv[p] = p;
  }
}

// entry[p] = the fragment port that fragment port p enters: the end port equal to p's peer whose own peer is p's end
__global__ __launch_bounds__(U_THREADS) void k_ufrag_resolve(const uint64_t *rest, uint64_t nf, const uint64_t *spk,
                                                              const uint64_t *spv, uint64_t *entry) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < 2 * nf; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t f = p >> 1;
    const int y = (int)(p & 1);
    uint64_t en = ~0ull;
    if (f_has(rest, f, y)) {
      const uint64_t want = f_peer(rest, f, y);
      uint64_t lo = 0, hi = 2 * nf;
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (spk[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      if (lo < 2 * nf && spk[lo] == want) {
        const uint64_t q = spv[lo];
        if (q < 2 * nf && (q >> 1) != f && f_has(rest, q >> 1, (int)(q & 1)) &&
            f_peer(rest, q >> 1, (int)(q & 1)) == f_end(rest, f, y))
          en = q;
      }
    }
    entry[p] = en;
  }
}

// k_uutig_init for fragments: the first, weighted state of every fragment port (or of the listed ones; cut: their
// cycles are opened between the start fragment's port 1 and the fragment it leads to)
__global__ __launch_bounds__(U_THREADS) void k_ufrag_init(const uint64_t *keys, const uint64_t *rest, uint64_t nf, int nl,
                                                           const uint64_t *entry, const uint64_t *list, uint64_t n_items,
                                                           const UutigPort *cut, uint32_t round, UutigPort *st) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_items; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = list ? list[x] : x;
    if (p >= 2 * nf) continue;
    const uint64_t f = p >> 1, q = entry[p];
    bool linked = q < 2 * nf;
    if (cut && linked) {
      const uint64_t cp = 2 * (uint64_t)cut[p].minrow + 1;
      if (p == cp || q == cp) linked = false;
    }
    UutigPort a;
    a.sum = f_sum(rest, f);
    a.minw0 = keys[f * nl];
    a.minrow = (uint32_t)f;
    a.dist = linked ? (uint32_t)f_rows(rest, q >> 1) : 0u;
    a.link = (linked ? (q ^ 1) : (p | DONE)) | (uint64_t)(round & 0xffu) << ROUND_SHIFT;
    st[p] = a;
  }
}

// Kmer::operator< on (first word, fragment), as key_before of kcount_uutig.hip
__device__ __forceinline__ bool frag_before(uint64_t aw, uint32_t ar, uint64_t bw, uint32_t br, const uint64_t *keys,
                                            uint64_t nf, int nl) {
  if (aw != bw) return aw < bw;
  if (ar == br || ar >= nf || br >= nf) return false;
  for (int j = 1; j < nl; j++) {
    const uint64_t x = keys[(uint64_t)ar * nl + j], y = keys[(uint64_t)br * nl + j];
    if (x != y) return x < y;
  }
  return false;
}

// Every fragment's contig (its start fragment), the rows before it and its strand against the start fragment;
// flag: 1 reversed, 2 a start fragment, 4 a start fragment of a cycle. isstart [nf + 1] feeds the scan of the contig places.
__global__ __launch_bounds__(U_THREADS) void k_ufrag_place(const uint64_t *keys, uint64_t nf, int nl, const UutigPort *st,
                                                            const uint64_t *entry, uint32_t *comp, uint32_t *off,
                                                            uint8_t *flag, uint32_t *isstart, unsigned long long *ctr) {
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f <= nf; f += (uint64_t)gridDim.x * blockDim.x) {
    if (f == nf) {
      isstart[f] = 0;
      continue;
    }
    const UutigPort a = st[2 * f], b = st[2 * f + 1];
    const uint64_t s = frag_before(b.minw0, b.minrow, a.minw0, a.minrow, keys, nf, nl) ? b.minrow : a.minrow;
    if (s >= nf) {
      atomicAdd(&ctr[UFRAG_C_BAD], 1ull);
      comp[f] = NO_ROW;
      off[f] = 0;
      flag[f] = 0;
      isstart[f] = 0;
      continue;
    }
    const uint64_t end0 = st[2 * s].link & PORT_MASK;
    const bool rc = (a.link & PORT_MASK) != end0;
    uint8_t fl = rc ? 1 : 0;
    if (s == f) {
      fl |= 2;
      if (entry[2 * f + 1] < 2 * nf && (b.link & PORT_MASK) == 2 * f + 1) {
        fl |= 4;
        atomicAdd(&ctr[UFRAG_C_XCYCLES], 1ull);
      }
    }
    comp[f] = (uint32_t)s;
    off[f] = rc ? b.dist : a.dist;
    flag[f] = fl;
    isstart[f] = s == f ? 1u : 0u;
  }
}

// what a fragment needs of its contig: its rows, its sum, the rotation of a cycle
struct UfragCtg {
  uint64_t rows, sum, rot;
  bool cyc;
};
__device__ __forceinline__ UfragCtg ctg_of(const UfragGraph &g, uint64_t s) {
  const UutigPort a = g.st[2 * s], b = g.st[2 * s + 1];
  const uint64_t ms = f_rows(g.rest, s), lp = f_lp(g.rest, s);
  UfragCtg c;
  c.rows = (uint64_t)a.dist + b.dist + ms;
  c.sum = a.sum + b.sum - f_sum(g.rest, s);
  c.cyc = (g.flag[s] & 4) != 0;
  c.rot = c.cyc && lp < ms ? ms - 1 - lp : 0;
  return c;
}
// the final position of the row that lies q rows into fragment f's stretch of the contig
__device__ __forceinline__ uint64_t ctg_pos(const UfragCtg &c, uint64_t off, uint64_t q) {
  return c.cyc ? (off + q + c.rot) % c.rows : off + q;
}
// whether fragment f (rows mf, offset off) holds the contig's last row
__device__ __forceinline__ bool holds_last(const UfragCtg &c, uint64_t off, uint64_t mf) {
  if (!c.cyc) return off + mf == c.rows;
  return (2 * c.rows - 1 - c.rot % c.rows - off % c.rows) % c.rows < mf;
}

// ---- stage 5: the contigs of this rank

// the start rows of the cross-rank contigs this rank owns join its contig starts
__global__ __launch_bounds__(U_THREADS) void k_ufrag_owned(const uint64_t *rest, uint64_t f0, uint64_t f1, uint64_t nf,
                                                            const uint8_t *flag, uint64_t n, uint32_t *cstarts,
                                                            unsigned long long *ctr) {
  for (uint64_t f = f0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < f1 && f < nf;
       f += (uint64_t)gridDim.x * blockDim.x) {
    if (!(flag[f] & 2)) continue;
    const uint64_t s = f_start(rest, f);
    const unsigned long long at = atomicAdd(&ctr[UFRAG_C_STARTS], 1ull);
    if (s < n && at < n) cstarts[at] = (uint32_t)s;
    atomicAdd(&ctr[UFRAG_C_MINE], 1ull);
  }
}

__global__ __launch_bounds__(U_THREADS) void k_ufrag_sort_word(const uint64_t *keys, uint64_t n, int nlo, int w,
                                                                const uint32_t *rows, uint64_t n_ctgs, uint64_t *word) {
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = rows[c];
    word[c] = r < n ? keys[r * nlo + w] : ~0ull;
  }
}

// contig c of this rank is the one with the c-th smallest start row: a closed fragment (its ranking state, as
// k_uutig_ctgs) or a cross-rank contig (the fragment graph's state of its start fragment, whose global id goes into gid)
__global__ __launch_bounds__(U_THREADS) void k_ufrag_ctgs(const uint32_t *sorted, uint64_t n_ctgs, OutRows t, uint64_t n,
                                                           int k, const UutigPort *rst, const uint32_t *row_ctg,
                                                           const uint32_t *lf_open, uint32_t *lf_ctg, uint64_t n_frag,
                                                           uint64_t f0, uint64_t n_open, UfragGraph g, uint64_t first_id,
                                                           uint32_t *gid, uint32_t *n_kmers, double *depths,
                                                           uint64_t *lens) {
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n_ctgs; c += (uint64_t)gridDim.x * blockDim.x) {
    if (c == n_ctgs) {
      lens[c] = 0;
      continue;
    }
    const uint64_t s = sorted[c];
    const uint64_t x = s < n ? row_ctg[s] : NO_ROW;
    uint64_t m = 0, sum = 0;
    if (x < n_frag) {
      lf_ctg[x] = (uint32_t)c;
      const uint64_t o = lf_open[x];
      if (o == NO_ROW) {
        const UutigPort a = rst[2 * s], b = rst[2 * s + 1];
        m = (uint64_t)a.dist + b.dist + 1;
        sum = a.sum + b.sum;
      } else if (o < n_open && f0 + o < g.nf) {
        const UfragCtg cc = ctg_of(g, f0 + o);
        m = cc.rows;
        sum = cc.sum + t.counts[s];
        const uint64_t at = g.cidx[f0 + o];
        if (at < g.xc) gid[at] = (uint32_t)(first_id + c);
      }
    }
    n_kmers[c] = (uint32_t)m;
    depths[c] = m ? (double)sum / (double)(m + 1) : 0;
    lens[c] = m ? m + (uint64_t)k - 1 : 0;
  }
}

// ---- stage 6: the bases that travel. A fragment of a contig that another rank owns is one segment: a base per row in
// contig order (before a cycle's rotation), then the k - 1 bases that follow the contig's last row if it holds it.
__global__ __launch_bounds__(U_THREADS) void k_ufrag_segs(UfragGraph g, int k, int n_ranks, uint32_t *key, uint64_t *len,
                                                           uint32_t *ident, unsigned long long *glen) {
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < g.nf; f += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = f_rank(g.rest, f), s = g.comp[f];
    uint64_t o = r, l = 0;
    if (s < g.nf && (int)r < n_ranks) {
      o = f_rank(g.rest, s);
      if (o != r && (int)o < n_ranks) {
        const UfragCtg c = ctg_of(g, s);
        const uint64_t mf = f_rows(g.rest, f);
        l = mf + (holds_last(c, g.off[f], mf) ? (uint64_t)k - 1 : 0);
        atomicAdd(&glen[r * n_ranks + o], (unsigned long long)l);
      } else {
        o = r;
      }
    }
    key[f] = (uint32_t)((int)r < n_ranks ? r * n_ranks + o : 0);
    len[f] = l;
    ident[f] = (uint32_t)f;
  }
}

__global__ __launch_bounds__(U_THREADS) void k_ufrag_take(const uint32_t *order, const uint64_t *len, uint64_t nf,
                                                           uint64_t *out) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < nf; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t f = order[x];
    out[x] = f < nf ? len[f] : 0;
  }
}

__global__ __launch_bounds__(U_THREADS) void k_ufrag_put(const uint32_t *order, const uint64_t *scanned, uint64_t nf,
                                                          uint64_t *pos) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < nf; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t f = order[x];
    if (f < nf) pos[f] = scanned[x];
  }
}

template <int NL>
__device__ __forceinline__ char base_of(const uint64_t *w, int k, bool rc, int b) {
  const int x = rc ? k - 1 - b : b;
  uint32_t code = 0;
#pragma unroll
  for (int j = 0; j < NL; j++)
    if (j == x >> 5) code = (uint32_t)(w[j] >> (2 * (31 - (x & 31)))) & 3u;
  if (rc) code = 3u - code;
  return (char)((0x54474341u >> (8 * code)) & 0xffu);
}

// The final row map of every own row, and its bases: into the rank's own contigs in place (as k_uutig_bases), into the
// segment of its fragment when another rank owns the contig. On entry row_ctg holds the row's local fragment, row_pos
// and row_rc its place in it (k_uutig_place).
template <int NL>
__global__ __launch_bounds__(U_THREADS) void k_ufrag_rows(OutRows t, uint64_t n, int k, int nlo, uint32_t *row_ctg,
                                                           uint32_t *row_pos, uint8_t *row_rc, const uint32_t *lf_open,
                                                           const uint32_t *lf_ctg, uint64_t n_frag, uint64_t f0,
                                                           uint64_t n_open, UfragGraph g, uint32_t me, uint64_t first_id,
                                                           uint64_t n_ctgs, const uint64_t *offsets, const uint32_t *n_kmers,
                                                           uint64_t n_bases, char *seqs, const uint64_t *seg_pos,
                                                           uint64_t seg_base, uint64_t send_bytes, char *send) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t x = row_ctg[i];
    if (x >= n_frag) {  // (a row with an X or F, or one whose fragment was refused)
      row_ctg[i] = NO_ROW;
      continue;
    }
    const uint64_t o = lf_open[x], lp = row_pos[i];
    bool rc = row_rc[i] != 0;
    uint64_t gidv = NO_ROW, pos = lp, m = 0, q = 0, f = 0, mf = 0;
    bool mine = true;
    if (o == NO_ROW) {
      const uint64_t c = lf_ctg[x];
      if (c < n_ctgs) {
        gidv = first_id + c;
        m = n_kmers[c];
      }
    } else if (o < n_open && f0 + o < g.nf) {
      f = f0 + o;
      const uint64_t s = g.comp[f];
      mf = f_rows(g.rest, f);
      if (s < g.nf && lp < mf && g.cidx[s] < g.xc) {
        const UfragCtg cc = ctg_of(g, s);
        const bool frc = (g.flag[f] & 1) != 0;
        q = frc ? mf - 1 - lp : lp;
        pos = ctg_pos(cc, g.off[f], q);
        rc = rc != frc;
        m = cc.rows;
        gidv = g.gid[g.cidx[s]];
        mine = f_rank(g.rest, s) == me;
      }
    }
    row_ctg[i] = (uint32_t)gidv;
    row_pos[i] = (uint32_t)pos;
    row_rc[i] = rc ? 1 : 0;
    if (gidv == NO_ROW || pos >= m) continue;
    const bool last = pos + 1 == m;
    uint64_t w[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) w[j] = t.keys[i * (uint64_t)nlo + j];
    if (mine) {
      const uint64_t c = gidv - first_id;
      if (gidv < first_id || c >= n_ctgs) continue;
      const uint64_t at = offsets[c] + pos;
      const int nb = last ? k : 1;
      if (at + (uint64_t)nb > n_bases) continue;
      for (int b = 0; b < nb; b++) seqs[at + b] = base_of<NL>(w, k, rc, b);
    } else {
      const uint64_t at = seg_pos[f] - seg_base;  // (the segment's place in this rank's send buffer)
      if (seg_pos[f] < seg_base || at + mf + (last ? (uint64_t)k - 1 : 0) > send_bytes) continue;
      send[at + q] = base_of<NL>(w, k, rc, 0);
      if (last)
        for (int b = 1; b < k; b++) send[at + mf + b - 1] = base_of<NL>(w, k, rc, b);
    }
  }
}

// The received segments into their contigs, a wave per fragment: base q of fragment f lies at the final position of
// its row, the k - 1 trailing bases behind the contig's last row. recv_base [n_ranks]: what turns a segment's place in
// the global layout into its place in this rank's receive buffer.
__global__ __launch_bounds__(U_THREADS) void k_ufrag_scatter(UfragGraph g, int k, uint32_t me, int n_ranks,
                                                              uint64_t first_id, uint64_t n_ctgs, const uint64_t *offsets,
                                                              uint64_t n_bases, char *seqs, const uint64_t *seg_pos,
                                                              const uint64_t *recv_base, const char *recv,
                                                              uint64_t recv_bytes) {
  const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) / warpSize;
  const uint64_t lane = threadIdx.x & (warpSize - 1);
  for (uint64_t f = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / warpSize; f < g.nf; f += waves) {
    const uint64_t r = f_rank(g.rest, f), s = g.comp[f];
    if (r == me || (int)r >= n_ranks || s >= g.nf || f_rank(g.rest, s) != me || g.cidx[s] >= g.xc) continue;
    const uint64_t gidv = g.gid[g.cidx[s]], c = gidv - first_id;
    if (gidv < first_id || c >= n_ctgs) continue;
    const UfragCtg cc = ctg_of(g, s);
    const uint64_t mf = f_rows(g.rest, f), off = g.off[f];
    const bool last = holds_last(cc, off, mf);
    const uint64_t src = seg_pos[f] + recv_base[r], len = mf + (last ? (uint64_t)k - 1 : 0), dst = offsets[c];
    if (src + len > recv_bytes || src + len < src || dst + cc.rows + (uint64_t)k - 1 > n_bases) continue;
    for (uint64_t q = lane; q < mf; q += warpSize) seqs[dst + ctg_pos(cc, off, q)] = recv[src + q];
    if (last)
      for (uint64_t b = lane; b + 1 < (uint64_t)k; b += warpSize) seqs[dst + cc.rows + b] = recv[src + mf + b];
  }
}

}  // namespace

// ---- launches

hipError_t launch_ufrag_claim_count(uint64_t n, int me, int g, const uint8_t *rl_rank, const uint8_t *rl_status,
                                    unsigned long long *hist, hipStream_t s) {
  if (!n) return hipSuccess;
  k_ufrag_claim_count<<<grid_for(2 * n), U_THREADS, 0, s>>>(n, me, g, rl_rank, rl_status, hist);
  return hipGetLastError();
}

hipError_t launch_ufrag_claim_pack(uint64_t n, int me, int g, const uint32_t *rl_row, const uint8_t *rl_rank,
                                   const uint8_t *rl_status, unsigned long long *cursor, uint64_t cap, uint32_t *send,
                                   hipStream_t s) {
  if (!n || !cap) return hipSuccess;
  k_ufrag_claim_pack<<<grid_for(2 * n), U_THREADS, 0, s>>>(n, me, g, rl_row, rl_rank, rl_status, cursor, cap, send);
  return hipGetLastError();
}

hipError_t launch_ufrag_claim_match(const uint32_t *recv, uint64_t n_recv, int from, uint64_t n, const uint32_t *rl_row,
                                    const uint8_t *rl_rank, const uint8_t *rl_status, uint8_t *xlink,
                                    unsigned long long *n_links, hipStream_t s) {
  if (!n || !n_recv) return hipSuccess;
  k_ufrag_claim_match<<<grid_for(n_recv), U_THREADS, 0, s>>>(recv, n_recv, (uint32_t)from, n, rl_row, rl_rank, rl_status,
                                                              xlink, n_links);
  return hipGetLastError();
}

hipError_t launch_ufrag_local_links(uint64_t n, int me, const uint32_t *rl_row, const uint8_t *rl_rank,
                                    const uint8_t *rl_status, uint32_t *next, uint8_t *status, hipStream_t s) {
  if (!n) return hipSuccess;
  k_ufrag_local_links<<<grid_for(2 * n), U_THREADS, 0, s>>>(n, me, rl_row, rl_rank, rl_status, next, status);
  return hipGetLastError();
}

hipError_t launch_ufrag_classify(const uint32_t *starts, uint64_t n_frag, uint64_t n, const UutigPort *st,
                                 const uint8_t *xlink, const uint32_t *next, const uint8_t *status, uint32_t *row_ctg,
                                 uint32_t *lf_open, uint32_t *cstarts, unsigned long long *ctr, hipStream_t s) {
  if (!n_frag) return hipSuccess;
  k_ufrag_classify<<<grid_for(n_frag), U_THREADS, 0, s>>>(starts, n_frag, n, st, xlink, next, status, row_ctg, lf_open,
                                                           cstarts, ctr);
  return hipGetLastError();
}

hipError_t launch_ufrag_emit(const OutRows &t, uint64_t n, int nl, int nlo, const uint32_t *starts, uint64_t n_frag,
                             const UutigPort *st, const uint8_t *xlink, const uint32_t *rl_row, const uint8_t *rl_rank,
                             const uint8_t *rl_status, const uint32_t *lf_open, int me, uint64_t n_open, uint64_t *keys,
                             uint64_t *rest, hipStream_t s) {
  if (!n_frag || !n_open) return hipSuccess;
  if (nlo < nl || nl < 1 || nl > 4) return hipErrorInvalidValue;
  k_ufrag_emit<<<grid_for(n_frag), U_THREADS, 0, s>>>(t, n, nl, nlo, starts, n_frag, st, xlink, rl_row, rl_rank, rl_status,
                                                       lf_open, (uint32_t)me, n_open, keys, rest);
  return hipGetLastError();
}

size_t ufrag_tmp_bytes(uint64_t n_items) {
  size_t a = 0, b = 0, c = 0, d = 0, e = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr,
                                  (uint64_t *)nullptr, (size_t)n_items);
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)n_items);
  (void)rocprim::exclusive_scan(nullptr, c, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n_items,
                                rocprim::plus<uint64_t>());
  (void)rocprim::exclusive_scan(nullptr, d, (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t)0, (size_t)n_items,
                                rocprim::plus<uint32_t>());
  e = std::max(std::max(a, b), std::max(c, d));
  return e + 512;
}

size_t ufrag_resolve_scratch_bytes(uint64_t nf) { return 2 * nf * 4 * 8 + 256; }

hipError_t launch_ufrag_resolve(const uint64_t *rest, uint64_t nf, void *scratch, size_t scratch_bytes, void *tmp,
                                size_t tmp_bytes, uint64_t *entry, hipStream_t s) {
  if (!nf) return hipSuccess;
  if (nf >= 0xffffffffull || scratch_bytes < ufrag_resolve_scratch_bytes(nf)) return hipErrorInvalidValue;
  uint64_t *pk = (uint64_t *)scratch, *spk = pk + 2 * nf, *pv = spk + 2 * nf, *spv = pv + 2 * nf;
  k_ufrag_port_keys<<<grid_for(2 * nf), U_THREADS, 0, s>>>(rest, nf, pk, pv);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, pk, spk, pv, spv, (size_t)(2 * nf), 0, 41, s)) != hipSuccess) return e;
  k_ufrag_resolve<<<grid_for(2 * nf), U_THREADS, 0, s>>>(rest, nf, spk, spv, entry);
  return hipGetLastError();
}

hipError_t launch_ufrag_init(const uint64_t *keys, const uint64_t *rest, uint64_t nf, int nl, const uint64_t *entry,
                             const uint64_t *list, uint64_t n_items, const UutigPort *cut, uint32_t round, UutigPort *st,
                             hipStream_t s) {
  if (!nf || !n_items) return hipSuccess;
  if (nl < 1 || nl > 4) return hipErrorInvalidValue;
  k_ufrag_init<<<grid_for(n_items), U_THREADS, 0, s>>>(keys, rest, nf, nl, entry, list, n_items, cut, round, st);
  return hipGetLastError();
}

hipError_t launch_ufrag_place(const uint64_t *keys, uint64_t nf, int nl, const UutigPort *st, const uint64_t *entry,
                              uint32_t *comp, uint32_t *off, uint8_t *flag, uint32_t *isstart, uint32_t *cidx, void *tmp,
                              size_t tmp_bytes, unsigned long long *ctr, hipStream_t s) {
  k_ufrag_place<<<grid_for(nf + 1), U_THREADS, 0, s>>>(keys, nf, nl, st, entry, comp, off, flag, isstart, ctr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return rocprim::exclusive_scan(tmp, tmp_bytes, isstart, cidx, (uint32_t)0, (size_t)(nf + 1), rocprim::plus<uint32_t>(), s);
}

hipError_t launch_ufrag_owned(const uint64_t *rest, uint64_t f0, uint64_t f1, uint64_t nf, const uint8_t *flag, uint64_t n,
                              uint32_t *cstarts, unsigned long long *ctr, hipStream_t s) {
  if (f1 <= f0) return hipSuccess;
  k_ufrag_owned<<<grid_for(f1 - f0), U_THREADS, 0, s>>>(rest, f0, f1, nf, flag, n, cstarts, ctr);
  return hipGetLastError();
}

size_t ufrag_table_scratch_bytes(uint64_t n_ctgs) { return (n_ctgs + 64) / 64 * 64 * (4 + 8 + 8 + 8); }

hipError_t launch_ufrag_table(const OutRows &t, uint64_t n, int k, int nl, int nlo, uint32_t *cstarts, uint64_t n_ctgs,
                              const UutigPort *rst, const uint32_t *row_ctg, const uint32_t *lf_open, uint32_t *lf_ctg,
                              uint64_t n_frag, uint64_t f0, uint64_t n_open, const UfragGraph &g, uint64_t first_id,
                              uint32_t *gid, void *scratch, size_t scratch_bytes, void *tmp, size_t tmp_bytes,
                              uint32_t *n_kmers, double *depths, uint64_t *offsets, hipStream_t s) {
  if (nlo < nl || nl < 1 || nl > 4 || scratch_bytes < ufrag_table_scratch_bytes(n_ctgs)) return hipErrorInvalidValue;
  const size_t a = (n_ctgs + 64) / 64 * 64;
  uint64_t *word = (uint64_t *)scratch, *word2 = word + a, *lens = word2 + a;
  uint32_t *rows2 = (uint32_t *)(lens + a);
  uint32_t *cur = cstarts, *alt = rows2;
  hipError_t e;
  if (n_ctgs) {
    // least significant word first, each pass stable: the starts end up in Kmer::operator< order (launch_uutig_table)
    for (int w = nl - 1; w >= 0; w--) {
      k_ufrag_sort_word<<<grid_for(n_ctgs), U_THREADS, 0, s>>>(t.keys, n, nlo, w, cur, n_ctgs, word);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, word, word2, cur, alt, (size_t)n_ctgs, 0, 64, s)) != hipSuccess)
        return e;
      std::swap(cur, alt);
    }
    if (cur != cstarts && (e = hipMemcpyAsync(cstarts, cur, n_ctgs * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
  }
  k_ufrag_ctgs<<<grid_for(n_ctgs + 1), U_THREADS, 0, s>>>(cstarts, n_ctgs, t, n, k, rst, row_ctg, lf_open, lf_ctg, n_frag, f0,
                                                           n_open, g, first_id, gid, n_kmers, depths, lens);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return rocprim::exclusive_scan(tmp, tmp_bytes, lens, offsets, (uint64_t)0, (size_t)(n_ctgs + 1), rocprim::plus<uint64_t>(), s);
}

size_t ufrag_segs_scratch_bytes(uint64_t nf) { return nf * (3 * 8 + 4 * 4) + 256; }

hipError_t launch_ufrag_segs(const UfragGraph &g, int k, int n_ranks, void *scratch, size_t scratch_bytes, void *tmp,
                             size_t tmp_bytes, uint64_t *seg_pos, unsigned long long *glen, hipStream_t s) {
  if (!g.nf) return hipSuccess;
  if (scratch_bytes < ufrag_segs_scratch_bytes(g.nf) || n_ranks < 1 || n_ranks > 255) return hipErrorInvalidValue;
  const uint64_t nf = g.nf;
  uint64_t *len = (uint64_t *)scratch, *slen = len + nf, *scanned = slen + nf;
  uint32_t *key = (uint32_t *)(scanned + nf), *skey = key + nf, *ident = skey + nf, *order = ident + nf;
  hipError_t e;
  k_ufrag_segs<<<grid_for(nf), U_THREADS, 0, s>>>(g, k, n_ranks, key, len, ident, glen);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the segments grouped by (sender, owner), in fragment order inside a group: the order both sides derive
  if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, key, skey, ident, order, (size_t)nf, 0, 16, s)) != hipSuccess) return e;
  k_ufrag_take<<<grid_for(nf), U_THREADS, 0, s>>>(order, len, nf, slen);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = rocprim::exclusive_scan(tmp, tmp_bytes, slen, scanned, (uint64_t)0, (size_t)nf, rocprim::plus<uint64_t>(), s)) !=
      hipSuccess)
    return e;
  k_ufrag_put<<<grid_for(nf), U_THREADS, 0, s>>>(order, scanned, nf, seg_pos);
  return hipGetLastError();
}

hipError_t launch_ufrag_rows(const OutRows &t, uint64_t n, int k, int nl, int nlo, uint32_t *row_ctg, uint32_t *row_pos,
                             uint8_t *row_rc, const uint32_t *lf_open, const uint32_t *lf_ctg, uint64_t n_frag, uint64_t f0,
                             uint64_t n_open, const UfragGraph &g, int me, uint64_t first_id, uint64_t n_ctgs,
                             const uint64_t *offsets, const uint32_t *n_kmers, uint64_t n_bases, char *seqs,
                             const uint64_t *seg_pos, uint64_t seg_base, uint64_t send_bytes, char *send, hipStream_t s) {
  if (!n) return hipSuccess;
  if (nlo < nl || k / 32 + 1 != nl || k % 32 == 0) return hipErrorInvalidValue;
  const unsigned gr = grid_for(n);
#define MHM_UFRAG_ROWS(NL)                                                                                               \
  k_ufrag_rows<NL><<<gr, U_THREADS, 0, s>>>(t, n, k, nlo, row_ctg, row_pos, row_rc, lf_open, lf_ctg, n_frag, f0, n_open, g, \
                                            (uint32_t)me, first_id, n_ctgs, offsets, n_kmers, n_bases, seqs, seg_pos,      \
                                            seg_base, send_bytes, send)
  switch (nl) {
    case 1: MHM_UFRAG_ROWS(1); break;
    case 2: MHM_UFRAG_ROWS(2); break;
    case 3: MHM_UFRAG_ROWS(3); break;
    case 4: MHM_UFRAG_ROWS(4); break;
    default: return hipErrorInvalidValue;
  }
#undef MHM_UFRAG_ROWS
  return hipGetLastError();
}

hipError_t launch_ufrag_scatter(const UfragGraph &g, int k, int me, int n_ranks, uint64_t first_id, uint64_t n_ctgs,
                                const uint64_t *offsets, uint64_t n_bases, char *seqs, const uint64_t *seg_pos,
                                const uint64_t *recv_base, const char *recv, uint64_t recv_bytes, hipStream_t s) {
  if (!g.nf || !recv_bytes || !n_ctgs) return hipSuccess;
  k_ufrag_scatter<<<grid_for(g.nf * 64), U_THREADS, 0, s>>>(g, k, (uint32_t)me, n_ranks, first_id, n_ctgs, offsets, n_bases,
                                                             seqs, seg_pos, recv_base, recv, recv_bytes);
  return hipGetLastError();
}

}  // namespace mhm
