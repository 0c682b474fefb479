// Device functions shared by the query kernels (kcount_query.hip) and the routed queries between ranks
// (kcount_route.hip): the probe of the row index and the rules of mhmkc_dbjg_links (include/mhmkc.h), cut where a
// neighbour that lives on another rank has to be asked for. DESIGN.md §3.11, §3.11b.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mhmkc.h"

#include "kcount_launch.hpp"
#include "kmer_ops.hpp"

namespace mhm {

constexpr unsigned long long QSLOT_EMPTY = ~0ull;
constexpr uint32_t Q_NO_ROW = 0xFFFFFFFFu;

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

// The row holding key w (NL words, the unused bits zero), or Q_NO_ROW.
template <int NL>
__device__ __forceinline__ uint32_t find_row(const uint64_t *w, int nlo, const QueryIndex &ix, const uint64_t *keys) {
  const uint64_t h = key_hash<NL>(w, nlo);
  const uint32_t tag = (uint32_t)h;
  uint64_t s = h >> ix.shift;
  for (uint64_t probes = 0; probes <= ix.mask; probes++) {
    const unsigned long long v = ix.slots[s];
    const uint32_t row = (uint32_t)v;
    if (row == Q_NO_ROW) return Q_NO_ROW;
    if ((uint32_t)(v >> 32) == tag && (uint64_t)row < ix.n_rows) {
      bool eq = true;
#pragma unroll
      for (int j = 0; j < NL; j++) eq &= keys[(uint64_t)row * nlo + j] == w[j];
      if (eq) return row;
    }
    s = (s + 1) & ix.mask;
  }
  return Q_NO_ROW;
}

// w masked to k bases and, if asked, replaced by the smaller of itself and its reverse complement
template <int NL>
__device__ __forceinline__ void query_key(uint64_t *w, int k, int canonicalize) {
  w[NL - 1] &= top_mask(k - 32 * (NL - 1));
  if (canonicalize) {
    uint64_t rc[NL];
    revcomp<NL>(w, rc, k);
    if (kmer_less<NL>(rc, w)) {
#pragma unroll
      for (int j = 0; j < NL; j++) w[j] = rc[j];
    }
  }
}

__device__ __forceinline__ uint32_t base_code(char c) {  // set_kmer's bit trick (src/kmer.cpp:274-296)
  const uint32_t x = ((uint32_t)c & 4u) >> 1;
  return x + ((x ^ ((uint32_t)c & 2u)) >> 1);
}
__device__ __forceinline__ char base_char(uint32_t code) { return (char)((0x54474341u >> (8 * code)) & 0xffu); }
__device__ __forceinline__ char comp_char(char c) { return base_char(3u - base_code(c)); }

// Steps 1 and 2 of mhmkc_dbjg_links for row i in direction right_dirn. False: the row's own extensions end the entry
// and st is its status (nothing is looked up). True: key is the k-mer to look up (the smaller of the neighbour and its
// reverse complement), is_rc says which of the two it is, back_check the base the neighbour's extension must lead
// back to.
template <int NL>
__device__ __forceinline__ bool link_neighbour(const OutRows &t, uint64_t i, bool right_dirn, int k, int nlo,
                                               uint64_t *key, bool &is_rc, uint32_t &back_check, uint8_t &st) {
  const char l = t.left[i], r = t.right[i];
  if (l == 'X' || r == 'X') {
    st = MHMKC_LINK_DEADEND;
    return false;
  }
  if (l == 'F' || r == 'F') {
    st = MHMKC_LINK_FORK;
    return false;
  }
  uint64_t w[NL], nb[NL], rc[NL];
  load_key<NL>(t.keys, i, nlo, w);
  const int kl = k - 32 * (NL - 1);  // bases in the last word
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
  is_rc = kmer_less<NL>(rc, nb);
#pragma unroll
  for (int j = 0; j < NL; j++) key[j] = is_rc ? rc[j] : nb[j];
  st = MHMKC_LINK_OK;
  return true;
}

// Step 3: the status of an entry whose neighbour is in the table with the stored extensions jl / jr.
__device__ __forceinline__ uint8_t link_verdict(char jl, char jr, bool is_rc, bool right_dirn, uint32_t back_check) {
  if (jl == 'X' || jr == 'X') return MHMKC_LINK_DEADEND;
  if (jl == 'F' || jr == 'F') return MHMKC_LINK_FORK;
  if (is_rc) {
    const char tmp = jl;
    jl = comp_char(jr);
    jr = comp_char(tmp);
  }
  const char want = base_char(back_check);
  const bool ok = right_dirn ? jl == want : jr == want;
  return ok ? (uint8_t)(MHMKC_LINK_OK | (is_rc ? MHMKC_LINK_RC : 0)) : (uint8_t)MHMKC_LINK_CONFLICT;
}

}  // namespace mhm
