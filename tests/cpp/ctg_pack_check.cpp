// The host halves of the device contig input (mhm2_proxy_amd/csrc/kmer_ops.hpp: ctg_byte, ctg_pack4, ctg_depth_u16),
// the functions k_ctg_pack and k_ctgin_contigs run on the GPU, against their plainest statements. No GPU.
//   ctg_pack_check      prints "ok" and exits 0, or the first mismatches and exits 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../mhm2_proxy_amd/csrc/kmer_ops.hpp"

// mhmkc_add_ctgs's per-character conversion (seq_byte, mhmkc_host.cpp), restated
static int plain_byte(int c) {
  int code;
  switch (c) {
    case 'A': case 'a': code = 0; break;
    case 'C': case 'c': code = 1; break;
    case 'G': case 'g': code = 2; break;
    case 'T': case 't': code = 3; break;
    case 'N': case 'n': code = 4; break;
    default: return -1;
  }
  return code | ((c >= 'A' && c <= 'Z') ? (31 << 3) : 0);
}

// Contig::get_uint16_t_depth (src/contigs.hpp:65), the expression itself
static uint16_t ref_depth(double depth) { return (uint16_t)(depth > 65535 ? 65535 : depth); }

int main() {
  int bad = 0;
  // every byte value in every lane, the other lanes taking every kind of neighbour (valid upper / lower, invalid, 0, 0xff)
  const uint8_t others[] = {'A', 'c', 'G', 't', 'N', 'n', 'T', 0, 0xff, 'B', '@', 0x7f, 0x80, 'a' ^ 0x80, ' '};
  for (int lane = 0; lane < 4; lane++)
    for (int c = 0; c < 256; c++)
      for (uint8_t o : others) {
        uint8_t in[4] = {o, o, o, o};
        in[lane] = (uint8_t)c;
        uint32_t x = 0;
        for (int j = 0; j < 4; j++) x |= (uint32_t)in[j] << (8 * j);
        uint32_t flags = 0;
        const uint32_t y = mhm::ctg_pack4(x, &flags);
        if (flags & ~0x80808080u) {
          if (bad++ < 10) std::printf("flags %08x of %08x: bits outside the lanes' top bits\n", flags, x);
        }
        for (int j = 0; j < 4; j++) {
          const int want = plain_byte(in[j]);
          const bool flagged = (flags >> (8 * j + 7)) & 1u;
          const int got = (int)((y >> (8 * j)) & 0xffu);
          if (flagged != (want < 0) || (want >= 0 && got != want)) {
            if (bad++ < 10) std::printf("lane %d of %08x: byte %d flagged %d, want %d\n", j, x, got, (int)flagged, want);
          }
        }
        if (mhm::ctg_byte((uint8_t)c) != plain_byte(c)) {
          if (bad++ < 10) std::printf("ctg_byte(%d) = %d, want %d\n", c, mhm::ctg_byte((uint8_t)c), plain_byte(c));
        }
      }
  const double inf = std::numeric_limits<double>::infinity();
  const double good[] = {0, 0.4, 0.999, 1, 1.999, 65534.9, 65535, 65535.5, 1e9, inf};
  const uint16_t want[] = {0, 0, 0, 1, 1, 65534, 65535, 65535, 65535, 65535};  // truncation toward zero, then the cap
  for (int i = 0; i < 10; i++) {
    bool ok = false;
    const uint16_t got = mhm::ctg_depth_u16(good[i], &ok);
    if (!ok || got != ref_depth(good[i]) || got != want[i]) {
      if (bad++ < 10) std::printf("depth %g -> %u ok %d, the reference's expression gives %u\n", good[i], got, (int)ok, ref_depth(good[i]));
    }
  }
  const double invalid[] = {-1e-9, -1, std::nan(""), -inf};
  for (double d : invalid) {
    bool ok = true;
    (void)mhm::ctg_depth_u16(d, &ok);
    if (ok) {
      if (bad++ < 10) std::printf("depth %g not flagged\n", d);
    }
  }
  if (bad) {
    std::printf("FAILED %d\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
