// The host half of the contigs' wire format between ranks (mhm2_proxy_amd/csrc/kmer_ops.hpp: ctg_nib4, ctg_nib8), the
// functions k_ctgx_pack runs on the GPU, against their plainest statement, and the round trip through the rule
// k_expand_nibbles restores the bytes with. No GPU.
//   ctg_nib_check      prints "ok" and exits 0, or the first mismatches and exits 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mhm2_proxy_amd/csrc/kmer_ops.hpp"

// k_expand_nibbles' rule (kcount_kernels.hip)
static uint8_t expand(uint32_t v) { return (uint8_t)((v & 7u) | ((v >> 3) * 0xf8u)); }

int main() {
  int bad = 0;
  // the ten bytes a contig character becomes (ctg_byte): code 0..4, quality 31 or 0
  std::vector<uint8_t> vals;
  for (const char *p = "ACGTNacgtn"; *p; p++) {
    const int b = mhm::ctg_byte((uint8_t)*p);
    if (b < 0 || b > 255) {
      std::printf("ctg_byte('%c') = %d\n", *p, b);
      return 1;
    }
    vals.push_back((uint8_t)b);
  }
  for (uint8_t v : vals)
    if (expand(v & 15u) != v) {
      if (bad++ < 10) std::printf("byte %02x: & 15 then the expand rule gives %02x\n", v, expand(v & 15u));
    }
  // every pair of the ten values in every pair of lanes of the eight, the other lanes taking a third value
  for (int la = 0; la < 8; la++)
    for (int lb = 0; lb < 8; lb++)
      for (uint8_t a : vals)
        for (uint8_t b : vals)
          for (uint8_t fill : {vals[0], vals[4], vals[8]}) {
            uint8_t in[8];
            for (int j = 0; j < 8; j++) in[j] = fill;
            in[la] = a;
            in[lb] = b;  // (lb == la: the later value stands)
            uint32_t lo, hi;
            std::memcpy(&lo, in, 4);
            std::memcpy(&hi, in + 4, 4);
            const uint32_t got = mhm::ctg_nib8(lo, hi);
            uint32_t want = 0;
            for (int j = 0; j < 8; j++) want |= (uint32_t)(in[j] & 15u) << (4 * j);
            if (got != want) {
              if (bad++ < 10) std::printf("lanes %d,%d bytes %02x,%02x fill %02x: %08x, want %08x\n", la, lb, a, b, fill, got, want);
            }
            for (int j = 0; j < 8; j++)
              if (expand((got >> (4 * j)) & 15u) != in[j]) {
                if (bad++ < 10) std::printf("lane %d of %08x does not expand to %02x\n", j, got, in[j]);
              }
            if (mhm::ctg_nib4(lo) != (want & 0xffffu) || mhm::ctg_nib4(hi) != (want >> 16)) {
              if (bad++ < 10) std::printf("ctg_nib4 halves of %08x %08x\n", lo, hi);
            }
          }
  // a packed buffer as the kernel lays it out: byte i of the nibbles holds source bytes 2i (low half) and 2i + 1
  uint8_t src[16], dst[8], ref[8];
  for (int i = 0; i < 16; i++) src[i] = vals[(size_t)(i * 7 + 3) % vals.size()];
  for (int i = 0; i < 8; i++) ref[i] = (uint8_t)((src[2 * i] & 15u) | ((src[2 * i + 1] & 15u) << 4));
  uint32_t x[4], o[2];
  std::memcpy(x, src, 16);
  o[0] = mhm::ctg_nib8(x[0], x[1]);
  o[1] = mhm::ctg_nib8(x[2], x[3]);
  std::memcpy(dst, o, 8);
  if (std::memcmp(dst, ref, 8) != 0) {
    bad++;
    std::printf("16 bytes -> 8: the byte order differs from one pair per byte, low half first\n");
  }
  if (bad) {
    std::printf("FAILED %d\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
