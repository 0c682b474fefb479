// The route to a round's FASTA file and assembly statistics that exists without mhmkc_uutigs_fasta / mhmkc_uutigs_stats,
// timed for tools/fasta_bench.py in its process: the contig arrays fetched to the host (mhmkc_uutigs_fetch), a Contig
// object with its std::string per contig, then the adapter's plain host loops on one thread (include/mhmkc_kcount.hpp:
// dump_contigs, which formats with to_string as Contigs::dump_contigs does, and ctg_stats). Not part of the library.
//   int mhmkc_fhost(mhmkc_t h, unsigned min_ctg_len, const char *path, double *ms /*[4]*/, mhmkc_ctg_stats *st)
// ms: 0 mhmkc_uutigs_fetch, 1 the Contig objects, 2 dump_contigs into `path`, 3 ctg_stats. Returns 0, or -1 on a library
// error.
#include <chrono>
#include <vector>

#include "mhmkc_kcount.hpp"

extern "C" int mhmkc_fhost_abi(void) { return MHMKC_ABI_VERSION; }

extern "C" int mhmkc_fhost(mhmkc_t h, unsigned min_ctg_len, const char *path, double *ms, mhmkc_ctg_stats *st) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  if (!path || !ms || !st) return -1;
  uint64_t n_ctgs = 0, n_bases = 0;
  if (mhmkc_uutigs(h, &n_ctgs, &n_bases) != MHMKC_OK) return -1;
  auto t = clk::now();
  std::vector<uint64_t> offs(n_ctgs + 1);
  std::vector<char> seqs(n_bases);
  std::vector<double> depths(n_ctgs);
  if (mhmkc_uutigs_fetch(h, offs.data(), seqs.data(), depths.data(), nullptr) != MHMKC_OK) return -1;
  ms[0] = since(t);
  t = clk::now();
  mhm2::Contigs ctgs;
  ctgs.reserve(n_ctgs);
  for (uint64_t c = 0; c < n_ctgs; c++)
    ctgs.push_back(mhm2::Contig{(int64_t)c, std::string(seqs.data() + offs[c], seqs.data() + offs[c + 1]), depths[c]});
  ms[1] = since(t);
  t = clk::now();
  mhm2::dump_contigs(ctgs, path, min_ctg_len);
  ms[2] = since(t);
  t = clk::now();
  *st = mhm2::ctg_stats(ctgs, min_ctg_len);
  ms[3] = since(t);
  return 0;
}
