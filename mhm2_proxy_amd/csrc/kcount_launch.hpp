// Launch interface between the host orchestration (mhmkc_host.cpp) and the gfx950 kernels
// (kcount_kernels.hip). Plain structs of device pointers; no torch types anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mhm {

// Read stream in the PackedRead byte layout (src/packed_reads.cpp:73-109) + CSR offsets.
// A view may be a slice of a larger batch (one H2D chunk, mhmkc_add_reads): its offsets are then the
// batch's, and obase (<= offs[0], 16-byte aligned in the batch) is subtracted from them; bytes points
// at batch byte obase. Positions [0, head) belong to the previous slice's last read and hold no window.
struct ReadsView {
  const uint8_t *bytes;   // n_bases bytes: code (bits 0-2) | min(q-off,31) << 3
  const uint64_t *offs;   // n_reads+1 offsets, offs[n_reads] - obase = n_bases
  uint64_t n_reads;
  uint64_t n_bases;
  uint64_t obase;         // subtracted from every offset (0 for a whole batch)
  uint32_t head;          // offs[0] - obase (< 16)
  uint32_t pad;
};

// Record planes of one slab: word planes (SoA) + optional ext byte plane.
struct PlaneSet {
  uint64_t *w[4];
  uint8_t *ext;  // nullptr when the ext code is packed into the last key word
};

struct ExtractParams {
  ReadsView reads;
  const uint32_t *tile_first_read;  // per tile: first read r with offs[r] >= tile_lo
  uint32_t n_tiles;
  int k;
  int qual_cutoff;
  int coarse_bits;                  // coarse digit = h1 >> (64 - coarse_bits)
  uint32_t n_bins;                  // 1 << coarse_bits
  int hbits;                        // hash bits stored in the record after the ext code (0: none)
  int compact;                      // mixed records: compact (NL = 1, kmer_ops.hpp cmix): out = u32 plane w[0] +
                                    // byte plane ext; NL = 2: m2_mix records, two u64 planes
  unsigned long long *hist;         // [n_bins] (E-hist)
  unsigned long long *cursor;       // [E_NSUB * n_bins] (E-scatter): cursor of segment (b, s) at s * n_bins + b
  uint64_t bin_cap;                 // capped mode: segment (b, s) owns [i*bin_cap, (i+1)*bin_cap), i = b*E_NSUB+s,
                                    // s = blockIdx % E_NSUB; 0 = exact bases, everything in segment (b, 0)
  PlaneSet out;                     // (E-scatter)
  unsigned int *err;                // bit 0: input byte with code > 4
  unsigned int *ovf;                // bit 1: a capped bin of this slab overflowed (per slab)
  const uint32_t *tile_starts;      // the batch's flat read-start bits (k_read_start_bits; tile t's groups are words
                                    // [t tile / 32, t tile / 32 + kGroups)), or nullptr:
                                    // load_tile builds it from the offsets
  uint32_t bin_lo, bin_hi;          // k_smer_extract: only records of coarse bins [bin_lo, bin_hi) are kept (a finish
                                    // pass over part of the hash range); 0, n_bins = all
};

constexpr int SMER_SLICES = 64;  // counter slices per destination (spread the workgroups' atomics)
// Supermer exchange (kcount_kernels.hip). Sender side, per read slab: owners and per-destination
// counts (k_smer_owner), then the supermers packed into exact per-destination spans (k_smer_pack).
struct SmerParams {
  ReadsView reads;
  const uint32_t *tile_first_read;
  uint32_t n_tiles;
  int k, m, n_ranks, qual_cutoff;
  uint8_t *owners;              // [n_tiles * tile]: owner of the window at each tile position, 0xFF: not counted
  unsigned long long *hist;     // [n_ranks][SMER_SLICES][2]: words, supermers per destination and slice of tiles
                                // (tile % SMER_SLICES; k_smer_owner adds)
  unsigned long long *cursor;   // the same layout: word and supermer cursors (k_smer_pack)
  uint64_t *codes;              // supermer bases, 2-bit codes, 32 per word (MSB first)
  uint32_t *good;               // their "extension countable" bits, 32 per word
  uint64_t *desc;               // per supermer: first word << 16 | windows
  uint64_t n_words, n_smer;     // the planes' sizes (k_smer_pack writes nothing past them: err bit 3)
  unsigned int *err;
};
// Receiver side: the received supermers of every peer back to back (descriptors rebased), their window prefix
// wpre[n_smer + 1], and per tile of window indices the supermer holding its first window.
struct SmerSource {
  const uint64_t *codes;
  const uint32_t *good;
  const uint64_t *desc;
  const uint64_t *wpre;
  const uint64_t *tile_first;   // [n_tiles + 1]
  uint64_t n_smer, n_windows;
  uint64_t n_words;             // code / good words (a window reaching past them is not read: err bit 3)
};
hipError_t launch_smer_owner(const SmerParams &p, int nl, hipStream_t s);
hipError_t launch_smer_pack(const SmerParams &p, int nl, hipStream_t s);
// records of the received supermers into a coarse slab (p.out / p.cursor as launch_extract_scatter), or (hist) the
// exact bin histogram into p.hist
hipError_t launch_smer_extract(const ExtractParams &p, const SmerSource &src, int nl, bool packed, bool hist,
                               hipStream_t s);
// descriptors of a received span: word offsets += delta (mod 2^64), nwin[i] = windows of supermer i
hipError_t launch_smer_rebase(uint64_t *desc, uint64_t n, uint64_t delta, unsigned long long *nwin, hipStream_t s);
hipError_t launch_smer_tiles(const uint64_t *wpre, uint64_t n_smer, uint64_t *tile_first, uint32_t n_tiles, int tile,
                             hipStream_t s);

// One chunk of S work: <= tile records of one (source, coarse bucket) segment.
struct SChunk {
  uint64_t start;        // first record index in the source planes
  uint32_t count;        // records in the chunk
  uint32_t src;          // index into the source plane-set table
  uint32_t coarse_local; // coarse bucket index relative to this rank's first owned bucket
  uint32_t pad;
};

// A run = one non-empty (source, segment) span, cut into tile-sized chunks; chunk0 = its first chunk.
struct SRun {
  uint64_t start, count;
  uint32_t src, coarse_local;
  uint32_t chunk0, pad;
};

struct PartitionParams {
  const SRun *runs;                 // [n_runs]
  const SChunk *chunks;             // [n_chunks]: each chunk's span (launch_chunk_runs expands the runs into them)
  uint32_t n_runs;
  uint32_t n_chunks;
  // XCD-aware launch: the chunks are ordered by XCD class (coarse bucket % 8); class x holds chunks
  // [xcd_start[x], xcd_start[x + 1]) and is served by the workgroups b with b % 8 == x (grid = 8 * largest)
  uint32_t xcd_start[9];
  uint32_t grid;
  const PlaneSet *srcs;           // device table of source plane sets
  int k;
  int coarse_bits;
  int fine_bits;
  int hbits;                        // hash bits stored in the records (fine digit read from them if >= fine_bits)
  int compact;                      // mixed records (see ExtractParams): compact sources u32 + byte planes, out
                                    // one u32 plane; NL = 2: two u64 planes in and out
  unsigned long long *fine_hist;    // [n_coarse_local << fine_bits]
  unsigned long long *fine_cursor;  // [n_coarse_local << fine_bits]
  const unsigned long long *coarse_base;  // capped mode: first fine bucket of coarse bucket c starts here
  const unsigned long long *coarse_fcap;  // capped mode: capacity of every fine bucket of c; nullptr = exact
  unsigned int *err;                      // bit 1: a capped fine bucket overflowed
  PlaneSet out;
};

struct CountParams {
  PlaneSet recs;                      // fine-bucketed records (overwritten in place by overflow)
  const unsigned long long *bucket_base;
  const unsigned long long *bucket_end;  // == the fine cursors after the scatter
  int hbits;                           // stored hash bits to strip from the last key word
  int compact;                         // mixed records (compact u32 plane w[0], or NL = 2 m2_mix words); the key
                                       // is rebuilt from the bucket digits
  int coarse_bits, fine_bits;
  uint32_t bucket0;                    // global index of local fine bucket 0 (own_lo << fine_bits)
  uint32_t n_buckets;
  uint32_t grid;                      // persistent workgroups (one per CU); 0 = one per bucket
  int k;
  int cap;                            // LDS table slots
  int dmin_thres;
  double dyn_mult;                    // 1.0 - DYN_MIN_DEPTH, computed in double on the host
  int wide_thr;                       // (int)(dyn_mult * 65535) > 0x8000: a threshold can pass the extension counters'
                                      // clamp target, so every clamp is logged and undone at the decision (§3.4)
  int nlo;                            // output words per key
  uint64_t *out_keys;                 // [out_cap * nlo]
  uint16_t *out_counts;
  char *out_left;
  char *out_right;
  unsigned long long *out_cursor;
  unsigned long long out_cap;         // output rows allocated: a reservation past it sets err bit 4 (16) and writes
                                      // nothing (the cursor still counts, so the host learns the size and redoes the pass)
  unsigned long long *stats;          // [STAT_*]
  unsigned int *err;                  // k_part_scatter's flag word: bit 1 set = a capped fine bucket overflowed,
                                      // its cursor ran past the bucket, so the launch is void (returns at once)
  // contig pass (kcount_ctg.hip): folded contig k-mers sorted by bucket; 0 entries = no contig pass
  uint64_t ctg_n;
  const uint64_t *ctg_keys[4];        // [NL][ctg_n] canonical key words
  const uint32_t *ctg_state;          // count (16 bits) | left code << 16 | right code << 19
  const uint32_t *ctg_bucket;         // local fine bucket of each entry (sorted ascending)
  uint32_t ctg_base;                  // local fine bucket of this launch's bucket 0 (a finish pass over part of the
                                      // owned range: its first coarse bucket << fine_bits)
  PlaneSet spill;                     // deferred records of cold sweeps: SPILL_RECORDS per workgroup (fine record
                                      // layout; planes of grid * SPILL_RECORDS entries); w[0] == nullptr: none
  uint8_t *ctg_done;                  // [ctg_n] applied (zeroed before the launch)
  const uint8_t *coarse_skip;         // [n_buckets >> fine_bits] or null: a local coarse bucket whose fine buckets are
                                      // counted by a later launch (k_inc_fixup emptied them): no contig k-mers here
};

// Contig pass state word of one folded contig k-mer (kcount_ctg.hip).
__host__ __device__ inline uint32_t ctg_state_word(uint32_t count, uint32_t l, uint32_t r) {
  return (count & 0xffffu) | (l << 16) | (r << 19);
}

// Input of the contig-pass extraction: contigs in the PackedRead byte layout (case -> quality 31 / 0).
struct CtgView {
  const uint8_t *bytes;
  const uint64_t *offs;        // [n_ctgs + 1]
  const uint16_t *depth;       // [n_ctgs]: Contig::get_uint16_t_depth() (0 counts as 1)
  const uint64_t *win_prefix;  // [n_ctgs + 1]: counted windows before each contig
  uint64_t n_ctgs;
  uint64_t n_windows;
};

// Owner filter of the contig pass with the supermer exchange: keep the k-mers whose get_kmer_target_rank
// (quick_hash(minimizer_fast(m)) % n_ranks) is `rank`; n_ranks = 0: no filter.
struct CtgOwner {
  int n_ranks, rank, m;
};

// Contig pass (kcount_ctg.hip). Scratch sizes come from ctg_scratch_bytes.
size_t ctg_scratch_bytes(uint64_t n_windows, int nl);
// Extract, sort by key (stable: contig order kept within a key), fold every key's contig occurrences in
// order (insert_supermer_from_ctg) and sort the folded k-mers by local fine bucket. Outputs (n_out of them)
// go to out_keys[NL] (SoA, each out_cap long), out_state, out_bucket.
// Only k-mers whose coarse bucket is in [own_lo, own_hi) (this rank's hash range) are kept.
hipError_t ctg_prepare(const CtgView &cv, int k, int nl, bool mixed, int qual_cutoff, int dmin_thres,
                       double dyn_mult, int coarse_bits, int fine_bits, uint32_t own_lo, uint32_t own_hi,
                       const CtgOwner &ow, void *scratch, size_t scratch_bytes,
                       uint64_t *const out_keys[4], uint32_t *out_state, uint32_t *out_bucket, uint64_t *n_out,
                       unsigned int *err, hipStream_t s);

// Contigs that are already on the device (kcount_ctgin.hip: mhmkc_add_ctgs_device, mhmkc_add_ctgs_from): ASCII bases,
// offsets and depths are converted into the arrays of a CtgView, appended to what the round holds. What the kernels
// find goes to a mailbox the host reads once per call.
struct CtgInBox {
  unsigned long long bad_pos;    // first byte outside ACGTNacgtn (~0: none)
  unsigned long long bad_off;    // first contig whose end offset is below its start (~0: none)
  unsigned long long bad_depth;  // first contig with a NaN or negative depth (~0: none)
  unsigned long long windows;    // the round's counted windows with this batch
  unsigned long long first_off, last_off;  // offs[0], offs[n_ctgs]
};
// Workgroups of the packing kernel's grid-stride launch. The test knob ctg_pack_grid (include/mhmkc_debug.h) caps them at
// ctg_pack_grid_cap, so that a lane takes several vectors in turn on a small batch; 0, the product's value: its own grid.
inline unsigned ctg_pack_grid_cap = 0;
size_t ctgin_tmp_bytes(uint64_t n_ctgs);
// seqs[n_bases], offs[n_ctgs + 1], depths[n_ctgs] (double when depth_f64, else uint16_t) -> out_bytes[n_bases] (the
// PackedRead bytes, at any byte address), out_offs[0..n_ctgs] = b0 + offs, out_win[0..n_ctgs] = w0 + the windows before
// each contig, out_depth[n_ctgs]; out_offs / out_win / out_depth point at the round's first free entry. Nothing is read
// through offs but the offsets themselves, so a bad CSR costs no out-of-bounds access: the mailbox names it.
hipError_t launch_ctgin(const char *seqs, const uint64_t *offs, const void *depths, bool depth_f64, uint64_t n_ctgs,
                        uint64_t n_bases, int k, uint64_t b0, uint64_t w0, uint8_t *out_bytes, uint64_t *out_offs,
                        uint64_t *out_win, uint16_t *out_depth, void *tmp, size_t tmp_bytes, CtgInBox *box, hipStream_t s);

// The contigs of several ranks gathered on the device (kcount_ctgx.hip). What the kernels find goes to
// a mailbox the host reads once per gather.
struct CtgxBox {
  unsigned long long bad_rank;  // lowest rank whose lengths do not sum to the bytes it announced (~0: none)
  unsigned long long long_ctg;  // first contig of this rank with 2^32 or more bytes (~0: none)
  unsigned long long windows;   // the counted windows of the gathered lengths
};
// Workgroups of the gather kernels' grid-stride launches. The test knob ctgx_grid (include/mhmkc_debug.h) caps them at
// ctgx_grid_cap, so that their loops turn several times on a small set; 0, the product's value: their own grids.
inline unsigned ctgx_grid_cap = 0;
hipError_t launch_ctgx_begin(CtgxBox *box, hipStream_t s);
// This rank's wire format: lens[n_ctgs] = offs[i + 1] - offs[i] as u32, nib[(n_bytes + 1) / 2] = the nibbles of
// bytes[n_bytes] (bytes 16-byte aligned, nib 8-byte aligned: the starts of their buffers).
hipError_t launch_ctgx_pack(const uint64_t *offs, uint64_t n_ctgs, const uint8_t *bytes, uint64_t n_bytes, uint32_t *lens,
                            uint8_t *nib, CtgxBox *box, hipStream_t s);
size_t ctgx_tmp_bytes(uint64_t n_all);
// lens[n_all], every rank's in rank order -> offs[n_all + 1] (byte offsets), win[n_all + 1] (counted-window prefix);
// tab[2 (g + 1)] = the ranks' first contigs, then their first bytes, as announced (device memory): the mailbox names a
// rank whose lengths do not sum to its bytes. No index comes from lens.
hipError_t launch_ctgx_assemble(const uint32_t *lens, uint64_t n_all, int k, const uint64_t *tab, int g, uint64_t *offs,
                                uint64_t *win, void *tmp, size_t tmp_bytes, CtgxBox *box, hipStream_t s);

enum {
  STAT_DISTINCT = 0,
  STAT_NOUT = 1,
  STAT_PURGED = 2,
  STAT_COUNTSUM = 3,
  STAT_SWEEPS = 4,
  STAT_MAXBUCKET = 5,
  STAT_MISSES = 6,    // records worked off in phase B (not in their home group)
  STAT_N = 8,         // stats[STAT_N - 1]: internal error flag
};
constexpr int STAT_ALLOC = 16;
// k_count's cold sweeps (< 0xC000 records) hand their waves the rounds' record slots dynamically; their deferred
// records go to a per-workgroup spill area of this many records (and from there back to the bucket's own region)
constexpr uint32_t SPILL_RECORDS = 0xC000;  // stats[8..13]: k_count phase stamps in MHMKC_STAMP builds
// ... for keys of at most this many words (with three and four key words the dynamic instantiation spilled 20-40 VGPRs
// and made k_count 10-22 % slower): the host allocates the spill area only for them
constexpr int DYN_SWEEP_MAX_NL = 2;

// Workgroup shapes (each measured against its neighbours on MI355X).
constexpr int E_THREADS = 256;  // default threads of the extract / partition workgroups
constexpr int E_NSUB = 8;       // segments per coarse bucket: one per group of workgroups sharing an XCD
// k_count: one persistent 1024-thread workgroup per CU with all 160 KB of LDS (two 512-thread workgroups with half
// the LDS each measured slower once the fine partition's cost is counted, §4.2). MHMKC_CSPLIT=2 builds (A/B variants
// only) run that split: C_SPLIT workgroups per CU, each with 1/C_SPLIT of the threads, the LDS and the table.
#ifndef MHMKC_CSPLIT
#define MHMKC_CSPLIT 1
#endif
constexpr int C_SPLIT = MHMKC_CSPLIT;
constexpr int C_THREADS = 1024 / C_SPLIT;
constexpr size_t C_LDS = 163840 / C_SPLIT;

// Hash bits stored in a packed record next to the ext code (bits [6, 6 + hbits) of the last word).
inline int stored_hash_bits(int k, int nl, bool packed) {
  if (!packed) return 0;
  const int room = 64 - 2 * (k - 32 * (nl - 1)) - 6;
  return room >= 16 ? 16 : (room >= 8 ? room : 0);
}

// Bases per extract tile, by key words. Two-word keys: 4096-base tiles of 16 windows per thread (78 KB of LDS before
// the capped stage, two workgroups per CU) measured faster than 2048 (k = 63 extract 9.29 -> 8.52 ms). Three-word
// keys: 1536-base tiles, so that the staged 24-byte records of three workgroups fit a CU's LDS (2048: k = 77 14.70 ->
// 13.05 ms); four-word keys keep 2048 (1536: 16.08 -> 19.09 ms).
constexpr int TILE_BASES[5] = {0, 4096, 4096, 1536, 2048};
inline int tile_bases(int nl) { return TILE_BASES[nl]; }
// threads of an extract workgroup (tile_bases / threads windows each); four-word keys: 8 windows per thread at 256
// threads and 128 VGPRs fit four workgroups per CU (512 threads: 13.23 ms, 256: 10.04 ms at k = 99)
constexpr int E_THREADS_NL[5] = {0, 256, 256, 256, 256};
// records per partition chunk and threads per partition workgroup; two-, three- and four-word keys take longer chunks
// over more threads (the chunk's runs per fine bucket grow, the LDS per wave stays; four-word: the staged chunk + 2048
// bins' counters fit 160 KB; two-word 3072 over 512: k = 63 5.59 -> 5.50 ms, k = 33 7.49 -> 7.33)
constexpr int P_TILE[5] = {0, 4096, 3072, 4096, 3072};
constexpr int P_THREADS[5] = {0, 256, 512, 512, 512};
inline int chunk_records(int nl) { return P_TILE[nl]; }
// LDS hash-table slots of the count kernel for NL words per key (~143 KB of LDS); compact records keep
// 32-bit keys (the stored bits of the mixed key), 24 bytes per slot instead of 28.
// k_count LDS: table (keys, count, 4 extension words per slot) + 192 B of scalars + the miss queues of the waves
// (key words + ext code per entry); together <= 160 KiB. Two-word keys: 3800 / 4200 slots measured slower than 4000,
// three / four-word keys 2880 / 2400 slower than 3264 / 2752 (§4.2).
constexpr int COUNT_CAP[5] = {0, 5120, 4000, 3264, 2752};
__host__ __device__ constexpr int count_key_bytes(bool cmp) { return cmp ? 4 : 8; }
__host__ __device__ constexpr int count_cap(int nl, bool cmp = false) {
  return ((cmp ? 6144 : COUNT_CAP[nl]) / C_SPLIT) & ~3;
}
__host__ __device__ constexpr size_t count_table_bytes(int nl, bool cmp = false) {
  return (size_t)count_cap(nl, cmp) * (count_key_bytes(cmp) * nl + 4 + 16) + 256;  // + k_count's scalars
}
__host__ __device__ constexpr int miss_cap(int nl, bool cmp = false) {
  return (int)(((C_LDS - count_table_bytes(nl, cmp)) / (count_key_bytes(cmp) * nl + 4)) & ~(size_t)63);
}
// the clamp log (CountParams.wide_thr, §3.4) follows the miss queues: CLAMP_LOG words (slot << 3 | half) << 16 | the
// amount the clamps took from that half, saturating; miss_cap rounds down to 64 entries, which leaves the room
constexpr int CLAMP_LOG = 64;
__host__ __device__ constexpr size_t count_log_offset(int nl, bool cmp = false) {
  return count_table_bytes(nl, cmp) + (size_t)miss_cap(nl, cmp) * (count_key_bytes(cmp) * nl + 4);
}
__host__ __device__ constexpr size_t count_lds_bytes(int nl, bool cmp = false) {
  return count_log_offset(nl, cmp) + 4 * (size_t)CLAMP_LOG;
}
static_assert(count_lds_bytes(1) <= C_LDS && count_lds_bytes(2) <= C_LDS && count_lds_bytes(3) <= C_LDS &&
                  count_lds_bytes(4) <= C_LDS && count_lds_bytes(1, true) <= C_LDS,
              "k_count LDS budget");

hipError_t launch_tile_first_read(const ReadsView &r, uint32_t *out, uint32_t n_tiles, int tile, hipStream_t s);
// the batch's read-start bits for the extraction (read_start_words(n_tiles, nl) u32, every word written):
// ExtractParams tile_starts
hipError_t launch_read_start_bits(const ReadsView &r, uint32_t *bits, uint64_t n_words, hipStream_t s);
uint64_t read_start_words(uint64_t n_tiles, int nl);
// total counted windows sum(max(0, L - k - 1)) of a batch, added to *out; err bit 2 (4) when the offsets are
// not a valid PackedReads CSR (offs[0] != 0, decreasing, a read longer than 65535, offs[n] != n_bases)
hipError_t launch_count_windows(const ReadsView &r, int k, unsigned long long *out, unsigned int *err, hipStream_t s);
// one H2D chunk of a host batch sent as nibbles (code | (q >= qcut) << 3, two per byte): arena[b0, b0 + n) as PackedRead
// bytes again (code | (q >= qcut ? 31 : 0) << 3)
hipError_t launch_expand_nibbles(const uint8_t *nib, uint8_t *arena, uint64_t b0, uint64_t n, hipStream_t s);
// offs[i] = b0 + d[i], i < n: a chunk's offsets from the u32 distances the nibble H2D sends
hipError_t launch_offs_from_deltas(const uint32_t *d, uint64_t *offs, uint64_t n, uint64_t b0, hipStream_t s);
// capped fine layout: base/cursor of bucket (c, d) = coarse_base[c] + d * coarse_fcap[c]
// The incremental layout after its last round: a coarse bucket with a fine bucket past its capped
// segment (k_part_scatter wrote none of that bucket's overflowing runs) gets skip[c] = 1 and all its fine buckets
// emptied (cursor = base), so k_count counts the others and the host redoes just the skipped coarse buckets; err bit 1
// (the overflow flag, which would void the k_count launch) is cleared.
hipError_t launch_inc_fixup(const unsigned long long *coarse_base, const unsigned long long *coarse_fcap,
                            uint32_t n_coarse, int fine_bits, unsigned long long *cursor, uint8_t *skip,
                            unsigned int *err, hipStream_t s);
hipError_t launch_init_fine(const unsigned long long *coarse_base, const unsigned long long *coarse_fcap,
                            uint32_t n_coarse, int fine_bits, unsigned long long *base, unsigned long long *cursor,
                            hipStream_t s);
hipError_t launch_extract_hist(const ExtractParams &p, int nl, bool packed, hipStream_t s);
hipError_t launch_extract_scatter(const ExtractParams &p, int nl, bool packed, hipStream_t s);
// chunk_run[c] for every chunk of the runs (one workgroup per run)
hipError_t launch_chunk_runs(const SRun *runs, uint32_t n_runs, SChunk *chunks, int tile, hipStream_t s);
hipError_t launch_part_hist(const PartitionParams &p, int nl, bool packed, hipStream_t s);
hipError_t launch_part_scatter(const PartitionParams &p, int nl, bool packed, hipStream_t s);
// HyperLogLog sketch of the distinct keys in chunks [0, n_chunks) of p's chunk table (one coarse bucket):
// hll[SKETCH_M] registers, max-merged, and hll[SKETCH_M] += the records' extension adds; hll[SKETCH_M + 1 ..
// 2 SKETCH_M + 1) the registers of the even-numbered chunks alone (a second sample point for the growth of the distinct
// keys with the records). Zero all 2 SKETCH_M + 1 words first. fine_hist (p.fine_bits =
// SKETCH_FB): also the records per fine digit, hll[SKETCH_WORDS ..) (SKETCH_FH more words, zeroed too), from which the
// incremental layout learns how unevenly the records fall on fine buckets (a key's copies all land in one).
constexpr int SKETCH_M = 1024;
constexpr int SKETCH_WORDS = 2 * SKETCH_M + 1;
constexpr int SKETCH_FB = 11, SKETCH_FH = 1 << SKETCH_FB;
hipError_t launch_sketch(const PartitionParams &p, uint32_t n_chunks, unsigned int *hll, int nl, bool packed,
                         hipStream_t s, bool fine_hist = false);
hipError_t launch_scan(const unsigned long long *in, unsigned long long *base, unsigned long long *cursor,
                       uint32_t n, hipStream_t s);
hipError_t launch_count(const CountParams &p, int nl, bool packed, hipStream_t s);
// The exchange's send side: the filled part of every capped segment a peer owns, copied back to back into a dense
// send plane (a slab's owned range has up to the capped slack between its segments, which the wire need not carry).
// Elements of elem_bytes (1, 4, 8 or 16); segs in elements.
struct SegCopy {
  uint64_t src, dst, n;
};
hipError_t launch_seg_gather(const SegCopy *segs, uint32_t n_segs, const void *src, void *dst, int elem_bytes,
                             hipStream_t s);

// FASTQ ingest (fastq.hip): text -> PackedRead bytes. FQ_CHUNK bytes of text per count / lines block.
constexpr int FQ_CHUNK = 4096;
// longest line (without its newline) that the reference's fgets buffer reads whole (BUF_SIZE 2047,
// src/fastq.hpp:61)
constexpr uint64_t FQ_MAX_LINE = 2045;
// error kinds, in the order the reference checks them (src/fastq.cpp:525-547, packed_reads.cpp:104)
enum { FQ_E_ID = 1, FQ_E_PLUS = 2, FQ_E_NAME = 3, FQ_E_LEN = 4, FQ_E_LONG = 5, FQ_E_CHAR = 6, FQ_E_TRUNC = 7 };
// read-pair merging (merge_reads.cpp), reported at the pair's second record so that both records' own checks
// come first, in the reference's order: names, pair numbers, mate 2's revcomp, an overlap quality, mate 1's
// (or the merged read's) PackedRead
enum { FQ_E_PAIR_NAME = 8, FQ_E_PAIR_NUM = 9, FQ_E_CHAR2 = 10, FQ_E_QUAL = 11, FQ_E_CHAR1 = 12 };
size_t fq_scan_tmp_bytes(uint64_t n_items);
hipError_t fq_scan(void *tmp, size_t tmp_bytes, const unsigned long long *in, unsigned long long *out,
                   uint64_t n_items, hipStream_t s);
// newlines per FQ_CHUNK chunk -> chunk[ceil(n / FQ_CHUNK)]
hipError_t launch_fq_count(const char *text, uint64_t n, unsigned long long *chunk, hipStream_t s);
hipError_t launch_offs_rebase(unsigned long long *dst, const unsigned long long *src, uint64_t n, unsigned long long delta,
                              hipStream_t s);
// every newline, in order, from the scanned chunk counts, as one word per line: position (bits 0-39),
// trailing whitespace count of the line it ends (bits 40-55), first character of the next line (56-63)
constexpr int FQ_LE_BITS = 40;
constexpr uint64_t FQ_LE_MASK = (1ull << FQ_LE_BITS) - 1;
hipError_t launch_fq_lines(const char *text, uint64_t n, const unsigned long long *chunk_base,
                           unsigned long long *line_end, hipStream_t s);
// per record: sequence length (len[n_rec] = 0 for the scan) and format checks (err: atomicMin of
// record << 4 | FQ_E_*)
// paired input: k_fq_records' checks and the pair descriptors in one pass (launch_fq_merge reads the descriptors)
hipError_t launch_fq_pair_records(const char *text, uint64_t n, const unsigned long long *line_end, uint64_t n_rec,
                                  unsigned long long *len, unsigned long long *err, void *desc_buf, hipStream_t s);
hipError_t launch_fq_records(const char *text, uint64_t n, const unsigned long long *line_end, uint64_t n_rec,
                             unsigned long long *len, unsigned long long *err, hipStream_t s);
// pair p = records 2p, 2p+1: verdict in pair_info, output read lengths (merged + 1, or L1, L2) in out_len
// [2 n_pairs + 1]; stats[1..3] += merged pairs, ambiguous events, overlap bases. scratch: rec_offs[2 n_pairs]
// bytes (quality copies of pairs with an N).
// bytes of the per-pair line descriptors (desc_buf) of launch_fq_merge / launch_fq_merge_pack
size_t fq_pair_desc_bytes(uint64_t n_pairs);
hipError_t launch_fq_merge(const char *text, uint64_t n, const unsigned long long *line_end, uint64_t n_pairs,
                           const unsigned long long *rec_offs, int qual_offset, char *scratch, void *desc_buf,
                           uint32_t *pair_info, unsigned long long *out_len, unsigned long long *err,
                           unsigned long long *stats, hipStream_t s);
hipError_t launch_fq_merge_pack(const char *text, const void *desc_buf, uint64_t n_pairs,
                                const unsigned long long *rec_offs, const char *scratch, const uint32_t *pair_info,
                                const unsigned long long *out_offs, int qual_offset, uint8_t *out,
                                unsigned long long *err, hipStream_t s);
hipError_t launch_fq_pack(const char *text, const unsigned long long *line_end, uint64_t n_rec,
                          const unsigned long long *offs, int qual_offset, uint8_t *out, unsigned long long *err,
                          hipStream_t s);
// read pairs from two texts (A: mates /1, B: mates /2, each with its own line words): launch_fq_pair_records for
// that layout. len and err use the alternating order's record indices (A's record p is 2p, B's 2p + 1); extra: A's
// record n_pairs is checked as a record only (len has 2 n_pairs + extra + 1 elements). The descriptors' offsets are
// relative to fq_mates_base, the text pointer to give launch_fq_merge / launch_fq_merge_pack.
const char *fq_mates_base(const char *text_a, const char *text_b, uint64_t *offs_a, uint64_t *offs_b);
hipError_t launch_fq_mate_records(const char *text_a, uint64_t n_a, const unsigned long long *line_a, const char *text_b,
                                  uint64_t n_b, const unsigned long long *line_b, uint64_t n_pairs, bool extra,
                                  unsigned long long *len, unsigned long long *err, void *desc_buf, hipStream_t s);

// Output hand-off to the reference's owner rank (kcount_owner.hip): get_kmer_target_rank =
// minimizer_hash_fast(minimizer_len) % rank_n (src/kcount/kmer_dht.cpp:193-196, src/kmer.cpp:344-393,454-463).
struct OutRows {
  uint64_t *keys;  // [n * nlo] Kmer::longs layout
  uint16_t *counts;
  char *left, *right;
};
// KmerDHT minimizer length for k (src/kcount/kmer_dht.cpp:114-116)
inline int minimizer_len_for(int k) { return k * 2 / 3 + 1 < 15 ? 15 : (k * 2 / 3 + 1 > 27 ? 27 : k * 2 / 3 + 1); }
// mhmkc_fetch_ordered: the output rows in the order of the top 32 bits of mhmkc_map_hash (kcount_owner.hip)
size_t map_order_scratch_bytes(uint64_t n, int nlo);
hipError_t preload_owner_kernels();
// mhmkc_fetch_map_range: each of the n ordered rows' slot in a KmerMap of cap (a power of two) slots filled in this
// order from empty (0xFFFFFFFF: past the last slot) and its tag byte
size_t map_slots_scratch_bytes(uint64_t n);
hipError_t launch_map_slots(const uint64_t *keys, uint64_t n, int nlo, uint64_t cap, void *scratch, size_t scratch_bytes,
                            uint32_t *slot, uint8_t *tag, hipStream_t s);
hipError_t launch_map_order(const OutRows &in, uint64_t n, int nlo, void *scratch, size_t scratch_bytes, const OutRows &out,
                            hipStream_t s);
// minimizer_hash_fast of n keys (nlo words each, the first k/32+1 used)
hipError_t launch_minimizer_hash(const uint64_t *keys, uint64_t n, int nlo, int k, int m, uint64_t *out, hipStream_t s);
// dest[i] = owner rank of row i; hist[r] += rows owned by rank r (zero hist first)
hipError_t launch_owner_hist(const uint64_t *keys, uint64_t n, int nlo, int k, int m, int n_ranks, uint8_t *dest,
                             unsigned long long *hist, hipStream_t s);
// rows grouped by owner: row i goes to out at cursor[dest[i]]++ (cursor = per-owner start offsets)
hipError_t launch_owner_scatter(const OutRows &in, uint64_t n, int nlo, const uint8_t *dest, int n_ranks,
                                unsigned long long *cursor, const OutRows &out, hipStream_t s);

// Queries on the finished table (kcount_query.hip): an open-addressing index over the output rows, 8-byte slots
// row | tag << 32 (tag = the low 32 bits of mhmkc_map_hash, home slot = hash >> shift, linear probing, an empty slot
// all ones). slots holds mask + 1 entries (a power of two > n_rows), set to 0xFF bytes before launch_query_build.
struct QueryIndex {
  unsigned long long *slots;
  uint64_t mask;    // capacity - 1
  uint64_t n_rows;  // rows of the table it indexes (< 2^32 - 1)
  int shift;        // 64 - log2(capacity)
};
hipError_t preload_query_kernels();
// Workgroups of a grid-stride launch over n items, 256 threads each, of kcount_query.hip and kcount_uutig.hip. The test
// knob query_grid (include/mhmkc_debug.h) caps them at query_grid_cap, so that the loops stride on a small table; 0, the
// product's value: the kernels' own grids.
inline unsigned query_grid_cap = 0;
inline unsigned query_grid_for(uint64_t n) {
  const uint64_t g = n + 255 < 16384ull * 256 ? (n + 255) / 256 : 16384;
  return (unsigned)(g < 1 ? 1 : (query_grid_cap && query_grid_cap < g ? query_grid_cap : g));
}
// Workgroups of the read-pair merge's grid-stride launches (fastq.hip: launch_fq_merge, both instances, and
// launch_fq_merge_pack), four waves each, one pair per wave and turn. The test knob merge_grid (include/mhmkc_debug.h)
// caps them at merge_grid_cap, so that a wave takes several pairs in turn on a small batch; 0, the product's value: the
// launches' own grids.
inline unsigned merge_grid_cap = 0;
inline uint64_t merge_grid_for(uint64_t blocks) { return merge_grid_cap && merge_grid_cap < blocks ? merge_grid_cap : blocks; }
// nl = k/32 + 1 key words (1..4) of the nlo words per row / query
hipError_t launch_query_build(const uint64_t *keys, uint64_t n, int nl, int nlo, const QueryIndex &ix, hipStream_t s);
// rows[i] = the row of query i (0xFFFFFFFF: not in the table), counts / left / right its fields (0 on a miss); any
// output may be null. canonicalize: min(key, revcomp(key)) is looked up. The unused low bits of a query's last word
// are ignored.
hipError_t launch_query_lookup(const uint64_t *q, uint64_t n, bool canonicalize, int k, int nl, int nlo,
                               const QueryIndex &ix, const OutRows &t, uint32_t *rows, uint16_t *counts, char *left,
                               char *right, hipStream_t s);
// next / status [2 * n]: entry d * n + i = row i's de Bruijn neighbour in direction d (mhmkc_dbjg_links)
hipError_t launch_dbjg_links(const OutRows &t, uint64_t n, int k, int nl, int nlo, const QueryIndex &ix, uint32_t *next,
                             uint8_t *status, hipStream_t s);

// Queries answered by the rank that owns the key (kcount_route.hip). A round serves m queries of one
// rank, given as keys (links = 0: q holds m * nlo words, canonicalize as in launch_query_lookup) or as the link entries
// [e0, e0 + m) of the rank's table t of n_rows rows (links = 1: entry d * n_rows + i asks for row i's neighbour in
// direction d, or for nothing when the row's own extensions end it).
struct RouteSource {
  int links;
  const uint64_t *q;
  int canonicalize;
  OutRows t;
  uint64_t n_rows, e0;
};
hipError_t preload_route_kernels();
// dest[i] = get_kmer_target_rank of query i (0xFF: the entry asks nothing); hist[r] += the queries of owner r (zero first)
hipError_t launch_route(const RouteSource &src, uint64_t m, int k, int nl, int nlo, int mlen, int n_ranks, uint8_t *dest,
                        unsigned long long *hist, hipStream_t s);
// send: the queries' keys, nl words each, grouped by owner from cursor[r] on (cursor = the owners' first places, advanced
// by the kernel); pos[i] = the place of query i in that layout (0xFFFFFFFF: none). send and the replies hold m places.
hipError_t launch_route_pack(const RouteSource &src, uint64_t m, int k, int nl, int nlo, const uint8_t *dest, int n_ranks,
                             unsigned long long *cursor, uint64_t *send, uint32_t *pos, hipStream_t s);
// reply[i] = row | count << 32 | left << 48 | right << 56 of key i (nl words each) in the table ix indexes, a miss
// 0xFFFFFFFF; ix.n_rows == 0: no index, every key misses
hipError_t launch_route_answer(const uint64_t *keys, uint64_t n, int k, int nl, int nlo, const QueryIndex &ix,
                               const OutRows &t, unsigned long long *reply, hipStream_t s);
// the outputs of mhmkc_lookup_ranks for the round's m queries from reply[pos[i]] (any output may be null). layout: the
// places of reply; n_rows_of [n_ranks]: the ranks' row counts; a place or a row beyond them reads as a miss
hipError_t launch_route_unpack(const unsigned long long *reply, const uint32_t *pos, const uint8_t *dest, uint64_t m,
                               uint64_t layout, int n_ranks, const unsigned long long *n_rows_of, uint8_t *ranks,
                               uint32_t *rows, uint16_t *counts, char *left, char *right, hipStream_t s);
// entries [e0, e0 + m) of next_rank / next_row / status [2 * n_rows] (mhmkc_dbjg_links_ranks)
hipError_t launch_route_verdict(const RouteSource &src, uint64_t m, int k, int nl, int nlo,
                                const unsigned long long *reply, const uint32_t *pos, const uint8_t *dest, uint64_t layout,
                                int n_ranks, const unsigned long long *n_rows_of, uint8_t *next_rank, uint32_t *next_row,
                                uint8_t *status, hipStream_t s);

// one rank: next_rank[i] = 0 where next[i] names a row, else 0xFF (mhmkc_dbjg_links_ranks on a single-rank handle)
hipError_t launch_route_rank0(const uint32_t *next, uint64_t n, uint8_t *next_rank, hipStream_t s);

// The uutigs of the table from those links (kcount_uutig.hip). Port 2 * row + d; a port's ranking state:
// link = the port reached (bits 0-39) | the round that wrote it (bits 48-55) | done (bit 63: the port is the chain's end
// port), dist / sum / minw0, minrow = the rows passed, their counts, the smallest key among them.
struct alignas(32) UutigPort {
  uint64_t link, sum, minw0;
  uint32_t dist, minrow;
};
// the first state of all 2 n ports (list == null, n_items = 2 n) or of the listed ones; cut: the listed ports' cycles
// are opened at the start their state in cut names
hipError_t launch_uutig_init(const OutRows &t, uint64_t n, int nlo, const uint32_t *next, const uint8_t *status,
                             const uint64_t *list, uint64_t n_items, const UutigPort *cut, uint32_t round, UutigPort *st,
                             hipStream_t s);
// one pointer-jumping round src -> dst; *active += the ports that are not done after it
hipError_t launch_uutig_jump(const UutigPort *src, UutigPort *dst, uint64_t n, const uint64_t *list, uint64_t n_items,
                             const uint64_t *keys, int nl, int nlo, uint32_t round, unsigned long long *active,
                             hipStream_t s);
// the ports that are not done, appended to list (at most cap)
hipError_t launch_uutig_active(const UutigPort *st, uint64_t n, uint64_t *list, uint64_t cap, unsigned long long *n_list,
                               hipStream_t s);
// row_pos[i] = the start row of row i's component, row_ctg = 0xFFFFFFFF, the start rows appended to starts [n]
hipError_t launch_uutig_starts(const OutRows &t, uint64_t n, int nl, int nlo, const UutigPort *st, uint32_t *row_ctg,
                               uint32_t *row_pos, uint8_t *row_rc, uint32_t *starts, unsigned long long *n_starts,
                               hipStream_t s);
size_t uutig_table_scratch_bytes(uint64_t n_ctgs);
// starts sorted by key; n_kmers / depths [n_ctgs], offsets [n_ctgs + 1], row_ctg of the start rows
hipError_t launch_uutig_table(const OutRows &t, uint64_t n, int k, int nl, int nlo, const UutigPort *st, uint32_t *starts,
                              uint64_t n_ctgs, void *scratch, size_t scratch_bytes, uint32_t *row_ctg, uint32_t *n_kmers,
                              double *depths, uint64_t *offsets, hipStream_t s);
hipError_t launch_uutig_place(const OutRows &t, uint64_t n, const UutigPort *st, uint32_t *row_ctg, uint32_t *row_pos,
                              uint8_t *row_rc, hipStream_t s);
hipError_t launch_uutig_bases(const OutRows &t, uint64_t n, int k, int nl, int nlo, const uint32_t *row_ctg,
                              const uint32_t *row_pos, const uint8_t *row_rc, const uint64_t *offsets,
                              const uint32_t *n_kmers, uint64_t n_ctgs, uint64_t n_bases, char *seqs, hipStream_t s);

// What a rank keeps of the uutigs of the union of all ranks' tables (kcount_uutig_ranks.hip). The
// union's rows lie in rank order, rank r's at [base[r], base[r + 1]) (base: g + 1 device words); starts: the union's start
// rows in contig order. One scratch buffer of uutig_ranks_scratch_bytes serves _ids and _take, which hand out pointers
// into it.
size_t uutig_ranks_scratch_bytes(uint64_t n_ctgs);
// order: the union's contigs sorted (stably) by the rank of their start row; gid[c]: contig c's place in it, its global
// id; first[r] (g + 1 device words): the first place of rank r, ~0 when it has no contig
hipError_t launch_uutig_ranks_ids(const uint32_t *starts, uint64_t n_ctgs, const uint64_t *base, int g, void *scratch,
                                  size_t scratch_bytes, const uint32_t **order, const uint32_t **gid, uint64_t *first,
                                  hipStream_t s);
// places [first_me, first_me + n_mine) of order: n_kmers / depths [n_mine], offsets [n_mine + 1]
hipError_t launch_uutig_ranks_take(const uint32_t *order, uint64_t first_me, uint64_t n_mine, uint64_t n_ctgs,
                                   const uint64_t *uoff, const double *udepths, const uint32_t *unk, void *scratch,
                                   size_t scratch_bytes, uint32_t *n_kmers, double *depths, uint64_t *offsets,
                                   hipStream_t s);
hipError_t launch_uutig_ranks_seqs(const uint32_t *order, uint64_t first_me, uint64_t n_mine, uint64_t n_ctgs,
                                   const uint64_t *uoff, const char *useq, uint64_t u_bases, const uint64_t *offsets,
                                   uint64_t n_bases, char *seqs, hipStream_t s);
// the row map of union rows [base_me, base_me + n_me) with global contig ids
hipError_t launch_uutig_ranks_rows(const uint32_t *urow_ctg, const uint32_t *urow_pos, const uint8_t *urow_rc,
                                   uint64_t n_rows, uint64_t base_me, uint64_t n_me, const uint32_t *gid, uint64_t n_ctgs,
                                   uint32_t *row_ctg, uint32_t *row_pos, uint8_t *row_rc, hipStream_t s);

// The uutigs of the union from rank-local fragments (kcount_uutig_frags.hip). Routed links: entry
// d * n + i of rl_row / rl_rank / rl_status (mhmkc_dbjg_links_ranks). A claim is three u32 (MHMKC_UFRAG_CLAIM_BYTES). An
// open fragment's record is its start key (nl words, in keys) and UFRAG_REST_WORDS words (in rest):
//   0 the sum of its rows' counts; 1 start row | rows << 32; 2 the rows of its end ports 0 | 1 << 32; 3 the rows of their
//   peer ports; 4 start count | rank << 16 | peer ranks << 24, << 32 | end directions << 40, 41 | peer directions << 42, 43 |
//   has a peer << 44, 45; 5 the start row's position in the fragment.
// Fragment f has the ports 2 f + y, y the end; fragments of rank r lie at [base[r], base[r + 1]) of the gathered records.
constexpr int UFRAG_REST_WORDS = 6;
enum { UFRAG_C_OPEN = 0, UFRAG_C_CLOSED, UFRAG_C_CYCLES, UFRAG_C_LINKS, UFRAG_C_STARTS, UFRAG_C_MINE, UFRAG_C_XCYCLES,
       UFRAG_C_BAD, UFRAG_C_ACTIVE, UFRAG_COUNTERS };
// the replicated fragment graph after its ranking: entry [2 nf] the port a port enters (all ones: an end), st [2 nf] the
// ranking states, comp [nf] the contig's start fragment, off [nf] the contig's rows before the fragment, flag [nf] (1
// reversed against the start fragment, 2 a start fragment, 4 of a cycle), cidx [nf + 1] a start fragment's place among
// the xc cross-rank contigs, gid [xc] their global ids
struct UfragGraph {
  const uint64_t *keys, *rest;
  uint64_t nf;
  int nl;
  const uint64_t *entry;
  const UutigPort *st;
  const uint32_t *comp, *off;
  const uint8_t *flag;
  const uint32_t *cidx, *gid;
  uint64_t xc;
};
// hist[r] += the claims this rank sends rank r (zero first)
hipError_t launch_ufrag_claim_count(uint64_t n, int me, int g, const uint8_t *rl_rank, const uint8_t *rl_status,
                                    unsigned long long *hist, hipStream_t s);
// the claims grouped by receiver from cursor[r] on (the receivers' first places, advanced by the kernel); send holds cap
hipError_t launch_ufrag_claim_pack(uint64_t n, int me, int g, const uint32_t *rl_row, const uint8_t *rl_rank,
                                   const uint8_t *rl_status, unsigned long long *cursor, uint64_t cap, uint32_t *send,
                                   hipStream_t s);
// xlink[2 * row + d] = 1 for every own port a received claim of rank `from` cross-links (zero first); *n_links += them
hipError_t launch_ufrag_claim_match(const uint32_t *recv, uint64_t n_recv, int from, uint64_t n, const uint32_t *rl_row,
                                    const uint8_t *rl_rank, const uint8_t *rl_status, uint8_t *xlink,
                                    unsigned long long *n_links, hipStream_t s);
// next / status [2 n] in mhmkc_dbjg_links's layout for the rank's own table: a link to another rank is an end
hipError_t launch_ufrag_local_links(uint64_t n, int me, const uint32_t *rl_row, const uint8_t *rl_rank,
                                    const uint8_t *rl_status, uint32_t *next, uint8_t *status, hipStream_t s);
// row_ctg[start] = the fragment's index in starts; lf_open [n_frag]: its place among the rank's records or 0xFFFFFFFF;
// closed fragments' starts appended to cstarts [n]; ctr: UFRAG_C_OPEN, _CLOSED, _CYCLES, _STARTS, _BAD
hipError_t launch_ufrag_classify(const uint32_t *starts, uint64_t n_frag, uint64_t n, const UutigPort *st,
                                 const uint8_t *xlink, const uint32_t *next, const uint8_t *status, uint32_t *row_ctg,
                                 uint32_t *lf_open, uint32_t *cstarts, unsigned long long *ctr, hipStream_t s);
hipError_t launch_ufrag_emit(const OutRows &t, uint64_t n, int nl, int nlo, const uint32_t *starts, uint64_t n_frag,
                             const UutigPort *st, const uint8_t *xlink, const uint32_t *rl_row, const uint8_t *rl_rank,
                             const uint8_t *rl_status, const uint32_t *lf_open, int me, uint64_t n_open, uint64_t *keys,
                             uint64_t *rest, hipStream_t s);
// rocprim's scratch for the sorts and scans of these launches over at most n_items items
size_t ufrag_tmp_bytes(uint64_t n_items);
size_t ufrag_resolve_scratch_bytes(uint64_t nf);
hipError_t launch_ufrag_resolve(const uint64_t *rest, uint64_t nf, void *scratch, size_t scratch_bytes, void *tmp,
                                size_t tmp_bytes, uint64_t *entry, hipStream_t s);
// launch_uutig_init for the fragment graph: weighted states (dist: the rows of the fragment entered, sum: the fragment's)
hipError_t launch_ufrag_init(const uint64_t *keys, const uint64_t *rest, uint64_t nf, int nl, const uint64_t *entry,
                             const uint64_t *list, uint64_t n_items, const UutigPort *cut, uint32_t round, UutigPort *st,
                             hipStream_t s);
// comp / off / flag, isstart [nf + 1] and its exclusive scan cidx [nf + 1]; ctr: UFRAG_C_XCYCLES, _BAD
hipError_t launch_ufrag_place(const uint64_t *keys, uint64_t nf, int nl, const UutigPort *st, const uint64_t *entry,
                              uint32_t *comp, uint32_t *off, uint8_t *flag, uint32_t *isstart, uint32_t *cidx, void *tmp,
                              size_t tmp_bytes, unsigned long long *ctr, hipStream_t s);
// the start rows of the start fragments in [f0, f1) appended to cstarts; ctr: UFRAG_C_STARTS, _MINE
hipError_t launch_ufrag_owned(const uint64_t *rest, uint64_t f0, uint64_t f1, uint64_t nf, const uint8_t *flag, uint64_t n,
                              uint32_t *cstarts, unsigned long long *ctr, hipStream_t s);
size_t ufrag_table_scratch_bytes(uint64_t n_ctgs);
// cstarts sorted by key; n_kmers / depths [n_ctgs], offsets [n_ctgs + 1]; lf_ctg[fragment] = its contig here; gid of the
// cross-rank contigs this rank owns (rst: the states of the local ranking; f0, n_open: the rank's records)
hipError_t launch_ufrag_table(const OutRows &t, uint64_t n, int k, int nl, int nlo, uint32_t *cstarts, uint64_t n_ctgs,
                              const UutigPort *rst, const uint32_t *row_ctg, const uint32_t *lf_open, uint32_t *lf_ctg,
                              uint64_t n_frag, uint64_t f0, uint64_t n_open, const UfragGraph &g, uint64_t first_id,
                              uint32_t *gid, void *scratch, size_t scratch_bytes, void *tmp, size_t tmp_bytes,
                              uint32_t *n_kmers, double *depths, uint64_t *offsets, hipStream_t s);
size_t ufrag_segs_scratch_bytes(uint64_t nf);
// seg_pos [nf]: the place of every fragment's segment in the layout grouped by (sender, owner), in fragment order inside
// a group; glen [g * g] += the groups' bytes (zero first)
hipError_t launch_ufrag_segs(const UfragGraph &g, int k, int n_ranks, void *scratch, size_t scratch_bytes, void *tmp,
                             size_t tmp_bytes, uint64_t *seg_pos, unsigned long long *glen, hipStream_t s);
// the final row map (global ids) from the fragment-local one, and every own row's bases: into seqs, or into send at
// seg_pos[fragment] - seg_base
hipError_t launch_ufrag_rows(const OutRows &t, uint64_t n, int k, int nl, int nlo, uint32_t *row_ctg, uint32_t *row_pos,
                             uint8_t *row_rc, const uint32_t *lf_open, const uint32_t *lf_ctg, uint64_t n_frag, uint64_t f0,
                             uint64_t n_open, const UfragGraph &g, int me, uint64_t first_id, uint64_t n_ctgs,
                             const uint64_t *offsets, const uint32_t *n_kmers, uint64_t n_bases, char *seqs,
                             const uint64_t *seg_pos, uint64_t seg_base, uint64_t send_bytes, char *send, hipStream_t s);
// the received segments (of rank r at seg_pos + recv_base[r] of recv) into the contigs this rank owns
hipError_t launch_ufrag_scatter(const UfragGraph &g, int k, int me, int n_ranks, uint64_t first_id, uint64_t n_ctgs,
                                const uint64_t *offsets, uint64_t n_bases, char *seqs, const uint64_t *seg_pos,
                                const uint64_t *recv_base, const char *recv, uint64_t recv_bytes, hipStream_t s);

// Assembly statistics and FASTA text of device-resident contigs (kcount_fasta.hip). The contigs are
// given as mhmkc_add_ctgs_device takes them (offs: n_ctgs + 1 entries). A box's bad_* fields hold ~c of the first
// offending contig c, 0 when there is none.
constexpr uint64_t FASTA_STATS_CHUNK = 1024;  // contigs whose depths make one partial sum, in a fixed order
struct CtgStatsBox {
  unsigned long long n_ctgs, tot_len, max_len, n_ns, len_sums[5];
  unsigned long long bad_off, bad_len;  // offsets that fall or do not start at 0; a counted contig of 2^32 bases or more
  unsigned long long n_bases;           // offs[n_ctgs]
};
struct FastaBox {
  unsigned long long bad_off, bad_depth;  // a depth that is negative, -0.0, not finite or >= 2^32 (counted contigs only)
  unsigned long long n_bases, n_written, n_bytes;
};
// lens [n_ctgs] (a counted contig's length, else 0), partial [ceil(n_ctgs / FASTA_STATS_CHUNK)] (the chunks' depth sums,
// to be added in chunk order), box: zeroed here. Follows no offset into the bases.
hipError_t launch_ctg_stats_table(const uint64_t *offs, const double *depths, uint64_t n_ctgs, uint32_t min_len,
                                  uint32_t *lens, double *partial, CtgStatsBox *box, hipStream_t s);
// box->n_ns += the 'N' bytes of the counted contigs; only after the table's verdict on the offsets
hipError_t launch_ctg_stats_ns(const char *seqs, const uint64_t *offs, uint64_t n_ctgs, uint64_t n_bases, uint32_t min_len,
                               CtgStatsBox *box, hipStream_t s);
// N50 / L50 of the n lengths at ctg_n50_lens(scratch), of which n_counted are counted (the others are 0) and sum to
// tot_len: out[0] = n50, out[1] = l50 (device words)
size_t ctg_n50_scratch_bytes(uint64_t n);
uint32_t *ctg_n50_lens(void *scratch);
// after launch_ctg_n50: the lengths in descending order (the counted ones first)
const uint32_t *ctg_n50_sorted(const void *scratch, uint64_t n);
hipError_t launch_ctg_n50(uint64_t n, uint64_t n_counted, uint64_t tot_len, void *scratch, size_t scratch_bytes,
                          unsigned long long *out, hipStream_t s);
// the records' places: dst_off [n_ctgs + 1] in scratch, box->n_bytes = the text's length
size_t fasta_scratch_bytes(uint64_t n_ctgs);
hipError_t launch_fasta_table(const uint64_t *offs, const double *depths, uint64_t n_ctgs, uint64_t first_id,
                              uint32_t min_len, void *scratch, size_t scratch_bytes, FastaBox *box, const uint64_t **dst_off,
                              hipStream_t s);
// the bases, then the headers, into text (16-byte aligned, whole 16-byte units allocated); only after the table's verdict
hipError_t launch_fasta_copy(const char *seqs, const uint64_t *offs, uint64_t n_ctgs, uint64_t n_bases,
                             const uint64_t *dst_off, uint64_t n_bytes, char *text, hipStream_t s);
hipError_t launch_fasta_headers(const uint64_t *offs, const double *depths, uint64_t n_ctgs, uint64_t first_id,
                                const uint64_t *dst_off, uint64_t n_bytes, char *text, hipStream_t s);

}  // namespace mhm
