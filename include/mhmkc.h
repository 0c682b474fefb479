/*
 * mhmkc.h — C ABI of the MI355X-native k-mer counting stage (libmhmkc.so).
 *
 * This is the drop-in boundary for the MetaHipMer2 kcount hot path of ajpowelsnl/mhm2_proxy
 * (reference: src/kcount/). The reference has no C ABI; its backend seam is two pimpl classes,
 * SeqBlockInserter<MAX_K> (src/kcount/kcount.hpp:57-69) and HashTableInserter<MAX_K>
 * (src/kcount/kmer_dht.hpp:95-116), linked either from kcount_cpu.cpp or kcount_gpu.cpp
 * (src/kcount/CMakeLists.txt:23-43). Every entry point below names the reference interface it
 * replaces. include/mhmkc_kcount.hpp rebuilds those C++ shapes (Kmer<MAX_K>, KmerCounts, KmerMap,
 * analyze_kmers) on top of this ABI; INTEGRATION.md shows the binding.
 *
 * Semantics are bit-exact with the reference CPU kcount (kcount_cpu.cpp), not with its CUDA
 * backend (which drops N-k-mers, caps extension counts at 10000 and uses an approximate filter).
 *
 * Conventions (mirroring the reference's error behaviour, which DIEs on bad input):
 *   - every function returns MHMKC_OK (0) or a negative MHMKC_E* code; mhmkc_last_error() holds the
 *     message; the C++ adapter turns a failure into a fatal error like the reference's DIE;
 *   - host input buffers are borrowed only for the duration of the call;
 *   - device input buffers passed to *_device functions must stay valid until mhmkc_finish returns, and
 *     are read on the handle's stream: data written on another stream must be ordered first with
 *     mhmkc_wait_stream (or by creating the handle on that stream, mhmkc_config.stream);
 *   - a handle drives exactly one GPU and is not thread-safe. Multi-GPU = one process (rank) per
 *     GPU, all ranks calling the same sequence; the k-mer exchange is an all-to-all inside mhmkc_finish
 *     (replacing the UPC++ supermer store, src/kcount/kmer_dht.cpp:133-149,222-224): RCCL over xGMI
 *     (mhmkc_config.comm_id), or a host-staged transport the caller provides (mhmkc_set_transport: a
 *     UPC++/MPI/gloo host, several nodes, or several ranks sharing one GPU). The traversal of a contigging round
 *     over all ranks' tables is mhmkc_uutigs_ranks (the replicated build) or mhmkc_uutigs_frags (rank-local
 *     fragments joined across ranks), collective over the same transport.
 */
#ifndef MHMKC_H
#define MHMKC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (14 gained symbols without a new number: mhmkc_uutigs_frags, mhmkc_uutigs_frags_info; then mhmkc_ctgs_stats_device,
 * mhmkc_uutigs_stats, mhmkc_ctgs_fasta_device, mhmkc_uutigs_fasta, mhmkc_fasta_device, mhmkc_fasta_fetch,
 * mhmkc_fasta_write, mhmkc_fasta_info and the code MHMKC_EIO) */
#define MHMKC_ABI_VERSION 14
#define MHMKC_COMM_ID_BYTES 128

enum {
  MHMKC_OK = 0,
  MHMKC_EINVAL = -1,      /* bad argument or configuration */
  MHMKC_ENOMEM = -2,      /* device or host allocation failed */
  MHMKC_EHIP = -3,        /* HIP runtime error */
  MHMKC_ERCCL = -4,       /* RCCL error */
  MHMKC_ESTATE = -5,      /* call out of order (e.g. fetch before finish) */
  MHMKC_EBADCHAR = -6,    /* input byte outside the PackedRead code range (reference DIE, kcount_cpu.cpp:453-458) */
  MHMKC_EUNSUPPORTED = -7, /* valid for the reference but not supported here */
  MHMKC_ETRANSPORT = -8,   /* a mhmkc_set_transport callback failed, or none was set where needed */
  MHMKC_EIO = -9           /* mhmkc_fasta_write: the file could not be created, sized, opened or written */
};

typedef struct mhmkc *mhmkc_t;

/* Configuration of one counting round (one k). Replaces the KmerDHT constructor arguments
 * (src/kcount/kmer_dht.cpp:106-154) and the analyze_kmers parameters (src/kcount/kcount.hpp:71-73). */
typedef struct {
  int32_t k;              /* k-mer length; 1 <= k <= 127, k % 32 != 0 */
  int32_t n_longs;        /* output words per key; 0 = k/32+1 (= MAX_K/32, src/main.cpp:170) */
  int32_t qual_offset;    /* 33 or 64 (only used by mhmkc_add_seqs' PackedRead-free path) */
  int32_t qual_cutoff;    /* KCOUNT_QUAL_CUTOFF (CMakeDefinitions.txt:46), default 20 */
  int32_t dmin_thres;     /* --min-depth-thres (src/options.cpp:289-290), default 2; <= 32768 */
  double dyn_min_depth;   /* DYN_MIN_DEPTH (CMakeDefinitions.txt:60), default 0.9 */
  int32_t device;         /* HIP device ordinal; -1 = current device */
  int32_t rank;           /* this rank, 0 <= rank < n_ranks */
  int32_t n_ranks;        /* number of GPUs (ranks) sharing the k-mer space */
  const uint8_t *comm_id; /* MHMKC_COMM_ID_BYTES from mhmkc_comm_id() on rank 0; NULL if n_ranks==1 or
                             the exchange goes through mhmkc_set_transport */
  void *stream;           /* hipStream_t to run on; NULL = the library creates its own */
  int32_t output_owner;   /* MHMKC_OWNER_*: where a finished k-mer lives when n_ranks > 1 */
  int32_t minimizer_len;  /* m of get_kmer_target_rank; 0 = the KmerDHT rule clamp(2k/3+1, 15, 27)
                             (src/kcount/kmer_dht.cpp:114-116) */
} mhmkc_config;

enum {
  MHMKC_OWNER_HASH = 0,      /* the counting partition (hash range): no extra exchange */
  MHMKC_OWNER_MINIMIZER = 1  /* the reference's owner, KmerDHT::get_kmer_target_rank =
                                minimizer_hash_fast(minimizer_len) % n_ranks (src/kcount/kmer_dht.cpp:193-196),
                                which dbjg_traversal.cpp looks k-mers up on (:232-234,264-274) */
};

/* Statistics; replaces the SLOG lines of flush_inserts / insert_into_local_hashtable
 * (src/kcount/kcount_cpu.cpp:465-488,525-527). Counters are for this rank. */
typedef struct {
  uint64_t reads;          /* reads submitted */
  uint64_t bases;          /* bases submitted */
  uint64_t occurrences;    /* counted windows i in [1, L-k-1] (records produced by this rank) */
  uint64_t owned_records;  /* records counted on this rank after the exchange */
  uint64_t distinct;       /* distinct canonical k-mers owned by this rank */
  uint64_t purged;         /* dropped at finish: count < 2 or both extensions 'X' */
  uint64_t n_out;          /* k-mers in the output table (== distinct - purged) */
  uint64_t dropped;        /* always 0: the table never drops (reference num_dropped) */
  uint64_t count_sum;      /* sum over distinct k-mers of the unsaturated count (== owned_records) */
  uint64_t overflow_sweeps;/* extra LDS sweeps needed by over-full fine buckets */
  uint64_t max_bucket;     /* largest fine bucket, records */
  uint64_t fine_buckets;   /* number of fine buckets on this rank */
  uint64_t bytes_sent;     /* bytes sent to other ranks in the exchange */
  uint64_t exact_reruns;   /* capped partition passes redone with exact bucket sizes (skewed input) */
  uint64_t ctg_kmers;      /* distinct contig k-mers of the contig pass (0 without contigs) */
  uint64_t coarse_record_bytes; /* HBM bytes per k-mer record after extraction (5 for compact records) */
  uint64_t fine_record_bytes;   /* HBM bytes per k-mer record after the fine partition (4 when compact) */
  uint64_t distinct_estimate;   /* sketch estimate of this rank's distinct k-mers (sizes the fine partition) */
  double ms_total;         /* wall time of the last add_reads..finish sequence (device events) */
  double ms_kernel[8];     /* per-stage device time when profiling is on: see MHMKC_STAGE_* */
  uint64_t launches[8];    /* per-stage launch count when profiling is on */
  uint64_t bytes_recv;     /* bytes received from other ranks in the exchange */
  uint64_t handoff_sent;   /* finished k-mers moved to their MHMKC_OWNER_MINIMIZER owner (other ranks) */
  uint64_t handoff_recv;   /* finished k-mers received from other ranks at the hand-off */
  uint64_t h2d_bytes;      /* host bytes copied to the device by mhmkc_add_reads (PackedRead bytes + offsets) */
  uint64_t h2d_chunks;     /* H2D chunks of mhmkc_add_reads, each extracted as soon as it has landed */
  uint64_t slabs;          /* extracted record slabs (one per device batch or H2D chunk) */
  double ms_h2d;           /* device time of the H2D copies of the last mhmkc_add_reads (copy-stream events) */
  uint64_t lds_misses;     /* count kernel: records not found in their home slot group (LDS slow path) */
  uint64_t lds_ext_adds;   /* count kernel: extension-counter increments (from the sampled first coarse bucket,
                              scaled to all records) */
  uint64_t fq_pairs;       /* mhmkc_add_fastq_pairs: read pairs of the last call */
  uint64_t fq_merged;      /* ... of which merged (merge_reads num_merged) */
  uint64_t fq_ambiguous;   /* ... merge_reads' num_ambiguous increments */
  uint64_t fq_overlap_bases; /* ... overlap bases of the merged pairs (merge_reads overlap_len) */
  uint64_t table_slots;    /* count kernel: LDS table slots used per fine bucket (fitted to the sketch estimate) */
  uint64_t fq_file_blocks; /* mhmkc_add_fastq[_pairs]_file: blocks of the last call */
  uint64_t smer_count;     /* supermer exchange: supermers this rank built (all destinations, itself included) */
  uint64_t smer_words;     /* ... their 32-base words (each a u64 of 2-bit codes + a u32 of extension bits) */
  uint64_t xchg_rounds;    /* pipelined record exchange: rounds (one per slab of the rank with the most slabs) */
  double ms_xchg;          /* ... device time of the rounds' transfers (exchange stream events, summed) */
  double ms_xchg_exposed;  /* ... of it after the last extraction ended (what the overlap did not hide) */
  uint64_t finish_passes;  /* finish: parts of the owned hash range counted one after the other (memory: MHMKC_PASSES,
                              or as many as free device memory asks for) */
  uint64_t out_reruns;     /* finish passes redone because the output (sized from the distinct-key sketch) was full */
  uint64_t device_bytes;   /* device memory held by this process's handles after the finish */
  uint64_t device_bytes_peak; /* ... the most it held at any time */
  uint64_t inc_rounds;     /* pipelined record exchange: rounds fine-partitioned as they landed (0: all at finish) */
  uint64_t inc_fallbacks;  /* ... finishes whose incremental count failed and were redone from the sources */
  double ms_finish_tail;   /* device time from the last transfer's end (or finish's start) to the finished table */
  uint64_t inc_redone_coarse; /* ... coarse buckets whose capped fine layout overflowed (skew), counted again exactly */
  double inc_slack;           /* ... the capped fine buckets' slack over their expected records (0.25 .. 2) */
  double ms_h2d_pack;         /* last mhmkc_add_reads: host wall time packing its chunks for the wire (nibble H2D) */
  double ms_h2d_wait;         /* ... host wall time waiting for a pinned staging slot's previous copy */
  double ms_h2d_rounds;       /* ... host wall time enqueueing local rounds between its chunks (mhmkc_debug.h) */
  uint64_t h2d_raw_chunks;    /* ... its chunks sent as PackedRead bytes (the wire had drained while the host packed) */
} mhmkc_stats;

enum {
  MHMKC_STAGE_TILEIDX = 0, /* per-tile first-read index */
  MHMKC_STAGE_EHIST = 1,   /* extract + coarse histogram */
  MHMKC_STAGE_ESCAT = 2,   /* extract + coarse scatter */
  MHMKC_STAGE_XCHG = 3,    /* RCCL all-to-all exchange */
  MHMKC_STAGE_SHIST = 4,   /* fine histogram */
  MHMKC_STAGE_SSCAT = 5,   /* fine scatter */
  MHMKC_STAGE_COUNT = 6,   /* LDS hash-table count + finalize + compaction */
  MHMKC_STAGE_OTHER = 7    /* scans, memsets */
};

/* Fill *cfg with the reference defaults (k=21, qual 33/20, dmin 2, dyn 0.9, one rank). */
int mhmkc_config_init(mhmkc_config *cfg);

/* Create a counter. Replaces KmerDHT<MAX_K>::KmerDHT + HashTableInserter::init
 * (src/kcount/kmer_dht.cpp:106-154, src/kcount/kcount_cpu.cpp:425-443). With n_ranks > 1 every rank
 * must call this collectively with the same comm_id. */
int mhmkc_create(mhmkc_t *h, const mhmkc_config *cfg);

/* Release all device memory and the communicator (HashTableInserter::~HashTableInserter,
 * src/kcount/kcount_cpu.cpp:420-423). NULL is allowed. */
void mhmkc_destroy(mhmkc_t h);

/* RCCL unique id for mhmkc_config.comm_id (rank 0 calls it and broadcasts the bytes). */
int mhmkc_comm_id(uint8_t out[MHMKC_COMM_ID_BYTES]);

/* Add reads in the PackedRead byte layout (src/packed_reads.cpp:73-109): one byte per base,
 * bits 0-2 = A,C,G,T,N -> 0..4, bits 3-7 = min(q - qual_offset, 31). read_offsets has n_reads+1
 * entries, read_offsets[0] == 0, read i = bytes[read_offsets[i], read_offsets[i+1]).
 * Replaces the count_kmers read loop + SeqBlockInserter::process_seq
 * (src/kcount/kcount.cpp:54-98, src/kcount/kcount_cpu.cpp:73-103). Host buffers: copied to the device in
 * chunks on a copy stream, each chunk extracted as soon as it has landed (pinned host memory, e.g. from
 * hipHostMalloc, lets the copies run without the CPU). Returns once the copies are done. */
int mhmkc_add_reads(mhmkc_t h, const uint8_t *packed_bytes, const uint64_t *read_offsets, uint64_t n_reads);

/* Same, with device-resident buffers (no copy; must stay valid until mhmkc_finish returns). n_bases must be
 * d_read_offsets[n_reads]; the offsets are checked on the device (MHMKC_EINVAL: not a PackedReads CSR). */
int mhmkc_add_reads_device(mhmkc_t h, const uint8_t *d_packed_bytes, const uint64_t *d_read_offsets,
                           uint64_t n_reads, uint64_t n_bases);

/* Order the handle's later device work after everything enqueued so far on `stream` (a hipStream_t; NULL =
 * the legacy default stream): call it before passing buffers that another stream (e.g. torch's current
 * stream) has just written. */
int mhmkc_wait_stream(mhmkc_t h, void *stream);

/* Add sequences given as characters, lowercase = quality below the cutoff — the string that
 * SeqBlockInserter::process_seq receives (src/kcount/kcount.cpp:80-86). Host buffers. depth is the
 * per-sequence count (reads: 1). Only depth == 1 (the read pass) is supported in this version. */
int mhmkc_add_seqs(mhmkc_t h, const char *seqs, const uint64_t *seq_offsets, uint64_t n_seqs, uint16_t depth);

/* Add reads given as FASTQ text: parsed and packed on the device, then counted as mhmkc_add_reads.
 * Replaces FastqReader::get_next_fq_record (src/fastq.cpp:504-551: 4 lines per record, rtrim, the '@' and
 * '+' checks, get_fq_name :73-122, equal sequence and quality lengths) + the PackedRead constructor
 * (src/packed_reads.cpp:73-109: N and IUPAC codes -> 4, quality min(q - qual_offset, 31)) for reads that
 * reach kcount unchanged (single-end input; paired input goes through mhmkc_add_fastq_pairs, which merges
 * the pairs first). Where the reference DIEs the call fails:
 * MHMKC_EINVAL for a malformed record (the message names the first bad record, 0-based),
 * MHMKC_EBADCHAR for a base outside A C G T N U R Y K M S W B D H V, MHMKC_EUNSUPPORTED for a line
 * longer than 2045 characters (the reference's fgets buffer, src/fastq.hpp:61, would split it).
 * Host text of n_bytes bytes (no terminator needed). */
int mhmkc_add_fastq(mhmkc_t h, const char *text, uint64_t n_bytes);

/* Same, with device-resident text (only read during the call). The buffer must extend at least 4 bytes
 * past n_bytes (the parser reads whole aligned dwords; the padding bytes are never interpreted). */
int mhmkc_add_fastq_device(mhmkc_t h, const char *d_text, uint64_t n_bytes);

/* Add read pairs given as interleaved FASTQ text (records 2p and 2p+1 are the mates /1 and /2 of pair p, the
 * order FastqReader gives a pair of files, src/fastq.cpp:509-516): parsed on the device as mhmkc_add_fastq,
 * then merged as merge_reads does (src/merge_reads.cpp:237-588: mate 2 reverse-complemented, offsets scanned
 * with the mismatch, N and differential-quality rules, an unambiguous overlap merged base by base by quality),
 * and the resulting PackedReads counted: for each pair the merged read and a dummy mate "N", or both mates
 * unmerged (packed_reads_list of merge_reads). A last record without its mate is not added (the reference's
 * loop stops there). Fails where the reference DIEs: the mhmkc_add_fastq errors, MHMKC_EINVAL for mates whose
 * names differ or are not /1 and /2 ("Mismatched pairs"), for an overlap quality outside the Q2Perror table,
 * MHMKC_EBADCHAR for an illegal base. Statistics: fq_pairs, fq_merged, fq_ambiguous, fq_overlap_bases. */
int mhmkc_add_fastq_pairs(mhmkc_t h, const char *text, uint64_t n_bytes);
/* Same, with device-resident text (only read during the call; 4 bytes of padding as for mhmkc_add_fastq_device). */
int mhmkc_add_fastq_pairs_device(mhmkc_t h, const char *d_text, uint64_t n_bytes);

/* FASTQ file ingest with the file I/O overlapped: the file at `path` is read in blocks of
 * MHMKC_FQ_BLOCK bytes (environment; default 256 MB) into pinned memory, each block copied to the device and parsed
 * (as mhmkc_add_fastq / mhmkc_add_fastq_pairs) as soon as it is read, its cut last record (pair) carried into the
 * next block; a block's extraction runs on the device while the next block is read. Errors as for the text entry
 * points (record indices in messages count from the start of the failing block; the message names the block and
 * the file byte its text starts at); MHMKC_EINVAL if the file cannot be opened or read. A failure after the first
 * block leaves the earlier blocks' reads in the round: mhmkc_finish then fails with MHMKC_ESTATE until
 * mhmkc_reset. mhmkc_fastq_packed / mhmkc_fastq_fetch then hold the PackedReads of the whole file (every
 * block's, appended on the device: the later k rounds count them with mhmkc_add_reads_device). */
int mhmkc_add_fastq_file(mhmkc_t h, const char *path);
int mhmkc_add_fastq_pairs_file(mhmkc_t h, const char *path);

/* Read pairs given as two texts, the mates /1 in text1 and the mates /2 in text2: the reference's read library
 * "r1.fq:r2.fq" (src/main.cpp:110-119), which FastqReader hides behind one reader that alternates between the two
 * files (src/fastq.cpp:240-308, :509-516). The texts are read in that order, A[0], B[0], A[1], B[1], ..., until the
 * text whose turn it is has nothing left (merge_reads' loop, src/merge_reads.cpp:318-321; fastq.cpp:518): with c1 and
 * c2 complete records, P = min(c1, c2) pairs are merged; if c1 > P, record A[P] is checked as a record and not added
 * (the trailing unpaired record of mhmkc_add_fastq_pairs); a text that ends inside a record is MHMKC_EINVAL only if
 * that record's turn comes; nothing after the stop is checked. The result (PackedReads, fq_* statistics, reads, bases,
 * the table, the error code) is what mhmkc_add_fastq_pairs gives on the interleaving of exactly the records read. No
 * interleaved copy is made: each text gets its own line pass, one record pass pairs record p of one with record p of
 * the other, and the merge kernels read both texts in place. Error messages name the file (1 or 2) and the 0-based
 * record within that file, pair errors the pair. Host texts (no terminators needed). */
int mhmkc_add_fastq_mates(mhmkc_t h, const char *text1, uint64_t n1, const char *text2, uint64_t n2);
/* Same, with device-resident texts (only read during the call), each extending at least 4 bytes past its length as for
 * mhmkc_add_fastq_device: any two device addresses, in either order, in one allocation or two. */
int mhmkc_add_fastq_mates_device(mhmkc_t h, const char *d_text1, uint64_t n1, const char *d_text2, uint64_t n2);
/* Same, from two files read in rounds (replaces the two-file FastqReader of src/fastq.cpp:240-308 and its
 * alternating get_next_fq_record, :509-518). A round's text of each file is that file's carry (the bytes after the
 * last pair the previous round took) plus fresh bytes up to MHMKC_FQ_BLOCK in all (environment; default 256 MB); the
 * round takes min(n1, n2) pairs of the n1 and n2 complete records it finds, and each file carries its own remainder,
 * so a file with shorter records simply reads less per round and no carry outgrows a block. A file without a
 * complete record in its text gets a block more (a record longer than the block; a carry above 1 MiB without one is
 * MHMKC_EUNSUPPORTED). The next round's bytes are read (MHMKC_FQ_THREADS preads) while the device merges, packs and
 * extracts this round's pairs. Pinned memory: two slots of MHMKC_FQ_BLOCK + 1 MiB + 64 bytes per file, whatever the
 * files' sizes; with the allocator's slack at most 4.5 * (MHMKC_FQ_BLOCK + 1 MiB + 64) + 4096 bytes in all
 * (mhmkc_fastq_mates_info). The slots stay with the handle until mhmkc_destroy (about 1.16 GB at the default block,
 * besides the two blocks mhmkc_add_fastq_file keeps); a later call with a smaller block gives the larger slots back
 * first, so the bound holds for every call's own block. When one file is exhausted the rule above decides what of the other is still read.
 * fq_file_blocks counts the rounds, the statistics are sums over them, mhmkc_fastq_packed holds every round's
 * PackedReads. Errors name the round and, for each file, the byte at which that round's text starts (record and pair
 * indices count from there); MHMKC_EINVAL if a file cannot be opened or read. A failure after the first round leaves
 * the round partial, as for mhmkc_add_fastq_file. Every rank names its own files (the split of one file pair among
 * ranks, set_matching_pair, src/fastq.cpp:310-396, is not provided). */
int mhmkc_add_fastq_mates_files(mhmkc_t h, const char *path1, const char *path2);
/* A read library named as the reference's reads_fname (FastqReader's constructor, src/fastq.cpp:250-262; main.cpp:142-148
 * passes each name on): "a:b" is mhmkc_add_fastq_mates_files(a, b), "a:" (one unpaired file) mhmkc_add_fastq_file(a),
 * "a" (one interleaved file) mhmkc_add_fastq_pairs_file(a). The first colon splits. An empty name or an empty first part
 * (":b", ":") is MHMKC_EINVAL. */
int mhmkc_add_fastq_named(mhmkc_t h, const char *name);

/* What the last mhmkc_add_fastq_mates[_device|_files] call did. Every field is 8 bytes. */
typedef struct mhmkc_fastq_mates_info {
  uint64_t pairs;            /* pairs merged (fq_pairs) */
  uint64_t rounds;           /* rounds (1 for the text calls; fq_file_blocks) */
  uint64_t bytes_read_1;     /* bytes of text 1 / file 1 given to the parser (a file: bytes read from it) */
  uint64_t bytes_read_2;
  uint64_t bytes_used_1;     /* bytes of text 1 up to the end of its last record read */
  uint64_t bytes_used_2;
  uint64_t peak_carry_1;     /* files: the most bytes of file 1 carried from one round into the next */
  uint64_t peak_carry_2;
  uint64_t pinned_bytes;     /* files: pinned host memory the handle holds for the rounds' texts */
  uint64_t pinned_bound;     /* files: the documented bound on it for this call's block size */
  uint64_t block_bytes;      /* files: MHMKC_FQ_BLOCK of this call */
  uint64_t unpaired_checked; /* 1: an unpaired record A[P] was read and checked before text 2 ran out */
  double read_wait_s;        /* files: time the rounds waited for a read to finish after their device calls returned */
} mhmkc_fastq_mates_info_t;
int mhmkc_fastq_mates_info(mhmkc_t h, mhmkc_fastq_mates_info_t *info);

/* The PackedReads of the last mhmkc_add_fastq[_pairs][_device] call on the device: d_bytes[n_bases] in the
 * PackedRead layout, d_offsets[n_reads + 1]. Valid until the next add_fastq, reset or destroy. Any
 * pointer may be NULL. */
int mhmkc_fastq_packed(mhmkc_t h, const uint8_t **d_bytes, const uint64_t **d_offsets, uint64_t *n_reads,
                       uint64_t *n_bases);

/* Copy the PackedReads of the last mhmkc_add_fastq[_device] call to host arrays (either may be NULL):
 * bytes[n_bases], offsets[n_reads + 1] (sizes from mhmkc_fastq_packed). */
int mhmkc_fastq_fetch(mhmkc_t h, uint8_t *bytes, uint64_t *offsets);

/* Add contigs for the contig pass of rounds after the first k (add_ctg_kmers, src/kcount/kcount.cpp:100-138;
 * insert_supermer_from_ctg, src/kcount/kcount_cpu.cpp:356-406). seqs: contig sequences back to back (case
 * = quality as for reads; contigs are uppercase), seq_offsets: n_ctgs+1 offsets, depths:
 * Contig::get_uint16_t_depth() (src/contigs.hpp:65), 0 counting as 1. The contig pass runs inside
 * mhmkc_finish after every read, over the contigs in the order they were added (the reference's order,
 * which its rules depend on). Contigs shorter than k+2 contribute nothing. Host buffers. With several ranks
 * every rank passes its own contigs (possibly none) and the contigs of all ranks are applied in rank order
 * (rank 0's first), one serialisation the reference's concurrent supermer stores can produce; the result
 * equals a single rank given the concatenation. */
int mhmkc_add_ctgs(mhmkc_t h, const char *seqs, const uint64_t *seq_offsets, const uint16_t *depths, uint64_t n_ctgs);

/* mhmkc_add_ctgs with device arrays (add_ctg_kmers, src/kcount/kcount.cpp:100-138; Contig::get_uint16_t_depth,
 * src/contigs.hpp:65): d_seqs holds the contigs' ASCII bases back to back, d_seq_offsets n_ctgs+1 offsets, d_depths one
 * depth per contig. n_bases sizes the handle's buffers without a round trip and must equal d_seq_offsets[n_ctgs] (the
 * device checks it). The inputs are read during the call only, on the handle's stream (written on another stream:
 * mhmkc_wait_stream first), and converted into the handle's own device buffers: the caller may overwrite or free them
 * once the call returns. The call waits for the device once, on a few words that name what is wrong with the input.
 *   MHMKC_DEPTH_U16: uint16_t depths, taken as they are. MHMKC_DEPTH_F64: double, a Contig::depth as
 *   mhmkc_uutigs_device gives it, converted as the reference does: (uint16_t)(depth > 65535 ? 65535 : depth), which
 *   truncates toward zero and turns +inf into 65535. 0 counts as 1 in both. A NaN or negative depth has no defined
 *   conversion there: MHMKC_EINVAL, the message names the first such contig.
 *   MHMKC_EBADCHAR: a byte outside ACGTNacgtn (the message names the first position, as mhmkc_add_ctgs does).
 *   MHMKC_EINVAL: offsets[0] != 0, decreasing offsets, a wrong n_bases, a null pointer with n_ctgs > 0, or 2^32-1 or more
 *   contig k-mers in the round. MHMKC_ESTATE after finish. A failed call adds nothing to the round.
 * Contigs are applied in the order they were added, whichever of mhmkc_add_ctgs, mhmkc_add_ctgs_device and
 * mhmkc_add_ctgs_from added them. From the first device add of a round on, the round's contigs are kept on the device
 * (counted in mhmkc_stats.device_bytes[_peak]) until mhmkc_reset or mhmkc_destroy; host adds that follow are uploaded
 * at once.
 * Several ranks (n_ranks > 1): accepted with output_owner == MHMKC_OWNER_MINIMIZER, the placement on which
 * mhmkc_uutigs_ranks produces contigs. The call is local (no collective; the same checks, the same mailbox): every rank
 * passes its own contigs, possibly none, and the result is the one mhmkc_add_ctgs documents for several ranks: the
 * contigs of all ranks applied in rank order, within a rank in the order of its calls, the ranks' tables together equal
 * to a single rank's given the concatenation. Ranks may mix the routes: one may add on the host only, another on the
 * device only, a third nothing. mhmkc_finish decides from all-gathered values: when no rank of the round holds contigs
 * on the device, the contigs are gathered through the host as before; otherwise every rank gathers them on the device
 * (a rank with host contigs uploads them first; DESIGN.md §3.6b, mhmkc_ctgs_ranks_info), and the gathered copy is counted
 * in device_bytes[_peak] until the finish ends. With MHMKC_OWNER_HASH and n_ranks > 1: MHMKC_EUNSUPPORTED, checked
 * before the pointers and the state. */
enum { MHMKC_DEPTH_U16 = 0, MHMKC_DEPTH_F64 = 1 };
int mhmkc_add_ctgs_device(mhmkc_t h, const char *d_seqs, const uint64_t *d_seq_offsets, const void *d_depths,
                          int depth_type, uint64_t n_ctgs, uint64_t n_bases);
/* The uutigs of the finished handle src as h's contigs, without leaving the device: mhmkc_add_ctgs_device on
 * mhmkc_uutigs_device(src) with MHMKC_DEPTH_F64 (the step from one contigging round to the next k,
 * src/contigging.cpp:93-158; k may differ between the handles). The uutigs are built first if src has none yet; src's
 * stream is ordered before h's by an event. src not finished: MHMKC_ESTATE; another device: MHMKC_EINVAL; src with
 * n_ranks > 1 and no mhmkc_uutigs_ranks build: mhmkc_uutigs's MHMKC_EUNSUPPORTED; with such a build: this rank's part
 * of it (possibly no contig), so that every rank calling mhmkc_uutigs_ranks(src) and then mhmkc_add_ctgs_from(h, src)
 * hands the union's uutigs to the next k. h with n_ranks > 1: as mhmkc_add_ctgs_device (MHMKC_OWNER_MINIMIZER only).
 * The failure's text is in mhmkc_last_error(h). */
int mhmkc_add_ctgs_from(mhmkc_t h, mhmkc_t src);

/* How the contigs of the last mhmkc_finish on a handle with n_ranks > 1 reached every rank. All zeros before such a
 * finish with contigs (and after mhmkc_reset). device_route 0: through the host (no rank held contigs on the device);
 * the sizes are set, the rest is zero. device_route 1: per peer a rank sends 6 n_ctgs +
 * ceil(n_bases / 2) bytes (u32 lengths, u16 depths, bases as nibbles). */
typedef struct {
  uint64_t device_route;             /* 0 or 1 */
  uint64_t n_ctgs, n_bases;          /* this rank's contigs and their bases */
  uint64_t n_ctgs_all, n_bases_all;  /* the round's, over all ranks */
  uint64_t windows_all;              /* the round's counted contig k-mers (contigs of k + 2 bases or more) */
  uint64_t bytes_sent, bytes_recv;   /* between the ranks, by this rank */
  double ms_pack, ms_move, ms_assemble, ms_total; /* device events on the handle's stream (the move includes its host
                                                     staging under mhmkc_set_transport); ms_total: pack .. assemble */
  uint64_t gathered_bytes;           /* device memory of the gathered copy (freed when the finish ends) */
} mhmkc_ctg_ranks_info;
int mhmkc_ctgs_ranks_info(mhmkc_t h, mhmkc_ctg_ranks_info *info);

/* The depth threshold of the finish: the reference's global _dmin_thres (src/kcount/kmer_dht.hpp:57), which
 * analyze_kmers sets (src/kcount/kcount.cpp:145) after the KmerDHT was built and get_ext reads at finish
 * (src/kcount/kcount_cpu.cpp:178). Starts as mhmkc_config.dmin_thres; takes effect at the next finish. */
int mhmkc_set_dmin_thres(mhmkc_t h, int32_t dmin_thres);

/* Exchange (multi-GPU), count and finalize: purge count < 2 and X/X, choose extensions; with
 * MHMKC_OWNER_MINIMIZER, then move every finished k-mer to its get_kmer_target_rank owner.
 * Replaces KmerDHT::flush_updates + finish_updates -> HashTableInserter::insert_into_local_hashtable
 * (src/kcount/kmer_dht.cpp:227-236, src/kcount/kcount_cpu.cpp:490-528). *n_out may be NULL. */
int mhmkc_finish(mhmkc_t h, uint64_t *n_out);

/* Copy the finished table to host arrays (any may be NULL): keys[n_out*n_longs] in Kmer::longs layout,
 * counts[n_out], left[n_out], right[n_out] ('A','C','G','T','F' or 'X'). Order is unspecified, as the
 * reference's KmerMap iteration order is. Replaces the KmerMap fill (kcount_cpu.cpp:503-522). */
int mhmkc_fetch(mhmkc_t h, uint64_t *keys, uint16_t *counts, char *left, char *right);

/* The hash the C++ adapter's KmerMap (include/mhmkc_kcount.hpp) places a key with: a multiply-xorshift mix of its
 * n_longs words; the map's home slot for a key is the top log2(capacity) bits. */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline uint64_t mhmkc_map_hash(const uint64_t *w, int n_longs) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < n_longs; i++) {
    h = (h ^ w[i]) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 31;
  }
  h *= 0x94D049BB133111EBull;
  return h ^ (h >> 29);
}

/* mhmkc_fetch with the rows ordered by the top 32 bits of mhmkc_map_hash (a radix sort on the device): filling a
 * KmerMap in that order walks its slot array once from front to back instead of touching a random slot per row
 * (insert_into_local_hashtable's loop, src/kcount/kcount_cpu.cpp:503-522). At most 2^32-1 rows. */
int mhmkc_fetch_ordered(mhmkc_t h, uint64_t *keys, uint16_t *counts, char *left, char *right);

/* Rows [row0, row0 + n_rows) of mhmkc_fetch_ordered's order (the device sorts once per finish and keeps the ordered
 * rows until the next reset): a host that fills its KmerMap chunk by chunk while the next chunk is on the wire (the C++
 * adapter's insert_into_local_hashtable) never holds the whole table twice. */
int mhmkc_fetch_ordered_range(mhmkc_t h, uint64_t row0, uint64_t n_rows, uint64_t *keys, uint16_t *counts, char *left,
                              char *right);

/* Rows [row0, row0 + n_rows) of mhmkc_fetch_ordered's order, each with the slot it takes in a KmerMap of `capacity`
 * slots (a power of two, 16 .. 2^32; home slot = the top log2(capacity) bits of mhmkc_map_hash) filled with the rows
 * in this order from empty by linear probing, and its tag byte (0x80 | the low 7 bits of mhmkc_map_hash): slot i =
 * max(home i, slot i-1 + 1), computed on the device (a prefix maximum), or 0xFFFFFFFF past the last slot (the map
 * places that row itself). The C++ adapter's KmerMap then writes each row straight to its slot, with no hashing or
 * probing on the host (insert_into_local_hashtable, src/kcount/kcount_cpu.cpp:503-522). slots / tags may be NULL. */
int mhmkc_fetch_map_range(mhmkc_t h, uint64_t capacity, uint64_t row0, uint64_t n_rows, uint64_t *keys,
                          uint16_t *counts, char *left, char *right, uint32_t *slots, uint8_t *tags);

/* Pinned (page-locked) host memory for a caller's fetch buffers: a fetch into it is one DMA per array, with no copy
 * through the library's staging buffers (mhmkc_fetch copies into pageable memory chunk by chunk). Freed blocks are
 * kept by the library for the next mhmkc_host_alloc (up to 2 GiB), since pinning costs more than one copy. NULL when
 * the allocation fails; mhmkc_host_free ignores pointers it did not hand out. */
void *mhmkc_host_alloc(uint64_t bytes);
void mhmkc_host_free(void *p);

/* Device pointers of the finished table (valid until the next reset/destroy). */
int mhmkc_device_output(mhmkc_t h, const uint64_t **d_keys, const uint16_t **d_counts, const char **d_left,
                        const char **d_right, uint64_t *n_out);

/* Point queries on the finished table, answered on the GPU. "Row i" is row i of mhmkc_fetch / mhmkc_device_output.
 * The first query after a finish builds a device index over the rows (8 bytes per slot, a power of two >= 2 n_out
 * slots, counted in mhmkc_stats.device_bytes[_peak]); it is dropped at the next reset, finish or destroy. At most
 * 2^32-2 rows (MHMKC_EUNSUPPORTED beyond). Before finish: MHMKC_ESTATE. */
#define MHMKC_NO_ROW 0xFFFFFFFFu

/* KmerDHT::get_local_kmer_counts / kmer_exists (src/kcount/kmer_dht.cpp:198-219) for n k-mers at once. keys:
 * n * n_longs words in Kmer::longs layout (the handle's n_longs; the unused low bits of the last key word are ignored).
 * canonicalize = 0 looks the key up as given (get_local_kmer_counts), 1 looks up min(key, revcomp(key)) (kmer_exists);
 * left / right are the stored (canonical-frame) extensions in both cases. Output i belongs to query i; a miss gives
 * rows[i] = MHMKC_NO_ROW, counts[i] = 0, left[i] = right[i] = 0. Any output pointer may be NULL. With n_ranks > 1 the
 * call answers for this rank's rows only (get_local_kmer_counts). Host arrays: staged through the device in chunks. */
int mhmkc_lookup(mhmkc_t h, const uint64_t *keys, uint64_t n, int canonicalize, uint32_t *rows, uint16_t *counts,
                 char *left, char *right);
/* Same with device arrays, asynchronous on the handle's stream (inputs written on another stream: mhmkc_wait_stream
 * first; the outputs are complete once the handle's stream has reached this point). */
int mhmkc_lookup_device(mhmkc_t h, const uint64_t *d_keys, uint64_t n, int canonicalize, uint32_t *d_rows,
                        uint16_t *d_counts, char *d_left, char *d_right);

enum {
  MHMKC_LINK_OK = 0,       /* next is the neighbour's row and its extension leads back */
  MHMKC_LINK_DEADEND = 1,  /* an 'X' on the row or the neighbour, or the neighbour is not in the table */
  MHMKC_LINK_FORK = 2,     /* an 'F' on the row or the neighbour */
  MHMKC_LINK_CONFLICT = 3, /* the neighbour's extension does not lead back */
  MHMKC_LINK_RC = 0x80     /* or-ed into OK: the neighbour is entered reverse-complemented */
};
/* get_next_step (src/dbjg_traversal.cpp:165-239) for every row and both directions, without the visited state: entry
 * d * n_out + i describes row i in direction d (0 LEFT, 1 RIGHT), in row i's stored (canonical) orientation.
 *   1. row i's own left or right is 'X': DEADEND; else either is 'F': FORK; next = MHMKC_NO_ROW, nothing looked up;
 *   2. the neighbour is kmer.forward_base(right) (RIGHT) / kmer.backward_base(left) (LEFT); is_rc = revcomp(neighbour)
 *      < neighbour; the smaller of the two is looked up; not in the table: DEADEND, next = MHMKC_NO_ROW;
 *   3. otherwise next = the neighbour's row j; DEADEND if row j has an 'X', else FORK if it has an 'F', else with j's
 *      extensions oriented (complemented and swapped when is_rc): RIGHT needs j's left == kmer.front(), LEFT j's right
 *      == kmer.back(); no: CONFLICT, yes: OK (| MHMKC_LINK_RC when is_rc).
 * A walker over next / status needs no hashing and no k-mer arithmetic; the visited marks (REPEAT / VISITED) stay
 * with it. Single-rank handles only (MHMKC_EUNSUPPORTED with n_ranks > 1, checked before the state). Host arrays of
 * 2 * n_out entries (either may be NULL). */
int mhmkc_dbjg_links(mhmkc_t h, uint32_t *next, uint8_t *status);
/* The same arrays on the device, computed once per finish and kept until the next reset / finish / destroy. */
int mhmkc_dbjg_links_device(mhmkc_t h, const uint32_t **d_next, const uint8_t **d_status);

/* The uutigs of the finished table, built on the GPU from those links: traverse_debruijn_graph at one rank
 * (src/dbjg_traversal.cpp:165-289,301-307,404-407,539-541,569-596) without its visited array.
 *   Ports: row i has the ports (i,0) LEFT and (i,1) RIGHT. An OK port (i,d) leads to row j = next[d][i], where travel
 *   goes on in direction dc = d ^ rc: it enters j at port (j, dc^1). (i,d) is linked iff it is OK, the port it enters is
 *   not itself (a hairpin) and that port is OK and enters (i,d); every other port is an end.
 *   Components: under linked ports the rows whose two extensions are bases form simple paths and simple cycles. A
 *   component of m rows is one uutig of m + k - 1 bases; its start is its row with the smallest key (Kmer::operator<).
 *   Layout: in the start's stored orientation, leftwards first: position 0 is the end reached through the start's port
 *   0; a cycle is opened between the start's port 1 and the row it leads to, which takes position 0 (the start m - 1).
 *   The row at position p gives base p (its first base as it lies in the contig), the last row its whole k-mer.
 *   Depth: (the sum of the m counts + the start's count) / (m + 1), the sum in 64 bits, one double division: the host
 *   walker counts the start in both walks (:224) and divides by len - k + 2.
 *   Order: contig c is the component with the c-th smallest start, the id traverse_debruijn_graph assigns and the
 *   order mhmkc_add_ctgs of the next round expects.
 *   For even k a start that is its own reverse complement and whose port 0 is its non-mutual one comes out on the
 *   other strand than the host walker's; either strand is the same uutig.
 * Built once per finish (the index and the links first if needed), kept until the next reset / finish / destroy and
 * counted in mhmkc_stats.device_bytes[_peak]: 9 bytes per row (the row map), 1 per base, 20 per contig + 8. The
 * ranking's scratch (128 bytes per row at its peak) is freed before the call returns. Single-rank handles only
 * (MHMKC_EUNSUPPORTED with n_ranks > 1, checked before the state; with several ranks the uutigs are built by
 * mhmkc_uutigs_ranks, after which this call and the getters below answer for this rank's part); before finish:
 * MHMKC_ESTATE; at most 2^32-2 rows. */
int mhmkc_uutigs(mhmkc_t h, uint64_t *n_ctgs, uint64_t *n_bases);
/* Host copies (any may be NULL): offsets[n_ctgs + 1] into seqs[n_bases] (ASCII ACGT, the format mhmkc_add_ctgs takes),
 * depths[n_ctgs], n_kmers[n_ctgs] (m). */
int mhmkc_uutigs_fetch(mhmkc_t h, uint64_t *offsets, char *seqs, double *depths, uint32_t *n_kmers);
/* The same arrays on the device (any pointer may be NULL; an empty table still has offsets = {0}). */
int mhmkc_uutigs_device(mhmkc_t h, const uint64_t **d_offsets, const char **d_seqs, const double **d_depths,
                        uint64_t *n_ctgs, uint64_t *n_bases);
/* Where every row lies: row_ctg[n_out] (MHMKC_NO_ROW: in no contig), row_pos[n_out] (its position, 0 .. m-1),
 * row_rc[n_out] (1: reverse-complemented in its contig; 0 for a start). Host arrays, any may be NULL. */
int mhmkc_uutig_rows(mhmkc_t h, uint32_t *row_ctg, uint32_t *row_pos, uint8_t *row_rc);
int mhmkc_uutig_rows_device(mhmkc_t h, const uint32_t **d_row_ctg, const uint32_t **d_row_pos, const uint8_t **d_row_rc);

/* How the last mhmkc_uutigs build went (device events on the handle's stream). */
#define MHMKC_UUTIG_MAX_ROUNDS 48
typedef struct {
  uint64_t n_ctgs, n_bases;
  uint64_t rounds;        /* pointer-jumping rounds over all ports */
  uint64_t cycle_ports;   /* ports left on cycles after them (two per cycle row) */
  uint64_t cycle_rounds;  /* rounds over those ports alone: finding the start, then ranking the opened cycle */
  uint64_t scratch_bytes; /* the peak of the build's device memory above what stays */
  uint64_t kept_bytes;    /* what stays: contig arrays and row map */
  double ms_links;        /* index + links, when this call built them (else 0) */
  double ms_succ, ms_rank, ms_cycles, ms_table, ms_rows, ms_total; /* ms_total: succ .. rows */
  double ms_round[MHMKC_UUTIG_MAX_ROUNDS]; /* the first rounds' times, one by one */
} mhmkc_uutig_info;
int mhmkc_uutigs_info(mhmkc_t h, mhmkc_uutig_info *info);

/* The uutigs of the union of all ranks' tables: traverse_debruijn_graph at rank_n() > 1 (src/dbjg_traversal.cpp:291-335,
 * 517-567,569-596). Collective over the ranks of a finished MHMKC_OWNER_MINIMIZER handle (every rank calls it, a rank
 * without rows too). The result does not depend on the number of ranks:
 *   a contig is what mhmkc_uutigs gives for the union table at one rank (component, start, strand, layout, n_kmers,
 *   depth bits: the rule above, the even-k strand note included);
 *   it belongs to the rank that holds its start row; a rank's contigs are ordered by start key; a contig's global id is
 *   first_id (the number of contigs of the lower ranks, reduce_prefix of dbjg_traversal.cpp:581-587) + its local index.
 *   So the ranks' lists, concatenated and sorted by start key, are the single-rank list.
 * How: the replicated build. Every rank receives the other ranks' rows over the handle's transport
 * (RCCL or mhmkc_set_transport), ranks the union on its GPU with mhmkc_uutigs's kernels and keeps its own contigs and the
 * row map of its own rows; the union, its index and links are freed before the call returns. The union has at most
 * 2^32-2 rows (MHMKC_EUNSUPPORTED beyond, on every rank).
 * After a successful call mhmkc_uutigs, mhmkc_uutigs_fetch, mhmkc_uutigs_device, mhmkc_uutig_rows[_device] and
 * mhmkc_uutigs_info answer on this handle for this rank: its contigs, and for every one of its rows row_ctg (the GLOBAL
 * contig id, also when the contig belongs to another rank; MHMKC_NO_ROW: in no contig), row_pos and row_rc. Kept until
 * the next reset / finish / destroy and counted in mhmkc_stats.device_bytes[_peak]. Without such a build every call that
 * is MHMKC_EUNSUPPORTED on a multi-rank handle stays so.
 * n_ranks == 1: mhmkc_uutigs with *first_id = 0 (whatever the owner). n_ranks > 1 with MHMKC_OWNER_HASH:
 * MHMKC_EUNSUPPORTED (the reference's own placement is the supported one); before finish: MHMKC_ESTATE; both before any
 * collective. A failure on any rank after the first collective is a failure on every rank (the ranks exchange their
 * status at the end): MHMKC_ETRANSPORT on the ranks that did not fail themselves. Any output pointer may be NULL. */
int mhmkc_uutigs_ranks(mhmkc_t h, uint64_t *n_ctgs, uint64_t *n_bases, uint64_t *first_id, uint64_t *n_ctgs_all);

/* How the last mhmkc_uutigs_ranks went. Stages: rows moved between the ranks, the ranking of the union, the selection
 * of this rank's part. Routed records are table rows; only MHMKC_URANKS_GATHER moves any. */
enum { MHMKC_URANKS_GATHER = 0, MHMKC_URANKS_BUILD = 1, MHMKC_URANKS_SELECT = 2, MHMKC_URANKS_STAGES = 3 };
typedef struct {
  uint64_t n_ctgs, n_bases;      /* this rank's */
  uint64_t first_id, n_ctgs_all;
  uint64_t n_rows, n_rows_all;   /* this rank's rows, the union's */
  uint64_t rounds;               /* pointer-jumping rounds over all ports of the union */
  uint64_t cycle_rounds;         /* rounds over the ports on cycles alone */
  uint64_t cycle_ports;          /* ports left on cycles (two per cycle row of the union) */
  uint64_t routed_records_sent[MHMKC_URANKS_STAGES], routed_records_recv[MHMKC_URANKS_STAGES];
  uint64_t routed_bytes_sent[MHMKC_URANKS_STAGES], routed_bytes_recv[MHMKC_URANKS_STAGES];
  double ms_stage[MHMKC_URANKS_STAGES]; /* device events on the handle's stream (the gather includes its host staging) */
  double ms_total;
  uint64_t scratch_bytes;        /* the peak of the build's device memory above what stays */
  uint64_t kept_bytes;           /* what stays: this rank's contig arrays and row map */
} mhmkc_uutig_ranks_info;
int mhmkc_uutigs_ranks_info(mhmkc_t h, mhmkc_uutig_ranks_info *info);

/* The same uutigs, built from rank-local fragments instead of a replicated union: what
 * traverse_debruijn_graph does at rank_n() > 1, walking inside a rank and joining the fragments that cross ranks
 * (connect_frags, src/dbjg_traversal.cpp:291-335,517-567). The contract is mhmkc_uutigs_ranks's, word for word: the
 * contigs, the owner rule, the order, the global ids and the row map, none of which depend on the number of ranks; after a
 * successful call mhmkc_uutigs, mhmkc_uutigs_fetch, mhmkc_uutigs_device, mhmkc_uutig_rows[_device], mhmkc_uutigs_info
 * (n_ctgs, n_bases) and mhmkc_add_ctgs_from(next, h) answer for this rank exactly as after mhmkc_uutigs_ranks. Kept
 * until the next reset / finish / destroy and counted in mhmkc_stats.device_bytes[_peak].
 *   One build per finish: whichever of mhmkc_uutigs_ranks and mhmkc_uutigs_frags runs first after a finish builds; a
 *   later call of either returns the kept values and runs no collective. After a fragment build mhmkc_uutigs_ranks_info
 *   fills only n_ctgs, n_bases, first_id, n_ctgs_all, n_rows, n_rows_all and kept_bytes (the rest is zero), and after a
 *   replicated build mhmkc_uutigs_frags_info fills only the same seven.
 * How: 1. claims: every own port whose routed link (mhmkc_dbjg_links_ranks, built first if the handle has none, which is
 * itself a collective) is OK and names a row of another rank tells that rank which port it enters; a port is
 * cross-linked iff its own link is OK, points at another rank and it received the claim of exactly the port it points at,
 * naming it: the linked-port rule of mhmkc_uutigs with its two halves on two ranks. 2. local ranking: the rank's own
 * rows under links whose cross-rank neighbours are ends, with mhmkc_uutigs's kernels; what lies between two ends is a
 * fragment, closed (a contig of the union, cycles on one rank included) when neither end port is cross-linked, else
 * open. 3. every open fragment's record is gathered on every rank: the only replicated state. 4. every rank ranks the
 * fragment graph (fragments as rows, cross links as links) by the same pointer jumping with weighted states. 5. a
 * cross-rank contig belongs to the rank of its start row; every rank sorts its contigs by start key; the ranks gather
 * their contig counts and the owners the global ids of the cross-rank contigs. 6. every row gets its final place; the
 * open fragments of contigs another rank owns send that rank their bases, one segment per fragment.
 * Memory and traffic follow a rank's own rows and the open fragments of all ranks (frags_open_all), not the union's rows;
 * the fragment graph is replicated, so they shrink to the share of fragments and do not fall as 1 / n_ranks.
 * Bytes per record moved, per stage: MHMKC_UFRAGS_CLAIMS 12 (claiming row u32, entered row u32, directions u32);
 * MHMKC_UFRAGS_GATHER 8 NL + 48 (the start key; the sum of the counts; start row and rows; the two end rows; the two
 * peer rows; start count, ranks and directions; the start's position), sent to every other rank; MHMKC_UFRAGS_IDS 4 (a
 * cross-rank contig's global id), sent to every other rank; MHMKC_UFRAGS_BASES 1 (a base: a row's, or one of the k - 1
 * behind a contig's last row). _LOCAL and _RANK move nothing. The fixed-size all-gathers of counts and verdicts between
 * the stages (a few words per rank) are not counted.
 * scratch_bytes <= MHMKC_UFRAG_SCRATCH_ROW * n_rows + MHMKC_UFRAG_SCRATCH_FRAG * frags_open_all +
 *   (k + MHMKC_UFRAG_SCRATCH_CTG) * ctgs_cross_all + n_bases + MHMKC_UFRAG_SCRATCH_FIXED + 16 * n_ranks^2
 * (n_bases, this rank's kept bases, bounds the bases it receives); nothing is allocated in proportion to the union's
 * rows. The scratch of a links build inside the call is mhmkc_route_info's.
 * Collective over the ranks of a finished MHMKC_OWNER_MINIMIZER handle. n_ranks == 1: mhmkc_uutigs with *first_id = 0.
 * n_ranks > 1 with MHMKC_OWNER_HASH: MHMKC_EUNSUPPORTED; before finish: MHMKC_ESTATE; both before any collective, in that
 * order. A failure on any rank after the first collective is a failure on every rank: MHMKC_ETRANSPORT on the ranks that
 * did not fail themselves. Limits: a rank's own rows, the open fragments of all ranks together and the contigs of all
 * ranks together are each at most 2^32-2 (MHMKC_EUNSUPPORTED beyond, on every rank); the union's rows are not limited,
 * but one contig's are: n_kmers and the ranking's row counts are 32 bits, as in mhmkc_uutigs, so a contig has at most
 * 2^32-2 rows. This last limit is not checked.
 * Any output pointer may be NULL. */
int mhmkc_uutigs_frags(mhmkc_t h, uint64_t *n_ctgs, uint64_t *n_bases, uint64_t *first_id, uint64_t *n_ctgs_all);

enum { MHMKC_UFRAGS_CLAIMS = 0, MHMKC_UFRAGS_LOCAL = 1, MHMKC_UFRAGS_GATHER = 2, MHMKC_UFRAGS_RANK = 3,
       MHMKC_UFRAGS_IDS = 4, MHMKC_UFRAGS_BASES = 5, MHMKC_UFRAGS_STAGES = 6 };
#define MHMKC_UFRAG_CLAIM_BYTES 12
#define MHMKC_UFRAG_RECORD_BYTES(n_longs) (8 * (n_longs) + 48)
#define MHMKC_UFRAG_ID_BYTES 4
#define MHMKC_UFRAG_BASE_BYTES 1
#define MHMKC_UFRAG_SCRATCH_ROW 320
#define MHMKC_UFRAG_SCRATCH_FRAG 448
#define MHMKC_UFRAG_SCRATCH_CTG 8
#define MHMKC_UFRAG_SCRATCH_FIXED (1 << 20)
/* How the last mhmkc_uutigs_frags went. Every field is a uint64_t or a double. */
typedef struct {
  uint64_t n_ctgs, n_bases;      /* this rank's */
  uint64_t first_id, n_ctgs_all;
  uint64_t n_rows, n_rows_all;   /* this rank's rows, the union's */
  uint64_t frags_open;           /* this rank's fragments with a cross-linked end port */
  uint64_t frags_open_all;       /* of all ranks: the rows of the replicated fragment graph */
  uint64_t frags_closed;         /* this rank's fragments that are contigs of the union */
  uint64_t local_cycles;         /* of them, cycles */
  uint64_t cross_links;          /* own ports with a mutual link to another rank */
  uint64_t ctgs_cross_all;       /* contigs made of open fragments, of all ranks */
  uint64_t ctgs_cross_mine;      /* of them, this rank's */
  uint64_t cycles_cross_all;     /* of them, cycles */
  uint64_t rounds_local, cycle_rounds_local; /* pointer-jumping rounds of the local ranking: all ports, cycle ports alone */
  uint64_t rounds_frags, cycle_rounds_frags; /* the same of the fragment ranking */
  uint64_t links_built;          /* 1: this call built the routed links first */
  uint64_t records_sent[MHMKC_UFRAGS_STAGES], records_recv[MHMKC_UFRAGS_STAGES];
  uint64_t bytes_sent[MHMKC_UFRAGS_STAGES], bytes_recv[MHMKC_UFRAGS_STAGES];
  double ms_stage[MHMKC_UFRAGS_STAGES]; /* device events on the handle's stream (a stage's move and its host staging included) */
  double ms_total;
  uint64_t scratch_bytes;        /* the peak of the build's device memory above what stays */
  uint64_t kept_bytes;           /* what stays: this rank's contig arrays and row map */
} mhmkc_uutig_frags_info;
int mhmkc_uutigs_frags_info(mhmkc_t h, mhmkc_uutig_frags_info *info);

/* Queries answered by the rank that owns the key, and every row's de Bruijn links with neighbours on any rank
 * (DESIGN.md §3.11b). The reference's traversal computes get_kmer_target_rank of a neighbour and asks that rank by rpc
 * (src/dbjg_traversal.cpp:228-236,260-274, src/kcount/kmer_dht.cpp:193-219); here every rank hands over a batch, the
 * batches are grouped by owner on the GPUs, travel over the handle's transport (RCCL or mhmkc_set_transport), are
 * answered from the owner's own index and travel back. A rank holds state proportional to its own rows: nothing of
 * another rank's table is kept or indexed.
 * Both calls are collective over the ranks of a finished MHMKC_OWNER_MINIMIZER handle: every rank calls them, in the same
 * order. The work goes in rounds of at most MHMKC_ROUTE_CHUNK queries per rank (an environment variable read at the
 * call, default 2^22, at most 2^30); the number of rounds is the largest over the ranks, so a rank with fewer queries
 * (or none) takes part with empty rounds. A round's device scratch is at most chunk * (8 NL + 13) bytes for the asking
 * side, with NL = k / 32 + 1, plus (8 NL + 8) bytes per query received; all of it is freed before the call returns.
 * n_ranks == 1: the single-rank call, with rank 0. n_ranks > 1 with MHMKC_OWNER_HASH: MHMKC_EUNSUPPORTED; before
 * finish: MHMKC_ESTATE; both before any collective, in that order. A rank that cannot allocate gives MHMKC_ENOMEM on
 * every rank before a byte of that round moves; any other failure on one rank after the first collective is a failure
 * on every rank: MHMKC_ETRANSPORT on the ranks that did not fail themselves. */
#define MHMKC_NO_RANK 0xFFu

/* mhmkc_lookup for keys that may live on any rank (get_kmer_target_rank + the rpc to get_local_kmer_counts,
 * src/kcount/kmer_dht.cpp:193-219, src/dbjg_traversal.cpp:228-236). Every rank gives its own n (0 is allowed, with NULL
 * arrays). Query i is canonicalized or not exactly as in mhmkc_lookup. ranks[i] = get_kmer_target_rank of the key that
 * is looked up, always set, on a miss too (a key and its reverse complement have the same owner); rows[i], counts[i],
 * left[i], right[i] are what mhmkc_lookup on that rank's handle returns for the key: rows[i] is the row there, a miss
 * gives MHMKC_NO_ROW and zeros. Any output pointer may be NULL. Host arrays. */
int mhmkc_lookup_ranks(mhmkc_t h, const uint64_t *keys, uint64_t n, int canonicalize, uint8_t *ranks, uint32_t *rows,
                       uint16_t *counts, char *left, char *right);
/* The same with device arrays, on the handle's stream; the outputs are complete when the call returns. */
int mhmkc_lookup_ranks_device(mhmkc_t h, const uint64_t *d_keys, uint64_t n, int canonicalize, uint8_t *d_ranks,
                              uint32_t *d_rows, uint16_t *d_counts, char *d_left, char *d_right);

/* mhmkc_dbjg_links with the neighbour looked up on its target rank (get_next_step at rank_n() > 1,
 * src/dbjg_traversal.cpp:165-239,260-274). Entry d * n_out + i follows the three rules of mhmkc_dbjg_links unchanged, in
 * their order; in step 2 the neighbour is asked of get_kmer_target_rank(neighbour). next_rank / next_row name that rank
 * and the row there; where the single-rank call gives next = MHMKC_NO_ROW they are MHMKC_NO_RANK and MHMKC_NO_ROW.
 * Built by the first call after a finish (a collective) and kept on the device until the next reset / finish / destroy: 6
 * bytes per entry, 12 per row, counted in mhmkc_stats.device_bytes[_peak]; a later call returns the kept arrays and
 * runs no collective. Only a rank's own rows are limited to 2^32-2; the union of the ranks' tables is not. */
int mhmkc_dbjg_links_ranks(mhmkc_t h);
/* Host copies of the kept arrays, 2 * n_out entries each (any may be NULL); builds them first if needed, and is then
 * the collective. */
int mhmkc_dbjg_links_ranks_fetch(mhmkc_t h, uint8_t *next_rank, uint32_t *next_row, uint8_t *status);
/* The kept arrays on the device (builds them first if needed; NULL pointers for a rank without rows). */
int mhmkc_dbjg_links_ranks_device(mhmkc_t h, const uint8_t **d_next_rank, const uint32_t **d_next_row,
                                  const uint8_t **d_status);

/* How the last of the two collectives on this handle went (a call answered from the kept links changes nothing). A
 * query is one key asked of its owner; a link entry that its own row ends asks nothing. (The struct carries a _t, unlike
 * its sibling info structs, because the call is named mhmkc_route_info and C keeps types and functions in one name
 * space.) */
enum { MHMKC_ROUTE_ROUTE = 0, MHMKC_ROUTE_EXCHANGE = 1, MHMKC_ROUTE_ANSWER = 2, MHMKC_ROUTE_RETURN = 3,
       MHMKC_ROUTE_UNPACK = 4, MHMKC_ROUTE_STAGES = 5 };
typedef struct {
  uint64_t rounds;          /* rounds of the call, the largest need over the ranks */
  uint64_t chunk;           /* queries per rank and round (MHMKC_ROUTE_CHUNK) */
  uint64_t entries;         /* what this rank handed over: the batch's n, or 2 * n_out link entries */
  uint64_t queries;         /* queries this rank asked (entries minus those that ask nothing) */
  uint64_t queries_local;   /* of them, answered by this rank itself: they never touch the transport */
  uint64_t queries_sent;    /* of them, sent to other ranks (queries_local + queries_sent == queries) */
  uint64_t queries_recv;    /* queries of other ranks answered here */
  uint64_t bytes_sent;      /* 8 NL per query sent + 8 per reply to a query received */
  uint64_t bytes_recv;      /* 8 NL per query received + 8 per reply to a query sent */
  double ms_stage[MHMKC_ROUTE_STAGES]; /* device events on the handle's stream, summed over the rounds: owners and
                               histogram; pack + the queries' move; the answers; the replies' move; unpack / verdicts
                               (the moves include their host staging under mhmkc_set_transport and the wait for the
                               slowest rank) */
  double ms_total;          /* wall time of the call */
  uint64_t scratch_bytes;   /* the peak of the call's device scratch (asking side + received queries and replies) */
  uint64_t kept_bytes;      /* what stays on the device: the links of mhmkc_dbjg_links_ranks, else 0 */
} mhmkc_route_info_t;
int mhmkc_route_info(mhmkc_t h, mhmkc_route_info_t *info);

/* Assembly statistics and FASTA output from device-resident contigs: what the reference does with its
 * Contigs at the end of every contigging round and of the run, Contigs::print_stats (src/contigs.cpp:92-164;
 * src/contigging.cpp:152, src/main.cpp:216) and Contigs::dump_contigs (src/contigs.cpp:166-180; src/contigging.cpp:147-150,
 * src/main.cpp:213), without the contigs leaving the device as objects.
 *
 * The figures of print_stats over the contigs with len >= min_ctg_len. Integers are exact. tot_depth is a floating sum in
 * a fixed order (chunks of 1024 contigs: four per lane in index order, a tree over 256 lanes, the chunks in order), so it
 * depends on the inputs alone; all.tot_depth is the ranks' mine.tot_depth added in rank order. n50 / l50 (not printed by
 * the reference, whose approximate N50 is commented out, src/contigs.cpp:114-143): with the counted lengths in descending
 * order, l50 is the smallest number of leading contigs whose lengths sum to s with 2 s >= tot_len, n50 the length of the
 * last of them; both 0 when nothing is counted. */
typedef struct {
  uint64_t n_ctgs, tot_len, max_len, n_ns; /* contigs with len >= min_ctg_len; n_ns: bytes equal to 'N' in them */
  double tot_depth;                        /* sum of their depths; the reference prints tot_depth / n_ctgs */
  uint64_t len_sums[5];                    /* bases in contigs of len >= 1000, 5000, 10000, 25000, 50000 (contigs.cpp:96,108-110) */
  uint64_t n50, l50;
} mhmkc_ctg_stats;

/* d_seqs, d_seq_offsets (n_ctgs + 1 entries, the first 0, never falling), d_depths (double): device arrays of the shapes
 * mhmkc_add_ctgs_device takes, read during the call only, on the handle's stream (mhmkc_wait_stream first when another
 * stream wrote them). With n_ctgs == 0 the pointers may be NULL. The handle may be in any state. mine: this rank's
 * contigs; all: the reduction over the ranks of the handle (reduce_one of contigs.cpp:144-148,162, here returned on every
 * rank), n50 / l50 exact over all ranks' contigs (each rank's counted lengths travel as 4 bytes each). Either may be NULL.
 * n_ranks > 1: collective over RCCL or mhmkc_set_transport; a failure on one rank is a failure on all (MHMKC_ETRANSPORT on
 * the others). One rank: all == mine. MHMKC_EINVAL: offsets that do not start at 0 or fall (the message names the first
 * such contig); MHMKC_EUNSUPPORTED: a counted contig of 2^32 bases or more. The call's device scratch (16 bytes per contig)
 * is freed before it returns. */
int mhmkc_ctgs_stats_device(mhmkc_t h, const char *d_seqs, const uint64_t *d_seq_offsets, const double *d_depths,
                            uint64_t n_ctgs, uint32_t min_ctg_len, mhmkc_ctg_stats *mine, mhmkc_ctg_stats *all);
/* The same of the handle's uutigs (mhmkc_uutigs_device). One rank: built first if needed. n_ranks > 1: after
 * mhmkc_uutigs_ranks / mhmkc_uutigs_frags, else MHMKC_EUNSUPPORTED before any collective, as the other getters. */
int mhmkc_uutigs_stats(mhmkc_t h, uint32_t min_ctg_len, mhmkc_ctg_stats *mine, mhmkc_ctg_stats *all);

/* The text dump_contigs writes, built on the device and kept there: for every contig c with len >= min_ctg_len, in order,
 * ">Contig" + to_string(int64 id) + " " + to_string(double depth) + "\n" + seq + "\n" with id = first_id + c, c the index
 * in the unfiltered list. The sequence is written as it is (contigs.cpp:173-176 computes the canonical strand and then
 * writes ctg->seq); no line wrapping. to_string(double) is "%f": six decimals, correctly rounded, ties to even, done in
 * integers on the device.
 * Supported: depths finite with the sign bit clear and < 2^32 (only contigs that are written are checked);
 * first_id + n_ctgs <= 2^63 - 1; offsets as above. Else MHMKC_EINVAL, the message names the first offending contig, found
 * on the device before a byte is written. *n_bytes: this rank's text; *file_offset: the sum of the lower ranks' n_bytes
 * (dist_ofstream's prefix sum, upcxx-utils/src/ofstream.cpp:184,454); *n_bytes_all: the file's size. Any may be NULL.
 * n_ranks > 1: collective (one 16-byte all-gather: status and size); a failure on one rank is a failure on all
 * (MHMKC_ETRANSPORT on the others) and leaves no text.
 * The text stays on the device, one at a time: the next fasta call replaces it, mhmkc_reset, mhmkc_finish and
 * mhmkc_destroy free it; it is counted in mhmkc_stats.device_bytes[_peak]. The scratch (16 bytes per contig) is freed
 * before the call returns. */
int mhmkc_ctgs_fasta_device(mhmkc_t h, const char *d_seqs, const uint64_t *d_seq_offsets, const double *d_depths,
                            uint64_t n_ctgs, uint64_t first_id, uint32_t min_ctg_len, uint64_t *n_bytes,
                            uint64_t *file_offset, uint64_t *n_bytes_all);
/* The same of the handle's uutigs with the first_id of the ranks build (0 on one rank); state rules of mhmkc_uutigs_stats. */
int mhmkc_uutigs_fasta(mhmkc_t h, uint32_t min_ctg_len, uint64_t *n_bytes, uint64_t *file_offset, uint64_t *n_bytes_all);
/* The kept text (NULL when it is empty). Without one: MHMKC_ESTATE. */
int mhmkc_fasta_device(mhmkc_t h, const char **d_text, uint64_t *n_bytes);
/* Copy it to text[n_bytes] (host). */
int mhmkc_fasta_fetch(mhmkc_t h, char *text);
/* Write it to the file at `path`, at file_offset: chunks of fasta_chunk_bytes (mhmkc_debug_set; default 4 MiB, at least
 * 64) are copied into two pinned buffers in turn, chunk c + 1 on the wire while chunk c is written with pwrite.
 * One rank: the file is created, truncated and written. n_ranks > 1: collective. Rank 0 creates and truncates the file
 * and sets its length to n_bytes_all; the ranks exchange their status (which is the barrier); every rank with bytes opens
 * the file and writes its block; the ranks exchange their status again. A rank without bytes opens nothing. All ranks
 * must see the same file under `path` (one node, or a shared file system). Offsets are 64-bit. MHMKC_EIO with the
 * errno text on the rank that failed, MHMKC_ETRANSPORT on the others. */
int mhmkc_fasta_write(mhmkc_t h, const char *path);
/* How the last fasta build and the last mhmkc_fasta_write went. Every field is a uint64_t or a double. */
typedef struct {
  uint64_t n_ctgs, n_written;   /* contigs given; of them in the text */
  uint64_t n_bytes, file_offset, n_bytes_all;
  uint64_t text_bytes;          /* device memory of the kept text */
  uint64_t scratch_bytes;       /* the build's device scratch */
  double ms_table, ms_copy, ms_headers, ms_total; /* device events: checks + lengths + scan; bases; headers */
  uint64_t write_chunks;        /* chunks of the last mhmkc_fasta_write */
  double ms_write;              /* its wall time, status exchanges included */
} mhmkc_fasta_info_t;
int mhmkc_fasta_info(mhmkc_t h, mhmkc_fasta_info_t *info);

/* Host-staged exchange between ranks (instead of RCCL): for n_ranks > 1 with comm_id == NULL, set before
 * the first mhmkc_finish. Every rank's callbacks are called collectively, in the same order on all ranks, with
 * host buffers; a callback returns 0 on success.
 *   allgather: every rank contributes `bytes` bytes from send; recv receives n_ranks * bytes, rank order;
 *   alltoallv: send holds, back to back in rank order, send_bytes[p] bytes for every rank p (0 for itself);
 *              recv receives recv_bytes[p] bytes from every rank p, back to back in rank order.
 * This is the seam a UPC++ / MPI host (several nodes, or several ranks sharing one GPU) plugs into; the
 * reference's own transport is UPC++ RPC (src/kcount/kmer_dht.cpp:133-149,222-231). */
typedef struct {
  void *ctx;
  int (*allgather)(void *ctx, const void *send, void *recv, uint64_t bytes);
  int (*alltoallv)(void *ctx, const void *send, const uint64_t *send_bytes, void *recv, const uint64_t *recv_bytes);
} mhmkc_transport;
int mhmkc_set_transport(mhmkc_t h, const mhmkc_transport *t);

/* Kmer::minimizer_hash_fast(m) of n k-mers of the handle's k (src/kmer.cpp:344-393,454-463), computed on the
 * handle's GPU: keys[n * n_longs] in Kmer::longs layout (host), hashes[n] (host). get_kmer_target_rank is
 * hashes[i] % rank_n (src/kcount/kmer_dht.cpp:193-196). m = 0: the KmerDHT minimizer length for k. */
int mhmkc_minimizer_hashes(mhmkc_t h, const uint64_t *keys, uint64_t n, int32_t n_longs, int32_t m, uint64_t *hashes);

/* Statistics of the last round. */
int mhmkc_get_stats(mhmkc_t h, mhmkc_stats *s);

/* Forget all k-mers (keep allocations) so the handle can count the next batch/round
 * (KmerDHT::clear_stores + a fresh HashTableInserter, src/kcount/kcount.cpp:156). */
int mhmkc_reset(mhmkc_t h);

/* Per-stage HIP-event timing (mhmkc_stats.ms_kernel). Off by default (0); 1: every stage; 2: the heavy stages only
 * (extraction scatter, fine scatter, exchange, count), whose events cost the step less. */
int mhmkc_set_profiling(mhmkc_t h, int on);

/* Last error message of the handle (or of the last failed mhmkc_create when h is NULL). */
const char *mhmkc_last_error(mhmkc_t h);

/* Library ABI version (MHMKC_ABI_VERSION). */
int mhmkc_abi_version(void);

/* Build id of this library: the first 16 hex digits of the SHA-256 of the sources it was compiled from
 * (mhm2_proxy_amd/build.py: LIB_DEPS, paths and contents), fixed at compile time. A loader compares it with the id
 * of the tree it runs from to know that the binary it mapped is the one those sources make ("unknown": built
 * without build.py). Not part of the reference (provenance of the prebuilt library only). */
const char *mhmkc_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* MHMKC_H */
