"""Host-side mirror of the reference kcount interface over the C ABI of libmhmkc.so.

Reference shapes kept (ajpowelsnl/mhm2_proxy):
  * PackedRead / PackedReads        src/packed_reads.hpp:60-167, src/packed_reads.cpp:73-159
  * Kmer<MAX_K> longs layout        src/kmer.hpp:61-160 (here: a tuple/array of n_longs uint64)
  * KmerCounts{count, left, right}  src/kcount/kmer_dht.hpp:62-68
  * KmerDHT (local_kmers, get_local_kmer_counts, get_kmer_target_rank, dump_kmers)
                                    src/kcount/kmer_dht.hpp:118-172, src/kcount/kmer_dht.cpp
  * analyze_kmers(...)              src/kcount/kcount.hpp:71-73, src/kcount/kcount.cpp:140-157

The counting itself always runs on the GPU through libmhmkc.so; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import gzip
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Iterable, NamedTuple, Sequence

import numpy as np

from . import _native as N

NUCLEOTIDE_MAP = "ACGTN"
_BASE_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
_IUPAC = set("URYKMSWBDHV")  # mapped to N by the PackedRead constructor (packed_reads.cpp:90-101)


def n_longs_for(k: int) -> int:
    """N_LONGS of Kmer<MAX_K> with MAX_K = (k/32+1)*32 (src/main.cpp:170, src/kmer.hpp:64)."""
    return k // 32 + 1


def split_reads_fname(name: str) -> tuple:
    """A read library's name as FastqReader's constructor reads it (src/fastq.cpp:250-262; the first colon splits):
    "a:b" -> ("mates", a, b), two mate files; "a:" -> ("single", a, None), one unpaired file; "a" ->
    ("interleaved", a, None). What mhmkc_add_fastq_named does with each. An empty first part raises ValueError."""
    a, colon, b = str(name).partition(":")
    if not a:
        raise ValueError(f"reads file name {name!r}: no first file")
    if not colon:
        return ("interleaved", a, None)
    return ("mates", a, b) if b else ("single", a, None)


# ------------------------------------------------------------------------------------------------
# Kmer helpers (2-bit MSB-first longs, src/kmer.cpp:178-188)


def kmer_from_string(s: str, n_longs: int | None = None) -> tuple:
    """set_kmer (src/kmer.cpp:274-296): A0 C1 G2 T3, the bit trick maps N to G."""
    k = len(s)
    nl = n_longs or n_longs_for(k)
    longs = [0] * nl
    for i, ch in enumerate(s):
        c = ord(ch)
        x = (c & 4) >> 1
        code = x + ((x ^ (c & 2)) >> 1)
        longs[i // 32] |= code << (2 * (31 - i % 32))
    return tuple(longs)


def kmer_to_string(longs: Sequence[int], k: int) -> str:
    """to_string (src/kmer.cpp:595-634)."""
    return "".join("ACGT"[(int(longs[i // 32]) >> (2 * (31 - i % 32))) & 3] for i in range(k))


def keys_to_strings(keys: np.ndarray, k: int) -> list:
    """Vectorised to_string for an (n, n_longs) uint64 key array."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.shape[0]
    out = np.empty((n, k), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(k):
        w = keys[:, i // 32]
        out[:, i] = lut[((w >> np.uint64(2 * (31 - i % 32))) & np.uint64(3)).astype(np.intp)]
    return [bytes(r).decode() for r in out]


# ------------------------------------------------------------------------------------------------
# PackedReads


class PackedReads:
    """Reads in the PackedRead byte layout: one byte per base, code (A0 C1 G2 T3 N4) | min(q-off,31) << 3.

    Mirrors src/packed_reads.hpp:120-167. Reads are stored contiguously (bytes + CSR offsets) so the
    whole set can be handed to the device in one copy.
    """

    def __init__(self, qual_offset: int = 33, fname: str = ""):
        if qual_offset not in (33, 64):
            raise ValueError("qual_offset must be 33 or 64")
        self.qual_offset = qual_offset
        self.fname = fname
        self._chunks: list[np.ndarray] = []
        self._lens: list[int] = []
        self._ids: list[int] = []
        self._bytes: np.ndarray | None = None
        self._offsets: np.ndarray | None = None
        self.index = 0
        self.max_read_len = 0

    @classmethod
    def from_arrays(cls, packed_bytes: np.ndarray, offsets: np.ndarray, qual_offset: int = 33) -> "PackedReads":
        pr = cls(qual_offset)
        pr._bytes = np.ascontiguousarray(packed_bytes, dtype=np.uint8)
        pr._offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if pr._offsets.size == 0 or pr._offsets[0] != 0 or int(pr._offsets[-1]) != pr._bytes.size:
            raise ValueError("offsets must start at 0 and end at len(bytes)")
        lens = np.diff(pr._offsets)
        pr.max_read_len = int(lens.max()) if lens.size else 0
        return pr

    @staticmethod
    def pack(seq: str, quals: str, qual_offset: int = 33) -> np.ndarray:
        """PackedRead constructor encoding (src/packed_reads.cpp:73-109); raises on illegal characters
        (the reference DIEs)."""
        if len(seq) != len(quals):
            raise ValueError("seq and quals differ in length")
        if len(seq) > 65535:
            raise ValueError("read longer than 65535 (read_len is uint16)")
        out = np.empty(len(seq), dtype=np.uint8)
        for i, (ch, q) in enumerate(zip(seq, quals)):
            if ch in _BASE_CODE:
                code = _BASE_CODE[ch]
            elif ch in _IUPAC:
                code = 4
            else:
                raise ValueError(f"Illegal char in comp nucleotide of '{ch}'")
            qq = min(ord(q) - qual_offset, 31)
            out[i] = (code | ((qq & 0xFF) << 3)) & 0xFF
        return out

    def add_read(self, read_id: str, seq: str, quals: str) -> None:
        """PackedReads::add_read (src/packed_reads.cpp:236-244)."""
        if self._bytes is not None:
            self._materialized_to_chunks()
        self._chunks.append(self.pack(seq, quals, self.qual_offset))
        self._lens.append(len(seq))
        self.max_read_len = max(self.max_read_len, len(seq))

    def _materialized_to_chunks(self):
        b, o = self._bytes, self._offsets
        self._chunks = [b[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        self._lens = [int(o[i + 1] - o[i]) for i in range(len(o) - 1)]
        self._bytes = self._offsets = None

    def _materialize(self):
        if self._bytes is None:
            lens = np.asarray(self._lens, dtype=np.uint64)
            self._offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
            np.cumsum(lens, out=self._offsets[1:])
            self._bytes = (np.concatenate(self._chunks) if self._chunks else np.zeros(0, np.uint8)).astype(np.uint8)
            self._chunks, self._lens = [], []

    @property
    def packed_bytes(self) -> np.ndarray:
        self._materialize()
        return self._bytes

    @property
    def offsets(self) -> np.ndarray:
        self._materialize()
        return self._offsets

    def get_local_num_reads(self) -> int:
        return len(self.offsets) - 1

    def get_bases(self) -> int:
        return int(self.offsets[-1])

    def get_max_read_len(self) -> int:
        return self.max_read_len

    def reset(self) -> None:
        self.index = 0

    def get_read(self, i: int) -> tuple[str, str, str]:
        """PackedRead::unpack (src/packed_reads.cpp:147-159); ids are synthetic '@r<i>/1'."""
        b = self.packed_bytes[int(self.offsets[i]):int(self.offsets[i + 1])]
        seq = "".join(NUCLEOTIDE_MAP[int(x) & 7] for x in b)
        quals = "".join(chr(self.qual_offset + (int(x) >> 3)) for x in b)
        return f"@r{i}/1", seq, quals

    def get_next_read(self):
        if self.index >= self.get_local_num_reads():
            return None
        r = self.get_read(self.index)
        self.index += 1
        return r


# ------------------------------------------------------------------------------------------------
# The counter (C ABI wrapper)


class KmerCounts(NamedTuple):
    """KmerCounts (src/kcount/kmer_dht.hpp:62-68) without the dbjg-only uutig_frag pointer."""
    count: int
    left: str
    right: str


@dataclass
class KmerTable:
    """Finished count table on the host: keys (n, n_longs) uint64, counts uint16, left/right bytes."""
    k: int
    keys: np.ndarray
    counts: np.ndarray
    left: np.ndarray
    right: np.ndarray

    def __len__(self) -> int:
        return int(self.counts.shape[0])

    def sorted(self) -> "KmerTable":
        """Rows in Kmer::operator< order (word-wise unsigned, src/kmer.cpp:265-272)."""
        if len(self) == 0:
            return self
        order = np.lexsort(tuple(self.keys[:, w] for w in range(self.keys.shape[1] - 1, -1, -1)))
        return KmerTable(self.k, self.keys[order], self.counts[order], self.left[order], self.right[order])

    def lines(self) -> Iterable[str]:
        """dump_kmers line format "KMER count L R" (src/kcount/kmer_dht.cpp:243-266)."""
        strs = keys_to_strings(self.keys, self.k)
        for s, c, l, r in zip(strs, self.counts, self.left, self.right):
            yield f"{s} {int(c)} {chr(int(l))} {chr(int(r))}"


class KmerCounter:
    """One GPU's k-mer counter; wraps mhmkc_* (include/mhmkc.h).

    The lifecycle mirrors HashTableInserter (src/kcount/kmer_dht.hpp:95-116): construct (init), add reads
    (insert_supermer via process_seq), finish (flush_inserts + insert_into_local_hashtable), fetch.
    """

    def __init__(self, k: int, *, n_longs: int = 0, qual_offset: int = 33, qual_cutoff: int = 20,
                 dmin_thres: int = 2, dyn_min_depth: float = 0.9, device: int = -1, rank: int = 0,
                 n_ranks: int = 1, comm_id: bytes | None = None, stream: int | None = None,
                 transport: "TorchDistTransport | None" = None, output_owner: int = N.MHMKC_OWNER_HASH,
                 minimizer_len: int = 0):
        L = N.lib()
        cfg = N.MhmkcConfig()
        N.check(L.mhmkc_config_init(C.byref(cfg)))
        cfg.k, cfg.n_longs, cfg.qual_offset, cfg.qual_cutoff = k, n_longs, qual_offset, qual_cutoff
        cfg.dmin_thres, cfg.dyn_min_depth, cfg.device = dmin_thres, dyn_min_depth, device
        cfg.rank, cfg.n_ranks = rank, n_ranks
        cfg.output_owner, cfg.minimizer_len = output_owner, minimizer_len
        self._comm_buf = None
        if comm_id is not None:
            if len(comm_id) != N.MHMKC_COMM_ID_BYTES:
                raise ValueError("comm_id must be 128 bytes")
            self._comm_buf = C.create_string_buffer(bytes(comm_id), N.MHMKC_COMM_ID_BYTES)
            cfg.comm_id = C.cast(self._comm_buf, C.c_void_p)
        cfg.stream = stream
        h = C.c_void_p()
        N.check(L.mhmkc_create(C.byref(h), C.byref(cfg)))
        self._h = h
        self.k = k
        self.n_longs = n_longs or n_longs_for(k)
        self.rank, self.n_ranks = rank, n_ranks
        self.n_out = None
        self._transport = None
        if transport is not None:
            self.set_transport(transport)

    # -- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            N.lib().mhmkc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        N.check(rc, self._h)

    # -- input
    def add_packed_reads(self, packed_bytes: np.ndarray, offsets: np.ndarray) -> None:
        b = np.ascontiguousarray(packed_bytes, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        if o.size < 1:
            raise ValueError("offsets needs n_reads + 1 entries")
        self._check(N.lib().mhmkc_add_reads(self._h, b.ctypes.data, o.ctypes.data, o.size - 1))

    def add_packed_reads_device(self, bytes_ptr: int, offsets_ptr: int, n_reads: int, n_bases: int) -> None:
        self._check(N.lib().mhmkc_add_reads_device(self._h, bytes_ptr, offsets_ptr, n_reads, n_bases))

    def wait_stream(self, stream_ptr: int | None) -> None:
        """Order the counter's device work after what is enqueued on another stream (mhmkc_wait_stream)."""
        self._check(N.lib().mhmkc_wait_stream(self._h, stream_ptr))

    def _after_torch(self, t) -> None:
        """Device tensors are read on the counter's own stream: order it after torch's current stream."""
        import torch

        self.wait_stream(torch.cuda.current_stream(t.device).cuda_stream)

    def add_tensors(self, bytes_t, offsets_t, n_bases: int | None = None) -> None:
        """Device-resident torch tensors (uint8 bytes, int64/uint64 offsets with n_reads+1 entries). n_bases
        defaults to offsets_t[-1] (one device read); the library checks the offsets on the device."""
        n_reads = int(offsets_t.numel()) - 1
        if n_bases is None:
            n_bases = int(offsets_t[-1]) if n_reads >= 0 else 0
        if n_bases > int(bytes_t.numel()):
            raise ValueError("offsets_t[-1] exceeds the bytes tensor")
        self._after_torch(bytes_t)
        self.add_packed_reads_device(bytes_t.data_ptr(), offsets_t.data_ptr(), n_reads, n_bases)

    def add_fastq(self, text) -> None:
        """FASTQ text (bytes or str), parsed and packed on the device, then counted: FastqReader +
        PackedRead construction (src/fastq.cpp:504-551, src/packed_reads.cpp:73-109) for reads that reach
        kcount unmerged. Malformed input raises MhmkcError where the reference DIEs."""
        blob = text.encode("ascii") if isinstance(text, str) else bytes(text)
        self._check(N.lib().mhmkc_add_fastq(self._h, blob, len(blob)))

    def add_fastq_pairs(self, text) -> None:
        """Interleaved paired FASTQ text (mates /1, /2 back to back), parsed on the device, the pairs merged as
        merge_reads does (src/merge_reads.cpp:237-588: merged read + dummy "N" mate, or both mates), then
        counted. stats() reports fq_pairs / fq_merged / fq_ambiguous / fq_overlap_bases; fastq_packed() returns
        merge_reads' PackedReads."""
        blob = text.encode("ascii") if isinstance(text, str) else bytes(text)
        self._check(N.lib().mhmkc_add_fastq_pairs(self._h, blob, len(blob)))

    def add_fastq_file(self, path, pairs: bool = False) -> None:
        """A FASTQ file (interleaved pairs with pairs=True) read in blocks into pinned memory, each block parsed
        and counted on the device while the next is read (mhmkc_add_fastq_file: the file I/O overlapped with the
        kernels). Block size: MHMKC_FQ_BLOCK bytes (default 256 MB). fastq_packed() then holds the PackedReads of
        the whole file (for the later k rounds, as the reference keeps packed_reads_list)."""
        fn = N.lib().mhmkc_add_fastq_pairs_file if pairs else N.lib().mhmkc_add_fastq_file
        self._check(fn(self._h, os.fsencode(str(path))))

    def add_fastq_tensor(self, text_t, n_bytes: int | None = None, pairs: bool = False) -> None:
        """FASTQ text already in HBM (a uint8 torch tensor on the counter's device). The parser reads whole
        aligned dwords, so the buffer must extend 4 bytes past the text: pass n_bytes <= numel - 4 to use the
        tensor as is; otherwise the text is copied into a padded buffer first."""
        import torch

        n = int(text_t.numel()) if n_bytes is None else int(n_bytes)
        if int(text_t.numel()) < n + 4:
            padded = torch.zeros(n + 16, dtype=torch.uint8, device=text_t.device)
            padded[:n].copy_(text_t.reshape(-1)[:n])
            text_t = padded
        self._fq_text = text_t  # keep it alive while the call runs
        self._after_torch(text_t)
        fn = N.lib().mhmkc_add_fastq_pairs_device if pairs else N.lib().mhmkc_add_fastq_device
        self._check(fn(self._h, text_t.data_ptr(), n))

    def add_fastq_mates(self, text1, text2) -> None:
        """Read pairs as two FASTQ texts, the mates /1 in text1 and the mates /2 in text2 (the reference's library
        "r1.fq:r2.fq", src/main.cpp:110-119, which FastqReader alternates between, src/fastq.cpp:509-518): the
        result of add_fastq_pairs on the interleaving of the records read, without making that interleaving."""
        b1 = text1.encode("ascii") if isinstance(text1, str) else bytes(text1)
        b2 = text2.encode("ascii") if isinstance(text2, str) else bytes(text2)
        self._check(N.lib().mhmkc_add_fastq_mates(self._h, b1, len(b1), b2, len(b2)))

    def add_fastq_mates_tensors(self, t1, t2, n1: int | None = None, n2: int | None = None) -> None:
        """add_fastq_mates on texts already in HBM (uint8 torch tensors on the counter's device, anywhere in memory,
        in either order). Each buffer must extend 4 bytes past its text (pass n <= numel - 4 to use a tensor as is;
        otherwise that text is copied into a padded buffer first)."""
        import torch

        ts, ns = [], []
        for t, n in ((t1, n1), (t2, n2)):
            n = int(t.numel()) if n is None else int(n)
            if int(t.numel()) < n + 4:
                padded = torch.zeros(n + 16, dtype=torch.uint8, device=t.device)
                padded[:n].copy_(t.reshape(-1)[:n])
                t = padded
            ts.append(t)
            ns.append(n)
        self._fq_text = ts  # keep them alive while the call runs
        self._after_torch(ts[0])
        self._check(N.lib().mhmkc_add_fastq_mates_device(self._h, ts[0].data_ptr(), ns[0], ts[1].data_ptr(), ns[1]))

    def add_fastq_mates_files(self, path1, path2) -> None:
        """Two mate files read in rounds of MHMKC_FQ_BLOCK bytes per file (mhmkc_add_fastq_mates_files): each round
        merges the pairs both texts hold complete and every file carries its own remainder; the next round's bytes
        are read while the device works. fastq_packed() then holds the PackedReads of all rounds."""
        self._check(N.lib().mhmkc_add_fastq_mates_files(self._h, os.fsencode(str(path1)), os.fsencode(str(path2))))

    def add_fastq_named(self, name) -> None:
        """A read library named as the reference's reads_fname (split_reads_fname): "a:b" two mate files, "a:" one
        unpaired file, "a" one interleaved file."""
        self._check(N.lib().mhmkc_add_fastq_named(self._h, os.fsencode(str(name))))

    def fastq_mates_info(self) -> dict:
        """mhmkc_fastq_mates_info of the last add_fastq_mates* call."""
        info = N.MhmkcFastqMatesInfo()
        self._check(N.lib().mhmkc_fastq_mates_info(self._h, C.byref(info)))
        return info.as_dict()

    def fastq_packed(self) -> tuple[np.ndarray, np.ndarray]:
        """The PackedReads (bytes, offsets) of the last add_fastq call, copied to the host."""
        n_reads, n_bases = C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_fastq_packed(self._h, None, None, C.byref(n_reads), C.byref(n_bases)))
        b = np.empty(int(n_bases.value), dtype=np.uint8)
        o = np.empty(int(n_reads.value) + 1, dtype=np.uint64)
        self._check(N.lib().mhmkc_fastq_fetch(self._h, b.ctypes.data, o.ctypes.data))
        return b, o

    def add_reads(self, reads: PackedReads) -> None:
        self.add_packed_reads(reads.packed_bytes, reads.offsets)

    def add_seqs(self, seqs: Sequence[str], depth: int = 1) -> None:
        """Sequences whose lowercase letters mark bases below the quality cutoff (the string given to
        SeqBlockInserter::process_seq, src/kcount/kcount.cpp:80-86)."""
        lens = np.fromiter((len(s) for s in seqs), dtype=np.uint64, count=len(seqs))
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens, out=offs[1:])
        blob = "".join(seqs).encode("ascii")
        self._check(N.lib().mhmkc_add_seqs(self._h, blob, offs.ctypes.data, len(seqs), depth))

    def add_ctgs(self, seqs: Sequence[str], depths) -> None:
        """Contigs for the contig pass (add_ctg_kmers, src/kcount/kcount.cpp:100-138): uint16 depths as
        Contig::get_uint16_t_depth() gives them (src/contigs.hpp:65). Applied at finish, after the reads,
        in the order added."""
        d = np.ascontiguousarray(depths, dtype=np.uint16)
        if d.size != len(seqs):
            raise ValueError("one depth per contig")
        lens = np.fromiter((len(s) for s in seqs), dtype=np.uint64, count=len(seqs))
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens, out=offs[1:])
        blob = "".join(seqs).encode("ascii")
        self._check(N.lib().mhmkc_add_ctgs(self._h, blob, offs.ctypes.data, d.ctypes.data, len(seqs)))

    def add_ctgs_tensors(self, seqs_t, offsets_t, depths_t, n_bases: int | None = None) -> None:
        """add_ctgs with device-resident torch tensors (mhmkc_add_ctgs_device): uint8 ASCII bases back to back,
        int64/uint64 offsets with n_ctgs + 1 entries, one depth per contig as float64 (a Contig::depth, converted as
        Contig::get_uint16_t_depth() does) or uint16. The tensors are read during the call only. n_bases defaults
        to the bases tensor's size; the library checks it against offsets_t[-1] on the device.
        On a counter of several ranks (MHMKC_OWNER_MINIMIZER only) the call is local: every rank passes its own contigs,
        possibly none, ranks may mix this with add_ctgs, and finish() gathers the contigs of all ranks on the device, in
        rank order (ctgs_ranks_info())."""
        import torch

        n_ctgs = int(offsets_t.numel()) - 1
        if n_ctgs < 0:
            raise ValueError("offsets needs n_ctgs + 1 entries")
        if int(depths_t.numel()) != n_ctgs:
            raise ValueError("one depth per contig")
        if seqs_t.dtype != torch.uint8 or offsets_t.dtype not in (torch.int64, torch.uint64):
            raise TypeError("seqs_t must be uint8, offsets_t int64 or uint64")
        if depths_t.dtype == torch.float64:
            kind = N.MHMKC_DEPTH_F64
        elif depths_t.dtype == torch.uint16:
            kind = N.MHMKC_DEPTH_U16
        else:
            raise TypeError("depths_t must be float64 or uint16")
        for t in (seqs_t, offsets_t, depths_t):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("contiguous device tensors expected")
        if n_bases is None:
            n_bases = int(seqs_t.numel())
        if n_bases > int(seqs_t.numel()):
            raise ValueError("n_bases exceeds the bases tensor")
        self._after_torch(seqs_t)
        self._check(N.lib().mhmkc_add_ctgs_device(self._h, seqs_t.data_ptr(), offsets_t.data_ptr(), depths_t.data_ptr(),
                                                  kind, n_ctgs, n_bases))

    def add_ctgs_from(self, other: "KmerCounter") -> None:
        """The uutigs of a finished counter as this round's contigs, handed over on the device (mhmkc_add_ctgs_from):
        the step from one contigging round to the next k (src/contigging.cpp:93-158). The uutigs are built first if
        `other` has none yet. Several ranks (MHMKC_OWNER_MINIMIZER): after other.uutigs_ranks() on every rank, every rank
        hands over its own part of that build; finish() gathers the parts on the device (ctgs_ranks_info())."""
        self._check(N.lib().mhmkc_add_ctgs_from(self._h, other._h))

    def ctgs_ranks_info(self) -> dict:
        """How the contigs of the last finish() of a counter of several ranks reached every rank
        (mhmkc_ctgs_ranks_info): device_route (1: gathered on the device), this rank's and the round's sizes, the bytes this
        rank sent and received, stage times (device events) and the memory of the gathered copy. All zeros before such a
        finish with contigs."""
        info = N.MhmkcCtgRanksInfo()
        self._check(N.lib().mhmkc_ctgs_ranks_info(self._h, C.byref(info)))
        return info.as_dict()

    # -- ranks, thresholds
    def set_transport(self, transport: "TorchDistTransport") -> None:
        """Host-staged exchange between ranks (mhmkc_set_transport), e.g. over a gloo process group."""
        self._transport = transport  # the callbacks must outlive the handle
        self._check(N.lib().mhmkc_set_transport(self._h, C.byref(transport.struct)))

    def set_dmin_thres(self, dmin_thres: int) -> None:
        """The finish's depth threshold, the reference's _dmin_thres (src/kcount/kmer_dht.hpp:57), set by
        analyze_kmers (src/kcount/kcount.cpp:145)."""
        self._check(N.lib().mhmkc_set_dmin_thres(self._h, int(dmin_thres)))

    def minimizer_hashes(self, keys: np.ndarray, m: int = 0) -> np.ndarray:
        """Kmer::minimizer_hash_fast of (n, n_longs) keys, on the GPU (src/kmer.cpp:344-393,454-463)."""
        kk = np.ascontiguousarray(keys, dtype=np.uint64)
        if kk.ndim == 1:
            kk = kk.reshape(-1, 1)
        out = np.empty(kk.shape[0], dtype=np.uint64)
        self._check(N.lib().mhmkc_minimizer_hashes(self._h, kk.ctypes.data, kk.shape[0], kk.shape[1], m,
                                                   out.ctypes.data))
        return out

    def target_ranks(self, keys: np.ndarray, rank_n: int) -> np.ndarray:
        """KmerDHT::get_kmer_target_rank of every key (src/kcount/kmer_dht.cpp:193-196), on the GPU."""
        return (self.minimizer_hashes(keys) % np.uint64(rank_n)).astype(np.int64)

    # -- finish / output
    def finish(self) -> int:
        n = C.c_uint64()
        self._check(N.lib().mhmkc_finish(self._h, C.byref(n)))
        self.n_out = int(n.value)
        return self.n_out

    def fetch(self, ordered: bool = False, out: KmerTable | None = None) -> KmerTable:
        """The finished table on the host (mhmkc_fetch). ordered=True: rows in the order of the top 32 bits of
        map_hash(key) (mhmkc_fetch_ordered, a device sort), the slot order of the C++ adapter's KmerMap.
        out: a table whose arrays are filled (at least n_out rows; e.g. pinned host memory, which the copies reach
        directly) instead of new ones."""
        if self.n_out is None:
            raise RuntimeError("fetch before finish")
        n = self.n_out
        if out is not None:
            # (the native copy writes n * 8 * n_longs, n * 2, n and n bytes: the dtypes must be those widths)
            if (len(out) < n or out.keys.ndim != 2 or out.keys.shape[1] != self.n_longs or out.keys.dtype != np.uint64
                    or out.counts.dtype != np.uint16 or out.left.dtype.itemsize != 1 or out.right.dtype.itemsize != 1
                    or min(len(out.counts), len(out.left), len(out.right)) < n
                    or not all(a.flags.c_contiguous for a in (out.keys, out.counts, out.left, out.right))):
                raise ValueError("out: contiguous arrays of at least n_out rows: keys uint64 [n, n_longs], counts "
                                 "uint16, left / right one byte per row")
            keys, counts, left, right = out.keys[:n], out.counts[:n], out.left[:n], out.right[:n]
        else:
            keys = np.empty((n, self.n_longs), dtype=np.uint64)
            counts = np.empty(n, dtype=np.uint16)
            left = np.empty(n, dtype=np.uint8)
            right = np.empty(n, dtype=np.uint8)
        fn = N.lib().mhmkc_fetch_ordered if ordered else N.lib().mhmkc_fetch
        self._check(fn(self._h, keys.ctypes.data, counts.ctypes.data, left.ctypes.data, right.ctypes.data))
        return KmerTable(self.k, keys, counts, left, right)

    def device_output(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(4)]
        n = C.c_uint64()
        self._check(N.lib().mhmkc_device_output(self._h, *(C.byref(p) for p in ptrs), C.byref(n)))
        return {"keys": ptrs[0].value, "counts": ptrs[1].value, "left": ptrs[2].value, "right": ptrs[3].value,
                "n_out": int(n.value), "n_longs": self.n_longs}

    # -- queries on the finished table (mhmkc_lookup, mhmkc_dbjg_links)
    def _query_keys(self, keys) -> np.ndarray:
        if isinstance(keys, (list, tuple)) and (len(keys) == 0 or isinstance(keys[0], str)):
            if any(len(s) != self.k for s in keys):
                raise ValueError(f"every k-mer string must have {self.k} bases")
            keys = np.array([kmer_from_string(s, self.n_longs) for s in keys], dtype=np.uint64)
        kk = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.n_longs)
        return kk

    def lookup(self, keys, canonicalize: bool = False):
        """KmerDHT::get_local_kmer_counts (canonicalize=False: the key as given) or kmer_exists (canonicalize=True:
        min(key, revcomp(key))) for a batch of k-mers, answered on the GPU (src/kcount/kmer_dht.cpp:198-219).
        keys: an (n, n_longs) uint64 array in Kmer::longs layout, or a list of k-mer strings. Returns numpy arrays
        (rows, counts, left, right): rows[i] is the row of fetch() holding key i or MHMKC_NO_ROW (0xFFFFFFFF),
        counts / left / right that row's fields (0 on a miss; left / right in the stored, canonical frame)."""
        kk = self._query_keys(keys)
        n = kk.shape[0]
        rows = np.empty(n, dtype=np.uint32)
        counts = np.empty(n, dtype=np.uint16)
        left = np.empty(n, dtype=np.uint8)
        right = np.empty(n, dtype=np.uint8)
        self._check(N.lib().mhmkc_lookup(self._h, kk.ctypes.data, n, int(bool(canonicalize)), rows.ctypes.data,
                                         counts.ctypes.data, left.ctypes.data, right.ctypes.data))
        return rows, counts, left, right

    def synchronize(self) -> None:
        """Wait for the counter's stream (mhmkc_fetch with no output arrays copies nothing and waits for it)."""
        self._check(N.lib().mhmkc_fetch(self._h, None, None, None, None))

    def lookup_tensors(self, keys_t, canonicalize: bool = False, sync: bool = True):
        """lookup() for keys already in HBM: a uint64 / int64 torch tensor of n * n_longs words on the counter's
        device. Returns torch tensors (rows int32 holding the uint32 bits, so a miss reads -1; counts int16 holding
        the uint16 bits; left, right uint8) allocated by torch and written on the counter's own stream, which is first
        ordered after torch's current stream (as add_tensors). With sync=True (default) the call waits for the
        counter's stream, so the tensors are ready for any stream. With sync=False it returns at once: call
        synchronize() before reading them (or before freeing keys_t), or create the counter on the torch stream that
        consumes them (KmerCounter(stream=torch.cuda.current_stream().cuda_stream)), which orders everything."""
        import torch

        if keys_t.dtype not in (torch.uint64, torch.int64):
            raise ValueError("keys_t must be a uint64 or int64 tensor")
        if not keys_t.is_contiguous() or keys_t.numel() % self.n_longs:
            raise ValueError("keys_t must be contiguous with n * n_longs words")
        n = keys_t.numel() // self.n_longs
        dev = keys_t.device
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int16, device=dev)
        left = torch.empty(n, dtype=torch.uint8, device=dev)
        right = torch.empty(n, dtype=torch.uint8, device=dev)
        self._after_torch(keys_t)
        self._check(N.lib().mhmkc_lookup_device(self._h, keys_t.data_ptr(), n, int(bool(canonicalize)),
                                                rows.data_ptr(), counts.data_ptr(), left.data_ptr(), right.data_ptr()))
        if sync:
            self.synchronize()
        return rows, counts, left, right

    def dbjg_links(self):
        """The de Bruijn links of every row (mhmkc_dbjg_links): numpy arrays next[2, n_out] (uint32 rows, MHMKC_NO_ROW:
        none) and status[2, n_out] (MHMKC_LINK_*), direction 0 = LEFT, 1 = RIGHT, in each row's stored orientation."""
        n = self.n_out or 0  # (before finish the library refuses the call)
        nxt = np.empty((2, n), dtype=np.uint32)
        status = np.empty((2, n), dtype=np.uint8)
        self._check(N.lib().mhmkc_dbjg_links(self._h, nxt.ctypes.data, status.ctypes.data))
        return nxt, status

    def dbjg_links_device(self) -> dict:
        """Device pointers of the link arrays (mhmkc_dbjg_links_device), kept until the next reset / finish."""
        pn, ps = C.c_void_p(), C.c_void_p()
        self._check(N.lib().mhmkc_dbjg_links_device(self._h, C.byref(pn), C.byref(ps)))
        return {"next": pn.value, "status": ps.value, "n_out": self.n_out}

    # -- the uutigs of the finished table (mhmkc_uutigs)
    def uutigs(self):
        """The round's uutigs, built on the GPU from the de Bruijn links (mhmkc_uutigs; traverse_debruijn_graph at one
        rank, src/dbjg_traversal.cpp:404-407,539-596): numpy arrays (offsets uint64 [n_ctgs + 1], seqs uint8 [n_bases]
        holding ASCII ACGT, depths float64 [n_ctgs], n_kmers uint32 [n_ctgs]); contig c is seqs[offsets[c]:offsets[c+1]],
        in the order of the contigs' smallest k-mers (the ids the reference assigns)."""
        nc, nb = C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_uutigs(self._h, C.byref(nc), C.byref(nb)))
        offsets = np.empty(nc.value + 1, dtype=np.uint64)
        seqs = np.empty(nb.value, dtype=np.uint8)
        depths = np.empty(nc.value, dtype=np.float64)
        n_kmers = np.empty(nc.value, dtype=np.uint32)
        self._check(N.lib().mhmkc_uutigs_fetch(self._h, offsets.ctypes.data, seqs.ctypes.data, depths.ctypes.data,
                                               n_kmers.ctypes.data))
        return offsets, seqs, depths, n_kmers

    def uutig_rows(self):
        """Where every row of fetch() lies (mhmkc_uutig_rows): numpy arrays row_ctg uint32 (MHMKC_NO_ROW: in no contig),
        row_pos uint32, row_rc uint8 (1: reverse-complemented in its contig), n_out entries each."""
        n = self.n_out or 0  # (before finish the library refuses the call)
        row_ctg = np.empty(n, dtype=np.uint32)
        row_pos = np.empty(n, dtype=np.uint32)
        row_rc = np.empty(n, dtype=np.uint8)
        self._check(N.lib().mhmkc_uutig_rows(self._h, row_ctg.ctypes.data, row_pos.ctypes.data, row_rc.ctypes.data))
        return row_ctg, row_pos, row_rc

    def uutigs_device(self) -> dict:
        """Device pointers of the contig arrays and the row map (mhmkc_uutigs_device, mhmkc_uutig_rows_device), kept
        until the next reset / finish."""
        po, ps, pd = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nc, nb = C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_uutigs_device(self._h, C.byref(po), C.byref(ps), C.byref(pd), C.byref(nc), C.byref(nb)))
        rc_, rp, rr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(N.lib().mhmkc_uutig_rows_device(self._h, C.byref(rc_), C.byref(rp), C.byref(rr)))
        return {"offsets": po.value, "seqs": ps.value, "depths": pd.value, "n_ctgs": int(nc.value),
                "n_bases": int(nb.value), "row_ctg": rc_.value, "row_pos": rp.value, "row_rc": rr.value,
                "n_out": self.n_out}

    def uutig_strings(self):
        """(list of contig strings, depths float64) in contig order, ready for the next round's add_ctgs (which takes
        Contig::get_uint16_t_depth() of each depth, src/contigs.hpp:65: np.minimum(depths, 65535).astype(np.uint16))."""
        offsets, seqs, depths, _ = self.uutigs()
        blob = seqs.tobytes().decode("ascii")
        return [blob[int(offsets[c]):int(offsets[c + 1])] for c in range(len(depths))], depths

    def uutigs_info(self) -> dict:
        """Rounds, stage times (device events) and memory of the last uutigs build (mhmkc_uutigs_info)."""
        info = N.MhmkcUutigInfo()
        self._check(N.lib().mhmkc_uutigs_info(self._h, C.byref(info)))
        return info.as_dict()

    # -- the uutigs of all ranks' tables (mhmkc_uutigs_ranks)
    def uutigs_ranks(self) -> dict:
        """Collective over the ranks of a finished MHMKC_OWNER_MINIMIZER counter (mhmkc_uutigs_ranks; traverse_debruijn_graph
        at rank_n() > 1, src/dbjg_traversal.cpp:291-335,517-567,569-596): the uutigs of the union of all ranks' tables. This
        rank keeps the contigs whose start row it holds, in start-key order; a contig's global id is first_id + its local
        index. uutigs(), uutig_rows() (row_ctg: global ids), uutigs_device() and uutig_strings() then give this rank's
        part. Returns {"n_ctgs", "n_bases", "first_id", "n_ctgs_all"}. One rank: uutigs() with first_id 0."""
        nc, nb, fi, na = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_uutigs_ranks(self._h, C.byref(nc), C.byref(nb), C.byref(fi), C.byref(na)))
        return {"n_ctgs": int(nc.value), "n_bases": int(nb.value), "first_id": int(fi.value), "n_ctgs_all": int(na.value)}

    def uutigs_ranks_info(self) -> dict:
        """Rounds, rows and bytes moved between the ranks per stage, stage times (device events) and memory of the last
        uutigs_ranks build (mhmkc_uutigs_ranks_info)."""
        info = N.MhmkcUutigRanksInfo()
        self._check(N.lib().mhmkc_uutigs_ranks_info(self._h, C.byref(info)))
        return info.as_dict()

    # -- the same uutigs from rank-local fragments (mhmkc_uutigs_frags)
    def uutigs_frags(self) -> dict:
        """uutigs_ranks() by the fragment build (mhmkc_uutigs_frags): every rank ranks its own rows, the open
        fragments of all ranks are joined in a replicated fragment graph, and only they and the bases of contigs owned
        elsewhere travel. Collective over the ranks of a finished MHMKC_OWNER_MINIMIZER counter; the same contigs, ids and
        row map, and the same kept state: whichever of the two runs first after a finish builds, the other then returns it.
        Returns {"n_ctgs", "n_bases", "first_id", "n_ctgs_all"}."""
        nc, nb, fi, na = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_uutigs_frags(self._h, C.byref(nc), C.byref(nb), C.byref(fi), C.byref(na)))
        return {"n_ctgs": int(nc.value), "n_bases": int(nb.value), "first_id": int(fi.value), "n_ctgs_all": int(na.value)}

    def uutigs_frags_info(self) -> dict:
        """Fragment and contig counts, rounds, records and bytes moved per stage, stage times (device events) and memory of
        the last uutigs_frags build (mhmkc_uutigs_frags_info)."""
        info = N.MhmkcUutigFragsInfo()
        self._check(N.lib().mhmkc_uutigs_frags_info(self._h, C.byref(info)))
        return info.as_dict()

    # -- assembly statistics and FASTA output of device-resident contigs
    def _ctg_tensors(self, seqs_t, offsets_t, depths_t):
        import torch

        n_ctgs = int(offsets_t.numel()) - 1
        if n_ctgs < 0:
            raise ValueError("offsets needs n_ctgs + 1 entries")
        if int(depths_t.numel()) != n_ctgs:
            raise ValueError("one depth per contig")
        if seqs_t.dtype != torch.uint8 or offsets_t.dtype not in (torch.int64, torch.uint64) or \
                depths_t.dtype != torch.float64:
            raise TypeError("seqs_t must be uint8, offsets_t int64 or uint64, depths_t float64")
        for t in (seqs_t, offsets_t, depths_t):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("contiguous device tensors expected")
        self._after_torch(offsets_t)
        return n_ctgs

    def ctgs_stats_tensors(self, seqs_t, offsets_t, depths_t, min_ctg_len: int = 0) -> dict:
        """Contigs::print_stats' figures (src/contigs.cpp:92-164) of device-resident contigs (mhmkc_ctgs_stats_device):
        uint8 ASCII bases back to back, int64/uint64 offsets with n_ctgs + 1 entries, float64 depths. Returns {"mine": this
        rank's, "all": over the ranks of the counter}, each a dict of n_ctgs, tot_len, max_len, n_ns, tot_depth, len_sums
        (bases in contigs of >= 1, 5, 10, 25, 50 kbp), n50 and l50 (exact, over all ranks' contigs). Collective on a
        counter of several ranks. The bases tensor must hold offsets_t[-1] bytes."""
        n_ctgs = self._ctg_tensors(seqs_t, offsets_t, depths_t)
        mine, allr = N.MhmkcCtgStats(), N.MhmkcCtgStats()
        self._check(N.lib().mhmkc_ctgs_stats_device(self._h, seqs_t.data_ptr(), offsets_t.data_ptr(), depths_t.data_ptr(),
                                                    n_ctgs, int(min_ctg_len), C.byref(mine), C.byref(allr)))
        return {"mine": mine.as_dict(), "all": allr.as_dict()}

    def uutigs_stats(self, min_ctg_len: int = 0) -> dict:
        """The same of the counter's uutigs (mhmkc_uutigs_stats): ctgs.print_stats(500) of a contigging round
        (src/contigging.cpp:152). Several ranks: after uutigs_ranks() / uutigs_frags()."""
        mine, allr = N.MhmkcCtgStats(), N.MhmkcCtgStats()
        self._check(N.lib().mhmkc_uutigs_stats(self._h, int(min_ctg_len), C.byref(mine), C.byref(allr)))
        return {"mine": mine.as_dict(), "all": allr.as_dict()}

    def ctgs_fasta_tensors(self, seqs_t, offsets_t, depths_t, first_id: int = 0, min_ctg_len: int = 0) -> dict:
        """The text Contigs::dump_contigs writes (src/contigs.cpp:166-180), built and kept on the device
        (mhmkc_ctgs_fasta_device): ">Contig<first_id + c> <depth as %f>\\n<seq>\\n" for every contig of at least min_ctg_len
        bases. Returns {"n_bytes", "file_offset", "n_bytes_all"}; fasta_bytes(), fasta_tensor() and fasta_write() then
        use the kept text. Collective on a counter of several ranks."""
        n_ctgs = self._ctg_tensors(seqs_t, offsets_t, depths_t)
        nb, fo, na = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_ctgs_fasta_device(self._h, seqs_t.data_ptr(), offsets_t.data_ptr(), depths_t.data_ptr(),
                                                    n_ctgs, int(first_id), int(min_ctg_len), C.byref(nb), C.byref(fo),
                                                    C.byref(na)))
        return {"n_bytes": int(nb.value), "file_offset": int(fo.value), "n_bytes_all": int(na.value)}

    def uutigs_fasta(self, min_ctg_len: int = 0) -> dict:
        """The same of the counter's uutigs, with the global ids of the ranks build (mhmkc_uutigs_fasta): the text of
        ctgs.dump_contigs("contigs-<k>.fasta", 0) (src/contigging.cpp:147-150)."""
        nb, fo, na = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(N.lib().mhmkc_uutigs_fasta(self._h, int(min_ctg_len), C.byref(nb), C.byref(fo), C.byref(na)))
        return {"n_bytes": int(nb.value), "file_offset": int(fo.value), "n_bytes_all": int(na.value)}

    def fasta_bytes(self) -> bytes:
        """The kept text, copied to the host (mhmkc_fasta_fetch)."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(N.lib().mhmkc_fasta_device(self._h, C.byref(p), C.byref(n)))
        buf = np.empty(int(n.value), dtype=np.uint8)
        self._check(N.lib().mhmkc_fasta_fetch(self._h, buf.ctypes.data))
        return buf.tobytes()

    def fasta_tensor(self):
        """A uint8 device tensor over the kept text (no copy; mhmkc_fasta_device), valid until the next fasta call, reset or
        finish."""
        import torch

        p, n = C.c_void_p(), C.c_uint64()
        self._check(N.lib().mhmkc_fasta_device(self._h, C.byref(p), C.byref(n)))
        dev = torch.device("cuda", torch.cuda.current_device())
        if not n.value:
            return torch.empty(0, dtype=torch.uint8, device=dev)

        class _Text:  # (the array interface torch.as_tensor reads a foreign device pointer through)
            __cuda_array_interface__ = {"shape": (int(n.value),), "typestr": "|u1", "data": (int(p.value), False),
                                        "version": 2}

        return torch.as_tensor(_Text(), device=dev)

    def fasta_write(self, path) -> None:
        """Write the kept text into the file at its file_offset (mhmkc_fasta_write): one rank creates and writes the file;
        several ranks (collective) write one file together, rank 0 creating it. All ranks must see the same file."""
        self._check(N.lib().mhmkc_fasta_write(self._h, os.fsencode(path)))

    def fasta_info(self) -> dict:
        """Contigs written, bytes, stage times (device events), memory and the last fasta_write (mhmkc_fasta_info)."""
        info = N.MhmkcFastaInfo()
        self._check(N.lib().mhmkc_fasta_info(self._h, C.byref(info)))
        return info.as_dict()

    # -- queries answered by the owner rank (mhmkc_lookup_ranks, mhmkc_dbjg_links_ranks)
    def lookup_ranks(self, keys, canonicalize: bool = False):
        """lookup() for k-mers that may live on any rank (mhmkc_lookup_ranks; get_kmer_target_rank + the rpc of
        src/dbjg_traversal.cpp:228-236): collective over the ranks of a finished MHMKC_OWNER_MINIMIZER counter, every rank
        with its own batch (an empty one too). Returns numpy arrays (ranks uint8, rows, counts, left, right): ranks[i] is
        the key's owner, always set; rows[i] the row of that rank's fetch() or MHMKC_NO_ROW, the rest as lookup()."""
        kk = self._query_keys(keys)
        n = kk.shape[0]
        ranks = np.empty(n, dtype=np.uint8)
        rows = np.empty(n, dtype=np.uint32)
        counts = np.empty(n, dtype=np.uint16)
        left = np.empty(n, dtype=np.uint8)
        right = np.empty(n, dtype=np.uint8)
        self._check(N.lib().mhmkc_lookup_ranks(self._h, kk.ctypes.data if n else None, n, int(bool(canonicalize)),
                                               ranks.ctypes.data, rows.ctypes.data, counts.ctypes.data, left.ctypes.data,
                                               right.ctypes.data))
        return ranks, rows, counts, left, right

    def lookup_ranks_tensors(self, keys_t, canonicalize: bool = False):
        """lookup_ranks() for keys already in HBM (mhmkc_lookup_ranks_device), following lookup_tensors: torch tensors
        (ranks uint8, rows int32 holding the uint32 bits, counts int16 holding the uint16 bits, left, right uint8). The
        call is a collective and returns with the tensors complete."""
        import torch

        if keys_t.dtype not in (torch.uint64, torch.int64):
            raise ValueError("keys_t must be a uint64 or int64 tensor")
        if not keys_t.is_contiguous() or keys_t.numel() % self.n_longs:
            raise ValueError("keys_t must be contiguous with n * n_longs words")
        n = keys_t.numel() // self.n_longs
        dev = keys_t.device
        ranks = torch.empty(n, dtype=torch.uint8, device=dev)
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int16, device=dev)
        left = torch.empty(n, dtype=torch.uint8, device=dev)
        right = torch.empty(n, dtype=torch.uint8, device=dev)
        self._after_torch(keys_t)
        self._check(N.lib().mhmkc_lookup_ranks_device(self._h, keys_t.data_ptr() if n else None, n,
                                                      int(bool(canonicalize)), ranks.data_ptr(), rows.data_ptr(),
                                                      counts.data_ptr(), left.data_ptr(), right.data_ptr()))
        return ranks, rows, counts, left, right

    def dbjg_links_ranks(self):
        """dbjg_links() with every neighbour looked up on its owner rank (mhmkc_dbjg_links_ranks; get_next_step at
        rank_n() > 1): numpy arrays next_rank uint8 [2, n_out] (MHMKC_NO_RANK: none), next_row uint32 [2, n_out] (the
        row on that rank, MHMKC_NO_ROW: none) and status [2, n_out]. The first call after a finish is a collective; the
        arrays are kept on the device, so a later call runs none."""
        n = self.n_out or 0  # (before finish the library refuses the call)
        next_rank = np.empty((2, n), dtype=np.uint8)
        next_row = np.empty((2, n), dtype=np.uint32)
        status = np.empty((2, n), dtype=np.uint8)
        self._check(N.lib().mhmkc_dbjg_links_ranks_fetch(self._h, next_rank.ctypes.data, next_row.ctypes.data,
                                                         status.ctypes.data))
        return next_rank, next_row, status

    def dbjg_links_ranks_device(self) -> dict:
        """Device pointers of the kept arrays (mhmkc_dbjg_links_ranks_device), valid until the next reset / finish."""
        pk, pr, ps = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(N.lib().mhmkc_dbjg_links_ranks_device(self._h, C.byref(pk), C.byref(pr), C.byref(ps)))
        return {"next_rank": pk.value, "next_row": pr.value, "status": ps.value, "n_out": self.n_out}

    def route_info(self) -> dict:
        """Rounds, queries and bytes between the ranks, stage times and memory of the last lookup_ranks /
        dbjg_links_ranks collective on this counter (mhmkc_route_info)."""
        info = N.MhmkcRouteInfo()
        self._check(N.lib().mhmkc_route_info(self._h, C.byref(info)))
        return info.as_dict()

    def stats(self) -> dict:
        s = N.MhmkcStats()
        self._check(N.lib().mhmkc_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def reset(self) -> None:
        self._check(N.lib().mhmkc_reset(self._h))
        self.n_out = None

    def set_profiling(self, on: "bool | int" = True) -> None:
        """Per-stage event timing (stats()["ms_kernel"]): True / 1 every stage, 2 the heavy stages only, False off."""
        self._check(N.lib().mhmkc_set_profiling(self._h, int(on) if on is not True else 1))


class TorchDistTransport:
    """mhmkc_transport (host-staged exchange, include/mhmkc.h) over a torch.distributed process group whose
    backend moves CPU tensors (gloo). It stands where the reference's UPC++ RPC stands
    (src/kcount/kmer_dht.cpp:133-149,222-231) for hosts without RCCL between the ranks: several nodes, or
    several ranks sharing one GPU."""

    def __init__(self, group=None):
        import torch.distributed as dist

        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.error: BaseException | None = None
        self._ag = N.ALLGATHER_FN(self._allgather)
        self._a2a = N.ALLTOALLV_FN(self._alltoallv)
        self.struct = N.MhmkcTransport(None, self._ag, self._a2a)

    @staticmethod
    def _view(ptr: int, n: int):
        import torch

        if n == 0:
            return torch.empty(0, dtype=torch.uint8)
        return torch.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=torch.uint8)

    def _allgather(self, _ctx, send, recv, nbytes):
        try:
            if nbytes:
                import torch

                outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(self.world)]
                self.dist.all_gather(outs, self._view(send, nbytes).clone(), group=self.group)
                dst = self._view(recv, self.world * nbytes)
                for r in range(self.world):
                    dst[r * nbytes:(r + 1) * nbytes].copy_(outs[r])
            return 0
        except BaseException as e:  # the C side turns a non-zero return into MHMKC_ETRANSPORT
            self.error = e
            return 1

    def _alltoallv(self, _ctx, send, send_bytes, recv, recv_bytes):
        try:
            sb = [int(send_bytes[p]) for p in range(self.world)]
            rb = [int(recv_bytes[p]) for p in range(self.world)]
            inp, out = self._view(send, sum(sb)), self._view(recv, sum(rb))
            self.dist.all_to_all_single(out, inp, output_split_sizes=rb, input_split_sizes=sb, group=self.group)
            return 0
        except BaseException as e:
            self.error = e
            return 1


class SharedGpuCounter:
    """Several host ranks over fewer GPU counters: the reference's launch runs one rank per core and maps rank r to
    GPU r % n_devices (gpu_utils::set_gpu_device, src/gpu-utils/gpu_utils.cpp:68-75; src/devices_gpu.cpp:61), while
    one GPU holds one counter. Rank r belongs to counter group g = r % n_counters; the group's leader (rank g) owns
    the counter (KmerCounter rank g of n_counters, MHMKC_OWNER_MINIMIZER, the leaders exchanging through the host
    transport over their own process group), the other members hand their PackedReads to it, and after the finish
    the leader sends every member the rows it owns. With n_counters dividing the number of ranks, the rows of
    counter g (get_kmer_target_rank % n_counters == g) are exactly those whose get_kmer_target_rank over all ranks
    is a member of group g (t % n_ranks = r implies t % n_counters = r % n_counters), so every rank ends with the
    table the reference's KmerDHT would hold (kmer_dht.cpp:193-196). Non-leaders never touch a GPU.

    Collective over the default torch.distributed process group (gloo: CPU tensors); every rank creates it."""

    def __init__(self, k: int, n_counters: int, *, device: int = 0, **counter_kwargs):
        import torch.distributed as dist

        self.dist = dist
        self.k, self.world, self.rank = k, dist.get_world_size(), dist.get_rank()
        if n_counters < 1 or self.world % n_counters:
            raise ValueError("n_counters must divide the number of ranks")
        self.n_counters = n_counters
        self.group_id = self.rank % n_counters
        self.leader = self.group_id
        self.members = list(range(self.group_id, self.world, n_counters))
        # every rank takes part in creating every group (torch.distributed.new_group is collective)
        leaders = dist.new_group(list(range(n_counters)))
        self.counter = None
        if self.rank == self.leader:
            self.counter = KmerCounter(k, device=device, rank=self.group_id, n_ranks=n_counters,
                                       transport=TorchDistTransport(leaders) if n_counters > 1 else None,
                                       output_owner=N.MHMKC_OWNER_MINIMIZER, **counter_kwargs)
        self._reads = []

    def add_packed_reads(self, packed_bytes: np.ndarray, offsets: np.ndarray) -> None:
        self._reads.append((np.ascontiguousarray(packed_bytes, dtype=np.uint8),
                            np.ascontiguousarray(offsets, dtype=np.uint64)))

    def _send_arrays(self, arrays, dst: int) -> None:
        import torch

        sizes = torch.tensor([a.nbytes for a in arrays], dtype=torch.int64)
        self.dist.send(torch.tensor([len(arrays)], dtype=torch.int64), dst)
        self.dist.send(sizes, dst)
        for a in arrays:
            if a.nbytes:
                self.dist.send(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()), dst)

    def _recv_arrays(self, src: int) -> list:
        import torch

        n = torch.zeros(1, dtype=torch.int64)
        self.dist.recv(n, src)
        sizes = torch.zeros(int(n.item()), dtype=torch.int64)
        self.dist.recv(sizes, src)
        out = []
        for sz in sizes.tolist():
            t = torch.empty(sz, dtype=torch.uint8)
            if sz:
                self.dist.recv(t, src)
            out.append(t.numpy())
        return out

    def finish(self) -> KmerTable:
        """Count every member's reads on the group's GPU, exchange between the counters, and return this rank's
        rows (the k-mers whose get_kmer_target_rank over all ranks is this rank)."""
        if self.rank != self.leader:  # members: reads to the leader, then this rank's rows back
            flat = [a for pair in self._reads for a in pair]
            self._send_arrays(flat, self.leader)
            width, keys, counts, left, right = self._recv_arrays(self.leader)
            nl = int(width.view(np.int64)[0])  # the leader's key width (its counter's n_longs)
            return KmerTable(self.k, keys.view(np.uint64).reshape(-1, nl), counts.view(np.uint16), left, right)
        c = self.counter
        for b, o in self._reads:
            c.add_packed_reads(b, o)
        for m in self.members[1:]:
            got = self._recv_arrays(m)
            for i in range(0, len(got), 2):
                c.add_packed_reads(got[i], got[i + 1].view(np.uint64))
        c.finish()
        t = c.fetch()
        owner = c.target_ranks(t.keys, self.world) if len(t) else np.zeros(0, np.int64)
        mine = None
        for m in self.members:
            sel = np.flatnonzero(owner == m)
            part = [np.ascontiguousarray(t.keys[sel]), np.ascontiguousarray(t.counts[sel]),
                    np.ascontiguousarray(t.left[sel]), np.ascontiguousarray(t.right[sel])]
            if m == self.rank:
                mine = KmerTable(self.k, *part)
            else:
                self._send_arrays([np.array([c.n_longs], dtype=np.int64)] + part, m)
        return mine

    def close(self) -> None:
        if self.counter is not None:
            self.counter.close()
            self.counter = None



def _ostream_double(x: float) -> str:
    """A double as `ostream << x` prints it with the default precision: "%g" with six significant digits."""
    return "%g" % x


def perc_str(num: int, tot: int) -> str:
    """upcxx_utils perc_str (upcxx-utils/src/log.cpp:428-434): "num (p%)" with p = 100 num / tot in fixed notation,
    two decimals; 0.00 when tot is 0."""
    return "%d (%.2f%%)" % (num, 0.0 if tot == 0 else 100.0 * num / tot)


def assembly_stats_text(stats: dict, min_ctg_len: int) -> str:
    """The block Contigs::print_stats logs (src/contigs.cpp:151-163), line for line, from a stats dict (uutigs_stats()
    ["all"]): no colour codes; doubles as `ostream <<` prints them; a division by zero prints as the stream prints the
    result (nan, -nan for 0.0 / 0 as glibc does, or inf)."""
    def div(a: float, b: float) -> str:
        if b == 0:
            return "-nan" if a == 0 else ("inf" if a > 0 else "-inf")
        return _ostream_double(a / b)

    n, tot = int(stats["n_ctgs"]), int(stats["tot_len"])
    out = ["Assembly statistics (contig lengths >= %d)" % min_ctg_len,
           "    Number of contigs:       %d" % n,
           "    Total assembled length:  %d" % tot,
           "    Average contig depth:    %s" % div(float(stats["tot_depth"]), n),
           "    Number of Ns/100kbp:     %s (%d)" % (div(float(stats["n_ns"]) * 100000.0, tot), int(stats["n_ns"])),
           "    Max. contig length:      %d" % int(stats["max_len"]),
           "    Contig lengths:"]
    for kbp, s in zip((1, 5, 10, 25, 50), stats["len_sums"]):
        out.append("        > " + ("%dkbp:" % kbp).ljust(19) + perc_str(int(s), tot))
    return "\n".join(out) + "\n"


def comm_id() -> bytes:
    """RCCL unique id for multi-rank counters (rank 0 creates it and broadcasts it)."""
    buf = C.create_string_buffer(N.MHMKC_COMM_ID_BYTES)
    N.check(N.lib().mhmkc_comm_id(buf))
    return buf.raw


# ------------------------------------------------------------------------------------------------
# KmerDHT / analyze_kmers mirror


def map_hash(longs) -> int:
    """mhmkc_map_hash (include/mhmkc.h): the C++ adapter's KmerMap hash of a key's words."""
    M = (1 << 64) - 1
    h = 0x9E3779B97F4A7C15
    for w in longs:
        h = ((h ^ int(w)) * 0xBF58476D1CE4E5B9) & M
        h ^= h >> 31
    h = (h * 0x94D049BB133111EB) & M
    return h ^ (h >> 29)


def _quick_hash(v: int) -> int:
    """quick_hash (src/hash_funcs.c:332-342)."""
    M = (1 << 64) - 1
    v = (v * 3935559000370003845 + 2691343689449507681) & M
    v ^= v >> 21
    v = (v ^ (v << 37)) & M
    v ^= v >> 4
    v = (v * 4768777513237032717) & M
    v = (v ^ (v << 20)) & M
    v ^= v >> 41
    v = (v ^ (v << 5)) & M
    return v


def _revcomp_longs(longs: Sequence[int], k: int) -> tuple:
    s = kmer_to_string(longs, k)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    return kmer_from_string("".join(comp[c] for c in reversed(s)), len(longs))


def minimizer_len(k: int) -> int:
    """KmerDHT minimizer length (src/kcount/kmer_dht.cpp:114-116)."""
    return min(27, max(15, k * 2 // 3 + 1))


def get_minimizer_fast(longs: Sequence[int], k: int, m: int) -> int:
    """Greatest least-complement m-mer (Kmer::get_minimizer_fast, src/kmer.cpp:344-403)."""
    M = (1 << 64) - 1
    mask = (M << (64 - 2 * m)) & M
    s = kmer_to_string(longs, k)
    rc = kmer_to_string(_revcomp_longs(longs, k), k)
    best = 0
    for i in range(k - m + 1):
        f = kmer_from_string(s[i:i + m], 1)[0] & mask
        r = kmer_from_string(rc[k - m - i:k - i], 1)[0] & mask
        best = max(best, min(f, r))
    return best


def get_kmer_target_rank(longs: Sequence[int], k: int, rank_n: int) -> int:
    """KmerDHT::get_kmer_target_rank (src/kcount/kmer_dht.cpp:193-196): the owner rank dbjg expects."""
    return _quick_hash(get_minimizer_fast(longs, k, minimizer_len(k))) % rank_n


class KmerDHT:
    """Per-rank result holder shaped like KmerDHT<MAX_K> (src/kcount/kmer_dht.hpp:118-172)."""

    def __init__(self, k: int, my_num_kmers: int = 0, *, counter: KmerCounter | None = None, rank: int = 0,
                 n_ranks: int = 1, **counter_kwargs):
        self.k = k
        self.my_num_kmers = my_num_kmers
        self.rank, self.n_ranks = rank, n_ranks
        self.counter = counter or KmerCounter(k, rank=rank, n_ranks=n_ranks, **counter_kwargs)
        self.minimizer_len = minimizer_len(k)
        self.table: KmerTable | None = None
        self._map: dict | None = None

    def get_minimizer_len(self) -> int:
        return self.minimizer_len

    def finish_updates(self) -> None:
        """flush_updates + finish_updates (src/kcount/kmer_dht.cpp:227-236)."""
        self.counter.finish()
        self.table = self.counter.fetch()
        self._map = None

    @property
    def local_kmers(self) -> dict:
        """KmerMap: {longs tuple: KmerCounts} (materialised lazily; use .table for large sets)."""
        if self._map is None:
            t = self.table
            self._map = {tuple(int(x) for x in t.keys[i]): KmerCounts(int(t.counts[i]), chr(int(t.left[i])),
                                                                       chr(int(t.right[i])))
                         for i in range(len(t))}
        return self._map

    def get_local_num_kmers(self) -> int:
        return 0 if self.table is None else len(self.table)

    def get_num_kmers(self) -> int:
        return self.get_local_num_kmers()

    def get_local_kmer_counts(self, kmer) -> KmerCounts | None:
        """get_local_kmer_counts (src/kcount/kmer_dht.cpp:198-204): the k-mer as given, no canonicalisation. With a
        finished counter attached it is one lookup on the GPU (KmerCounter.lookup); only a table without a live counter
        (closed, or reset since) goes through the local_kmers dict."""
        key = kmer_from_string(kmer) if isinstance(kmer, str) else tuple(int(x) for x in kmer)
        if self._counter_has_table() and len(key) == self.counter.n_longs:
            rows, counts, left, right = self.counter.lookup(np.array([key], dtype=np.uint64))
            if int(rows[0]) == N.MHMKC_NO_ROW:
                return None
            return KmerCounts(int(counts[0]), chr(int(left[0])), chr(int(right[0])))
        return self.local_kmers.get(key)

    def _counter_has_table(self) -> bool:
        c = self.counter
        return c is not None and getattr(c, "_h", None) is not None and c.n_out is not None and self.table is not None

    def kmer_exists(self, kmer) -> bool:
        """kmer_exists (src/kcount/kmer_dht.cpp:206-219) for this rank's k-mers: the k-mer is canonicalised, then
        looked up (KmerCounter.lookup with canonicalize=True)."""
        key = kmer_from_string(kmer, self.counter.n_longs) if isinstance(kmer, str) else tuple(int(x) for x in kmer)
        rows = self.counter.lookup(np.array([key], dtype=np.uint64), canonicalize=True)[0]
        return int(rows[0]) != N.MHMKC_NO_ROW

    def get_kmer_target_rank(self, kmer) -> int:
        longs = kmer_from_string(kmer) if isinstance(kmer, str) else kmer
        return get_kmer_target_rank(longs, self.k, self.n_ranks)

    def dump_kmers(self, out_dir: str | os.PathLike = ".") -> Path:
        """dump_kmers (src/kcount/kmer_dht.cpp:243-266): kmers-<k>.txt.gz in this rank's directory
        (get_rank_path: per_rank/<rank / 1000>/<rank>/, upcxx-utils/src/log.cpp:283-312), lines
        "KMER count L R"."""
        path = Path(out_dir) / "per_rank" / f"{self.rank // 1000:08d}" / f"{self.rank:08d}" / f"kmers-{self.k}.txt.gz"
        path.parent.mkdir(parents=True, exist_ok=True)
        with gzip.open(path, "wt") as f:
            for line in self.table.lines():
                f.write(line + "\n")
        return path

    def clear_stores(self) -> None:
        self.counter.reset()


def analyze_kmers(kmer_len: int, prev_kmer_len: int, qual_offset: int, packed_reads_list: Sequence[PackedReads],
                  dmin_thres: int, ctgs: Sequence, kmer_dht: KmerDHT, dump_kmers: bool = False,
                  dump_dir: str | os.PathLike = ".") -> None:
    """analyze_kmers<MAX_K> (src/kcount/kcount.hpp:71-73, src/kcount/kcount.cpp:140-157).

    Counts every read of every PackedReads on this rank's GPU, exchanges by hash range with the other
    ranks, applies the contig pass when ctgs is not empty (add_ctg_kmers, kcount.cpp:100-138; single rank),
    purges and chooses extensions; the result is kmer_dht.table / kmer_dht.local_kmers. ctgs: objects with
    .seq and .depth (a float, as Contig), or (seq, depth) pairs.
    """
    if kmer_len != kmer_dht.k:
        raise ValueError("kmer_len differs from the KmerDHT's k")
    kmer_dht.counter.set_dmin_thres(dmin_thres)  # _dmin_thres = dmin_thres (kcount.cpp:145)
    for pr in packed_reads_list:
        if pr.qual_offset != qual_offset:
            raise ValueError("PackedReads qual_offset differs")
        kmer_dht.counter.add_reads(pr)
    if len(ctgs):
        seqs, depths = [], []
        for c in ctgs:
            seq, depth = (c.seq, c.depth) if hasattr(c, "seq") else (c[0], c[1])
            seqs.append(seq)
            depths.append(min(int(depth), 65535))  # Contig::get_uint16_t_depth (src/contigs.hpp:65)
        kmer_dht.counter.add_ctgs(seqs, depths)
    kmer_dht.finish_updates()
    if dump_kmers:
        kmer_dht.dump_kmers(dump_dir)


# ------------------------------------------------------------------------------------------------
# synthetic reads


def synth_genome(genome_len: int, seed: int) -> np.ndarray:
    S = N.synth()
    cfg = N.SynthConfig()
    S.mhmkc_synth_config_init(C.byref(cfg), genome_len, 150, seed)
    g = np.empty(genome_len, dtype=np.uint8)
    if S.mhmkc_synth_genome(C.byref(cfg), g.ctypes.data) != 0:
        raise RuntimeError("mhmkc_synth_genome failed")
    return g


def synth_reads(genome: np.ndarray, n_reads: int, read_len: int, seed: int, first_read: int = 0,
                threads: int = 0, **rates) -> tuple[np.ndarray, np.ndarray]:
    """(packed_bytes, offsets) of reads first_read .. first_read + n_reads - 1 of the global set."""
    S = N.synth()
    cfg = N.SynthConfig()
    S.mhmkc_synth_config_init(C.byref(cfg), genome.size, read_len, seed)
    for key, val in rates.items():
        setattr(cfg, key, val)
    b = np.empty(n_reads * read_len, dtype=np.uint8)
    o = np.empty(n_reads + 1, dtype=np.uint64)
    g = np.ascontiguousarray(genome, dtype=np.uint8)
    nt = threads or min(16, os.cpu_count() or 1)
    if S.mhmkc_synth_reads(C.byref(cfg), g.ctypes.data, first_read, n_reads, b.ctypes.data, o.ctypes.data, nt) != 0:
        raise RuntimeError("mhmkc_synth_reads failed")
    return b, o
