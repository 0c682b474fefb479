"""Pinning the CPU oracle (runs without a GPU).

The checking chain is: reference build -> oracle and literal restatement -> golden fixtures -> GPU. Its top, the
reference's own kcount sources compiled single-rank (oracle/_ref/libkcountref.so), is compared with the oracle in
tests/test_reference_build.py; the golden tables are that build's output (tests/golden/make_golden.py). Still
unpinned by reference code: the multi-rank exchange over real UPC++, FASTQ ingest, merge_reads, and k < 15 or
k % 32 == 0, where the reference is undefined or wrong. This file holds the links below the top:

  1. MurmurHash3 / quick_hash == the reference's own src/hash_funcs.c compiled unmodified (oracle/_ref);
  2. SURVEY.md Appendix A known answers (Kmer layout, hash, minimizer, minimizer hash);
  3. the invariants of the reference's test/kmer-test.cpp (round trip, revcomp, hash, minimizers);
  4. the C oracle == a literal string-level restatement of the reference code (tests/ref_literal.py);
  5. the oracle reproduces every committed golden fixture;
  6. the record path (extract + count) == the read path (used by the multi-rank protocol tests).
"""
from __future__ import annotations

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
import ref_literal as R
from common import (GOLDEN, assert_tables_equal, ctg_set, edge_case_set, golden_input, oracle_ctg_table, oracle_table,
                    read_reads_file, read_table_file, synth_set)

# test/kmer-test.cpp:11-33 (data vectors of the reference's own unit test)
RANDOM_READ = ("CGCTGTTCCAGATGACGAACCAGGAATTCCGCCAGGTATTCGACTTTATTCGCGAAGTCAAGAAGTTGAACGTCATCAGTGTGAACTACGGTTGCGAAGG"
               "CTTCCTCGGCAGCTACGAGAAGGATGCACGCATCTGCCCGTTCTTCTGCCGTGCCGGCGTGAACGTGTCCTCGGTGCTTTGCGATGGCAGCATTTCGGCA"
               "TGCCCGAGCT")
REPEATS = ["A" * 166, "C" * 166, "G" * 166, "T" * 166, ("ACGT" * 42)[:166], ("TCGA" * 42)[:166], ("CAGT" * 42)[:166]]


# ---- 1. reference hash_funcs.c ------------------------------------------------------------------

def test_murmur_and_quick_hash_vs_reference_source():
    ref = O.hashref()
    if ref is None:
        pytest.skip("oracle/_ref/libhashref.so not built (reference tree absent)")
    rng = np.random.default_rng(0)
    L = O.oracle()
    for length in list(range(0, 65)) + [96, 127, 128, 255]:
        for _ in range(20):
            buf = rng.integers(0, 256, size=max(length, 1), dtype=np.uint8)
            assert L.orc_murmur3_x64_64(buf.ctypes.data, length) == ref.MurmurHash3_x64_64(buf.ctypes.data, length)
            a = np.zeros(2, np.uint64)
            b = np.zeros(2, np.uint64)
            seed = int(rng.integers(0, 2**32))
            L.orc_murmur3_x64_128(buf.ctypes.data, length, seed, a.ctypes.data)
            ref.MurmurHash3_x64_128(buf.ctypes.data, length, seed, b.ctypes.data)
            assert (a == b).all()
    for v in list(rng.integers(0, 2**63, size=2000, dtype=np.uint64)) + [0, 1, 2**64 - 1]:
        assert L.orc_quick_hash(int(v)) == ref.quick_hash(int(v))


# ---- 2. Appendix A known answers ----------------------------------------------------------------

def test_appendix_a_scalars():
    z = np.zeros(1, np.uint64)
    assert O.oracle().orc_murmur3_x64_64(z.ctypes.data, 8) == 0x864BA144DF098483
    assert O.oracle().orc_quick_hash(0) == 0x7B439D0C1FD00DE3
    assert O.oracle().orc_quick_hash(1) == 0xBEA952A971BA8E83


APPENDIX_A = [
    # (kmer, n_longs, longs, hash, get_minimizer_fast(m, true), minimizer_hash_fast(m))
    ("ACGTACGTACGTACGTACGTA", 1, [0x1B1B1B1B1B000000], 0xA47F0F8106BE6783, 0xB1B1B1B000000000, 0x7B9CF376CDBE4A50),
    ("CGCTGTTCCAGATGACGAACC", 1, [0x67BD48E181400000], 0xD3C6722CA54C5474, 0xDB4DE81000000000, 0xFBEED8639C5AE34F),
    (RANDOM_READ[:63], 2, [0x67BD48E1814A0F59, 0x4ACF61FCF660B420], 0x470509568A42D5B5, 0xCF61FCF660B42000,
     0xAA95C0BEB14E494F),
    (RANDOM_READ[:33], 2, [0x67BD48E1814A0F59, 0x4000000000000000], 0x44C66528D74660B1, 0xEF52386052800000,
     0x2E3C051BDE79A656),
    (RANDOM_READ[:99], 4, [0x67BD48E1814A0F59, 0x4ACF61FCF660B420, 0xBE06D34BB81C6BE6, 0x0800000000000000],
     0xF9FAD81E4B9F8AF0, 0xE1BD07DF87D98000, 0x40E1DEA4B0AA5EFD),
]


@pytest.mark.parametrize("kmer,nl,longs,h,mini,mhash", APPENDIX_A)
def test_appendix_a_kmers(kmer, nl, longs, h, mini, mhash):
    k = len(kmer)
    mlen = O.oracle().orc_minimizer_len(k)
    la = O.kmer_from_string(kmer, nl)
    assert [int(x) for x in la] == longs
    assert O.kmer_hash(la) == h
    assert O.minimizer_fast(la, k, mlen) == mini
    assert O.minimizer_hash_fast(la, k, mlen) == mhash
    # the package's host mirror agrees on layout and minimizer hash
    assert list(m.kmer_from_string(kmer, nl)) == longs
    assert m.kcount._quick_hash(m.kcount.get_minimizer_fast(longs, k, mlen)) == mhash


# ---- 3. test/kmer-test.cpp invariants ----------------------------------------------------------

def slow_revcomp(s: str) -> str:  # test/kmer-test.cpp:35-49
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))


@pytest.mark.parametrize("max_k", [32, 64])
def test_kmer_test_invariants(max_k):
    nl = max_k // 32
    for k in range(1, max_k):  # the reference test runs k = 1..MAX_K-1 for MAX_K 32 and 64 (:351-373)
        for seq in REPEATS + [RANDOM_READ]:
            seen = {}
            for i in range(len(seq) - k + 1):
                sub = seq[i:i + k]
                la = O.kmer_from_string(sub, nl)
                assert O.kmer_to_string(la, k) == sub  # :45-68
                rc = O.kmer_revcomp(la, k)
                assert O.kmer_to_string(rc, k) == slow_revcomp(sub)  # :70-170
                assert (O.kmer_revcomp(rc, k) == la).all()
                h = O.kmer_hash(la)
                if sub in seen:
                    assert seen[sub] == h
                else:
                    assert h not in seen.values()  # :172-245 (distinct k-mers, distinct hashes here)
                    seen[sub] = h
                if k >= 15:  # :247-313 symmetric least-complement minimizer
                    mm = 15
                    assert O.minimizer_fast(la, k, mm) == O.minimizer_fast(rc, k, mm)


# ---- 4. literal restatement ---------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 33, 63, 77])
def test_oracle_matches_literal_restatement(k):
    b, o = synth_set(250, 4000, 300 + k)
    lit = R.analyze_kmers([b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)], k)
    t = oracle_table(b, o, k)
    orc = {tuple(int(x) for x in t.keys[i]): (int(t.counts[i]), chr(t.left[i]), chr(t.right[i])) for i in range(len(t))}
    assert orc == lit


def test_oracle_matches_literal_edge_cases():
    b, o = edge_case_set(seed=8, n=300)
    for k in (21, 31):
        lit = R.analyze_kmers([b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)], k)
        t = oracle_table(b, o, k)
        orc = {tuple(int(x) for x in t.keys[i]): (int(t.counts[i]), chr(t.left[i]), chr(t.right[i]))
               for i in range(len(t))}
        assert orc == lit


@pytest.mark.parametrize("dmin,qcut", [(1, 20), (3, 0), (2, 31)])
def test_oracle_matches_literal_parameters(dmin, qcut):
    b, o = synth_set(200, 3000, 17)
    lit = R.analyze_kmers([b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)], 21, dmin_thres=dmin,
                          qual_cutoff=qcut)
    t = oracle_table(b, o, 21, dmin_thres=dmin, qual_cutoff=qcut)
    orc = {tuple(int(x) for x in t.keys[i]): (int(t.counts[i]), chr(t.left[i]), chr(t.right[i])) for i in range(len(t))}
    assert orc == lit


@pytest.mark.parametrize("k,dmin", [(21, 2), (21, 1), (21, 3), (33, 2), (63, 4)])
def test_oracle_contig_pass_matches_literal(k, dmin):
    """The contig pass (add_ctg_kmers -> insert_supermer_from_ctg, order-dependent) in the C oracle equals
    the literal restatement."""
    b, o, seqs, depths = ctg_set(seed=40 + k + dmin)
    lit = R.analyze_kmers([b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)], k, dmin_thres=dmin,
                          ctgs=list(zip(seqs, [int(d) for d in depths])))
    t = oracle_ctg_table(b, o, seqs, depths, k, dmin_thres=dmin)
    orc = {tuple(int(x) for x in t.keys[i]): (int(t.counts[i]), chr(t.left[i]), chr(t.right[i])) for i in range(len(t))}
    assert orc == lit
    plain = oracle_table(b, o, k, dmin_thres=dmin)
    assert len(t) != len(plain) or (t.sorted().counts != plain.sorted().counts).any(), "contigs changed nothing"


def test_dynamic_threshold_quirk():
    """(int)((1.0 - 0.9) * count) is one less than count/10 for multiples of 10."""
    assert int((1.0 - 0.9) * 10) == 0
    assert sum(1 for c in range(1, 65536) if c % 10 == 0 and int((1.0 - 0.9) * c) == c // 10 - 1) == 6553


# ---- 5. golden fixtures -------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(p.name for p in GOLDEN.glob("table_*.tsv.gz")))
def test_oracle_reproduces_golden(name):
    _, setname, kk = name[:-len(".tsv.gz")].split("_")
    k = int(kk[1:])
    b, o, seqs, depths = golden_input(setname)
    got = oracle_ctg_table(b, o, seqs, depths, k) if seqs else oracle_table(b, o, k)
    assert_tables_equal(got, read_table_file(GOLDEN / name, k), name)


def test_golden_s100_literal_k21():
    b, o = read_reads_file(GOLDEN / "reads_s100.txt.gz")
    lit = R.analyze_kmers([b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)], 21)
    t = read_table_file(GOLDEN / "table_s100_k21.tsv.gz", 21)
    got = {tuple(int(x) for x in t.keys[i]): (int(t.counts[i]), chr(t.left[i]), chr(t.right[i])) for i in range(len(t))}
    assert got == lit


# ---- 6. record path -----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 63])
def test_record_path_equals_read_path(k):
    b, o = edge_case_set(seed=12, n=600)
    keys, exts = O.extract(b, o, k)
    a = O.count_records(keys, exts, k)
    ka, ca, la, ra = a.fetch()
    assert_tables_equal(m.KmerTable(k, ka, ca, la, ra), oracle_table(b, o, k), "records vs reads")


# ---- the multi-threaded restatement (oracle/kcount_mt.c) ---------------------------------------------


@pytest.mark.parametrize("k,threads", [(21, 1), (21, 8), (33, 3), (63, 8), (99, 5), (15, 2), (127, 4)])
def test_mt_restatement_equals_oracle(k, threads):
    from common import assert_tables_equal, oracle_table, synth_set

    b, o = synth_set(3000, 15000, 300 + k)
    t = O.kcount_mt(b, o, k, threads=threads)
    keys, c, l, r = t.fetch()
    assert_tables_equal(m.KmerTable(k, keys, c, l, r), oracle_table(b, o, k), f"mt k={k} threads={threads}")
    ref = O.kcount(b, o, k).stats()
    st = t.stats()
    assert (st["occurrences"], st["distinct"], st["purged"]) == (ref["occurrences"], ref["distinct"], ref["purged"])


@pytest.mark.parametrize("k", [21, 63])
def test_mt_restatement_edge_and_hot(k):
    from common import assert_tables_equal, edge_case_set, hot_set, oracle_table

    for b, o in (edge_case_set(), hot_set()):
        t = O.kcount_mt(b, o, k, threads=4)
        keys, c, l, r = t.fetch()
        assert_tables_equal(m.KmerTable(k, keys, c, l, r), oracle_table(b, o, k), f"mt edge/hot k={k}")


@pytest.mark.parametrize("cutoff,dmin,dyn", [(0, 2, 0.9), (25, 3, 0.75), (20, 0, 0.0), (32, 5, 1.0)])
def test_mt_restatement_parameters(cutoff, dmin, dyn):
    from common import assert_tables_equal, oracle_table, synth_set

    b, o = synth_set(1500, 8000, 7)
    t = O.kcount_mt(b, o, 21, qual_cutoff=cutoff, dmin_thres=dmin, dyn_min_depth=dyn, threads=4)
    keys, c, l, r = t.fetch()
    assert_tables_equal(m.KmerTable(21, keys, c, l, r),
                        oracle_table(b, o, 21, qual_cutoff=cutoff, dmin_thres=dmin, dyn_min_depth=dyn), "mt params")


@pytest.mark.parametrize("name", sorted(p.name for p in GOLDEN.glob("table_*.tsv.gz")))
def test_mt_restatement_reproduces_golden(name):
    from common import GOLDEN, assert_tables_equal, golden_input, read_table_file

    _, setname, kk = name[:-len(".tsv.gz")].split("_")
    k = int(kk[1:])
    b, o, seqs, depths = golden_input(setname)
    if seqs:
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in seqs], out=offs[1:])
        t = O.kcount_mt_ctgs(b, o, "".join(seqs).encode(), offs, depths, k, threads=4)
    else:
        t = O.kcount_mt(b, o, k, threads=4)
    keys, c, l, r = t.fetch()
    assert_tables_equal(m.KmerTable(k, keys, c, l, r), read_table_file(GOLDEN / name, k), name)


@pytest.mark.parametrize("k,parts", [(21, 8), (63, 5), (99, 3)])
def test_mt_range_parts_union_is_the_table(k, parts):
    """kcount_mt built one key range at a time (the C3/C4 8-rank check builds a 1e8-read table that way): the parts
    are disjoint, every row is in the part mt_ranges names, and their union is the whole table; row fingerprints of
    equal tables are equal multisets and a changed row changes its fingerprint."""
    b, o = synth_set(3000, 20000, 700 + k)
    whole = O.kcount_mt(b, o, k, threads=4).fetch()
    fw = np.sort(O.row_fingerprints(*whole, k))
    got = []
    for p in range(parts):
        t = O.kcount_mt_range(b, o, k, p, parts, threads=4).fetch()
        assert (O.mt_ranges(t[0], k, parts) == p).all()
        got.append(O.row_fingerprints(*t, k))
    assert np.array_equal(np.sort(np.concatenate(got)), fw)
    keys, c, lft, rgt = whole
    assert (O.mt_ranges(keys, k, parts) < parts).all()
    c2 = c.copy()
    c2[0] ^= 1
    assert not np.array_equal(np.sort(O.row_fingerprints(keys, c2, lft, rgt, k)), fw)


@pytest.mark.parametrize("k,dmin", [(21, 2), (33, 2), (63, 3), (99, 2), (21, 1)])
def test_mt_contig_pass_equals_oracle(k, dmin):
    """kcount_mt's contig pass (the C5-shaped multi-k check's reference, tests/test_c5_scale.py) == the single-threaded
    restatement (orc_kcount_ctgs, itself pinned to tests/ref_literal.py above) on common.ctg_set: duplicates at other
    depths (min rule), mutated copies (disagreeing contigs purged, read k-mers replaced), novel keys, N bases,
    lowercase, contigs shorter than k + 2, depths 0 to 65535; whole, and built in 3 key-range parts."""
    for seed in (31, 32):
        b, o, seqs, depths = ctg_set(seed=seed + k, n_reads=400)
        exp = np.sort(O.row_fingerprints(*O.kcount_ctgs(b, o, seqs, depths, k, dmin_thres=dmin).fetch(), k))
        blob = "".join(seqs).encode("ascii")
        co = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=co[1:])
        got = O.kcount_mt_ctgs(b, o, blob, co, depths, k, threads=3, dmin_thres=dmin).fetch()
        assert np.array_equal(np.sort(O.row_fingerprints(*got, k)), exp)
        parts = [O.row_fingerprints(*O.kcount_mt_ctgs(b, o, blob, co, depths, k, threads=2, part=p, n_parts=3,
                                                      dmin_thres=dmin).fetch(), k) for p in range(3)]
        assert np.array_equal(np.sort(np.concatenate(parts)), exp)


@pytest.mark.parametrize("k,world", [(21, 8), (63, 8), (77, 3)])
def test_batch_target_ranks(k, world):
    b, o = synth_set(400, 5000, 720 + k)
    keys = O.kcount(b, o, k).fetch()[0]
    L = O.oracle()
    exp = [L.orc_kmer_target_rank(np.ascontiguousarray(keys[i]).ctypes.data, k, keys.shape[1], world)
           for i in range(len(keys))]
    assert O.target_ranks(keys, k, world).tolist() == exp
