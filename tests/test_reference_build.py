"""The top of the checking chain: the reference's own CPU kcount code, built single-rank (runs without a GPU).

oracle/_ref/libkcountref.so is the reference's unmodified kmer.cpp, kcount.cpp, kcount_cpu.cpp, kmer_dht.cpp,
packed_reads.cpp, contigs.cpp, utils.cpp and hash_funcs.c compiled against the one-rank stand-in headers of
oracle/ref_standin (oracle/Makefile `ref`, oracle/ref_driver.cpp). Here the C oracle, and with it everything the
oracle is the reference for, is compared with that build:

  1. the Kmer layer (layout, round trip, revcomp, operator<, hash, minimizer, minimizer hash, target rank) for every
     k in 1..127, the package's host mirrors included, and SURVEY.md Appendix A recomputed by the reference;
  2. whole tables, reference analyze_kmers == O.kcount / O.kcount_ctgs row for row, on the inputs of the GPU parity
     tests, with zero warnings and zero dropped inserts on the reference's side.

Kmer::get_minimizer_fast asserts m <= k (src/kmer.cpp:346) and KmerDHT's minimizer length is at least 15
(src/kcount/kmer_dht.cpp:114-116), so the reference defines no minimizer, no target rank and, because process_seq asks
for the target rank of every k-mer (src/kcount/kcount_cpu.cpp:85-88), no table for k < 15: its Release build has no
asserts and walks off the key there. Those k are compared up to the hash only; what the package computes for them
(the minimizer of no candidates, 0) is the project's own definition.

The tests skip when oracle/_ref was not built (the reference tree is absent).
"""
from __future__ import annotations

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
from common import (assert_tables_equal, ctg_set, edge_case_set, hot_set, long_ragged_set, oracle_ctg_table,
                    oracle_table, ref_table, synth_set)
from test_oracle import APPENDIX_A, RANDOM_READ, REPEATS

pytestmark = pytest.mark.skipif(O.kcountref() is None or O.kcountref("q25d75") is None,
                                reason="oracle/_ref/libkcountref.so not built (reference tree absent)")

WORLDS = (1, 2, 3, 8, 9)
MIN_MINIMIZER_K = 15  # the smallest k at which the reference's KmerDHT minimizer (m >= 15) is defined


def check_kmer_layer(rk: O.RefKmer, subs: list, mirror_every: int = 1):
    """Oracle == reference on every k-mer string of subs (all of length rk.k); the package's pure-Python mirrors on
    every mirror_every-th."""
    k, nl = rk.k, rk.nl
    mlen = O.oracle().orc_minimizer_len(k)
    assert mlen == m.kcount.minimizer_len(k)
    keys = []
    for i, sub in enumerate(subs):
        la = O.kmer_from_string(sub, nl)
        ref_la = rk.from_string(sub)
        assert (la == ref_la).all(), (k, sub)  # layout
        assert list(m.kmer_from_string(sub, nl)) == [int(x) for x in ref_la]
        assert rk.to_string(la) == sub == O.kmer_to_string(la, k)  # round trip
        rc = rk.revcomp(la)
        assert (O.kmer_revcomp(la, k) == rc).all(), (k, sub)
        for a, b in ((la, rc), (rc, la), (la, la)):  # operator<: the words in order, unsigned
            assert rk.less(a, b) == (tuple(int(x) for x in a) < tuple(int(x) for x in b))
        assert O.kmer_hash(la) == rk.hash(la), (k, sub)
        if k >= MIN_MINIMIZER_K:
            mini = rk.minimizer_fast(la, mlen)
            assert O.minimizer_fast(la, k, mlen) == mini, (k, sub)
            assert O.minimizer_fast(la, k, mlen, False) == rk.minimizer_fast(la, mlen, False)
            mhash = rk.minimizer_hash_fast(la, mlen)
            assert O.minimizer_hash_fast(la, k, mlen) == mhash, (k, sub)
            if i % mirror_every == 0:
                assert m.kcount.get_minimizer_fast(la, k, mlen) == mini
                assert m.kcount._quick_hash(mini) == mhash
        keys.append(la)
    if k >= MIN_MINIMIZER_K and keys:
        kk = np.array(keys, dtype=np.uint64)
        for world in WORLDS:
            ranks, ref_mlen = rk.target_ranks(kk, world)
            assert ref_mlen == mlen
            assert (O.target_ranks(kk, k, world) == ranks).all(), (k, world)
            assert (ranks >= 0).all() and (ranks < world).all()
            for i in range(0, len(keys), mirror_every):
                assert m.kcount.get_kmer_target_rank(keys[i], k, world) == ranks[i]


@pytest.mark.parametrize("max_k", [32, 64, 96, 128])
def test_kmer_layer_vs_reference(max_k):
    """Every k of this MAX_K over the data vectors of the reference's own unit test (test/kmer-test.cpp:11-33)."""
    for k in range(max(1, max_k - 32), max_k):
        rk = O.RefKmer(k)
        assert rk.nl == max_k // 32
        subs = []
        for seq in REPEATS + [RANDOM_READ]:
            windows = [seq[i:i + k] for i in range(len(seq) - k + 1)]
            got = rk.get_kmers(seq)  # Kmer::get_kmers: one k-mer per window, in order
            assert got.shape[0] == len(windows)
            exp = np.array([O.kmer_from_string(w, rk.nl) for w in windows], dtype=np.uint64)
            if k % 32 == 0:
                # The reference's get_kmers masks the last word with endmask, which is all ones when k % 32 == 0
                # (src/kmer.cpp:225-232), while n_longs = k / 32 + 1 there: the key's last word keeps the next 32
                # bases of the sequence, so Kmer(s) != get_kmers' k-mer and the reference's tables at k = 32, 64, 96
                # are not k-mer tables. The project zeroes that word; no parity case uses these k.
                for i in range(len(windows)):
                    nxt = seq[i + k:i + k + 32]
                    exp[i, -1] = O.kmer_from_string(nxt, 1)[0] if nxt else 0
            assert (got == exp).all(), (k, seq[:8])
            subs += list(dict.fromkeys(windows))  # the repeats have at most 4 distinct windows
        check_kmer_layer(rk, subs, mirror_every=13)


@pytest.mark.parametrize("max_k", [32, 64, 96, 128])
def test_kmer_layer_random_strings(max_k):
    rng = np.random.default_rng(max_k)
    by_k = {}
    for _ in range(200):
        k = int(rng.integers(max(1, max_k - 32), max_k))
        by_k.setdefault(k, []).append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, k)))
    for k, subs in by_k.items():
        check_kmer_layer(O.RefKmer(k), subs, mirror_every=3)


@pytest.mark.parametrize("kmer,nl,longs,h,mini,mhash", APPENDIX_A)
def test_appendix_a_recomputed_by_reference(kmer, nl, longs, h, mini, mhash):
    """SURVEY.md Appendix A's rows are what the reference's code returns, not only what the survey says it does."""
    k = len(kmer)
    rk = O.RefKmer(k)
    assert rk.nl == nl
    la = rk.from_string(kmer)
    assert [int(x) for x in la] == longs
    assert rk.hash(la) == h
    _, mlen = rk.target_ranks(la, 1)  # the length the reference's KmerDHT constructor picks
    assert rk.minimizer_fast(la, mlen) == mini
    assert rk.minimizer_hash_fast(la, mlen) == mhash


def test_minimizer_undefined_below_15():
    """Why no parity case has k < 15 (module docstring): the driver refuses what the reference asserts against."""
    for k in (9, 10, 11, 14):
        assert m.kcount.minimizer_len(k) == 15 > k
        rk = O.RefKmer(k)
        la = rk.from_string("ACGTACGTACGTAC"[:k])
        with pytest.raises(ValueError, match="undefined in the reference"):
            rk.minimizer_fast(la, 15)
        with pytest.raises(ValueError, match="undefined in the reference"):
            rk.target_ranks(la, 8)
    b, o = synth_set(10, 1000, 1)
    with pytest.raises(ValueError, match="undefined in the reference"):
        O.ref_analyze_kmers(b, o, 11)


# ---- whole tables: reference analyze_kmers == the C oracle ---------------------------------------------------------

# test_gpu_parity.test_synthetic_vs_oracle's k values; 9, 10 and 11 have no reference table (module docstring)
SYNTH_KS = [21, 33, 55, 63, 77, 99, 15, 31, 45, 127, 19, 22]


@pytest.mark.parametrize("k", SYNTH_KS)
def test_synthetic_reference_vs_oracle(k):
    b, o = synth_set(2000, 10000, 100 + k)
    assert_tables_equal(ref_table(b, o, k), oracle_table(b, o, k), f"k={k}")


@pytest.mark.parametrize("k", [21, 33, 63, 99])
def test_edge_cases_reference_vs_oracle(k):
    b, o = edge_case_set()
    assert_tables_equal(ref_table(b, o, k), oracle_table(b, o, k), f"edge k={k}")


@pytest.mark.parametrize("k", [21, 63])
def test_hot_kmer_reference_vs_oracle(k):
    b, o = hot_set()
    ref = ref_table(b, o, k)
    assert (ref.counts == 65535).any(), "fixture must saturate a count"
    assert_tables_equal(ref, oracle_table(b, o, k), f"hot k={k}")


@pytest.mark.parametrize("k", [33, 77])
def test_long_ragged_reference_vs_oracle(k):
    b, o = long_ragged_set(k)
    assert_tables_equal(ref_table(b, o, k), oracle_table(b, o, k), f"long/ragged k={k}")


# test_gpu_parity.test_contig_pass_vs_oracle's cases
@pytest.mark.parametrize("k,dmin", [(21, 2), (21, 1), (21, 3), (33, 2), (55, 2), (63, 4), (77, 2), (99, 3), (31, 2)])
def test_contig_pass_reference_vs_oracle(k, dmin):
    b, o, seqs, depths = ctg_set(seed=40 + k + dmin)
    ref = ref_table(b, o, k, seqs, depths, dmin_thres=dmin)
    assert_tables_equal(ref, oracle_ctg_table(b, o, seqs, depths, k, dmin_thres=dmin), f"contigs k={k} dmin={dmin}")


@pytest.mark.parametrize("dmin", [0, 1, 3, 5])
def test_dmin_thres_reference_vs_oracle(dmin):
    b, o = synth_set(1500, 8000, 7)
    assert_tables_equal(ref_table(b, o, 21, dmin_thres=dmin), oracle_table(b, o, 21, dmin_thres=dmin), f"dmin={dmin}")
    b, o, seqs, depths = ctg_set(seed=50 + dmin)
    assert_tables_equal(ref_table(b, o, 33, seqs, depths, dmin_thres=dmin),
                        oracle_ctg_table(b, o, seqs, depths, 33, dmin_thres=dmin), f"contigs dmin={dmin}")


def test_q25d75_variant_reference_vs_oracle():
    """KCOUNT_QUAL_CUTOFF and DYN_MIN_DEPTH are compile-time in the reference: the second build, at the row
    (25, 3, 0.75) of test_gpu_parity.test_parameters_vs_oracle. The two builds must differ on this input."""
    b, o = synth_set(1500, 8000, 7)
    ref = ref_table(b, o, 21, dmin_thres=3, variant="q25d75")
    assert_tables_equal(ref, oracle_table(b, o, 21, qual_cutoff=25, dmin_thres=3, dyn_min_depth=0.75), "q25d75")
    # an input on which the two parameter sets give different tables (qualities 0..31, a hot k-mer): each build
    # follows its own
    b, o = edge_case_set()
    exp_q25 = oracle_table(b, o, 21, qual_cutoff=25, dmin_thres=3, dyn_min_depth=0.75).sorted()
    exp_q20 = oracle_table(b, o, 21, dmin_thres=3).sorted()
    assert len(exp_q25) != len(exp_q20), "fixture must tell the two builds apart"
    assert_tables_equal(ref_table(b, o, 21, dmin_thres=3, variant="q25d75"), exp_q25, "q25d75, edge set")
    assert_tables_equal(ref_table(b, o, 21, dmin_thres=3), exp_q20, "default build, edge set")
    b, o, seqs, depths = ctg_set(seed=68)
    assert_tables_equal(ref_table(b, o, 21, seqs, depths, dmin_thres=3, variant="q25d75"),
                        oracle_ctg_table(b, o, seqs, depths, 21, qual_cutoff=25, dmin_thres=3, dyn_min_depth=0.75),
                        "q25d75 contigs")


@pytest.mark.parametrize("k", [21, 63, 77])
def test_world_8_equals_world_1(k):
    """With rank_n() = 8 process_seq cuts a supermer wherever the target rank changes, and every supermer still lands
    in the one local table: the table must not depend on the cuts (each k-mer in exactly one supermer, with both of
    its neighbours)."""
    b, o, seqs, depths = ctg_set(seed=70 + k)
    one = ref_table(b, o, k, seqs, depths, world=1)
    assert len(one) > 1000
    assert_tables_equal(ref_table(b, o, k, seqs, depths, world=8), one, f"world 8 vs 1, k={k}")
    assert_tables_equal(ref_table(b, o, k, seqs, depths, world=3), one, f"world 3 vs 1, k={k}")
    b, o = edge_case_set()
    assert_tables_equal(ref_table(b, o, k, world=8), ref_table(b, o, k), f"edge set, world 8 vs 1, k={k}")
