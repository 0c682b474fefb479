"""k_count's compact cold round and per-bucket path after round 9 (DESIGN.md §3.3 "Round 9"): the counter planes'
order (MHMKC_ADDLUT = 2), the add pair without a conditional region (MHMKC_ADD0), wave-uniform validity (MHMKC_VALIDU)
and the finalize's pass 1 (MHMKC_FIN1).

Every case counts a small input through the library and compares the whole table and the stats with the CPU oracle.
The test-only knobs `cap` (64-slot tables) and `fine_bits` put the rare paths into small inputs.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import mhm2_proxy_amd as m
from common import assert_tables_equal, ctg_set, oracle_ctg_table, oracle_table, synth_set
from test_count_tail_slots import _join, _run_bucket, _split, check_stats, hip_table

pytestmark = pytest.mark.gpu

Q31 = 31 << 3  # PackedRead quality bits: far above the cutoff
Q2 = 2 << 3    # below it
COMP = np.array([3, 2, 1, 0], dtype=np.uint8)


def _neighbour(x: int, alt: bool) -> np.uint8:
    """Extension x = 0..3 a good base; 4 none: an N, or (alt) a base below the quality cutoff."""
    if x < 4:
        return np.uint8(x | Q31)
    return np.uint8((1 | Q2) if alt else (4 | Q31))


def _rc(kmer: np.ndarray) -> np.ndarray:
    return COMP[kmer[::-1]]


def _canonical(kmer: np.ndarray) -> np.ndarray:
    r = _rc(kmer)
    return kmer if tuple(kmer) <= tuple(r) else r


def _pair_reads(kmer: np.ndarray, weights) -> list:
    """Reads x K y (one record each: K with left x and right y) for all 25 (x, y), weights[5 x + y] copies each."""
    reads = []
    for x in range(5):
        for y in range(5):
            r = np.concatenate([[_neighbour(x, (x + y) & 1)], kmer | np.uint8(Q31), [_neighbour(y, (x + y) & 1 == 0)]])
            reads += [r.astype(np.uint8)] * int(weights[5 * x + y])
    return reads


def _weights(dominant: int, big: int) -> np.ndarray:
    """Every pair a different number of times (1 .. 25), one of them `big` more often: the slot's ten counters all
    differ, and get_ext's choice on each side names the planes and halves the dominant pair was added to."""
    w = 1 + np.arange(25)
    w[dominant] += big
    return w


def _pair_keys(k: int, rc: bool, seed: int) -> list:
    """25 distinct random k-mers and poly-A (key word 0), each as its canonical form, or as the reverse complement of
    it (the extraction then swaps and complements the neighbours)."""
    rng = np.random.default_rng(seed)
    keys = [_canonical(rng.integers(0, 4, k).astype(np.uint8)) for _ in range(25)] + [np.zeros(k, dtype=np.uint8)]
    return [_rc(x) if rc else x for x in keys]


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("k", [15, 21])
def test_every_extension_pair_through_the_cold_adds(k, rc):
    """26 keys, each with all 25 (left, right) pairs of A, C, G, T and none a different number of times and another
    pair dominant (poly-A: T / none); their buckets hold ~3300 records, whole slots and a partial one."""
    reads = []
    for i, key in enumerate(_pair_keys(k, rc, 100 + k)):
        reads += _pair_reads(key, _weights(i if i < 25 else 19, 3000 + 100 * i))  # (every key another count)
    rng = np.random.default_rng(3)
    b, o = _join([reads[i] for i in rng.permutation(len(reads))])
    got, st = hip_table(b, o, k)
    exp = oracle_table(b, o, k)
    assert len(exp) == 25  # (the key whose dominant pair is none / none has no extension on either side: purged)
    assert st["max_bucket"] < 0xC000
    assert_tables_equal(got, exp, f"extension pairs k={k} rc={rc}")
    check_stats(st)


@pytest.mark.parametrize("dominant", [0 * 5 + 3, 1 * 5 + 4, 4 * 5 + 2, 3 * 5 + 0, 2 * 5 + 1])
def test_extension_pairs_through_a_hot_first_sweep(dominant):
    """One key with more than 0xC000 records: the static round loop with returning adds and clamps (lds_add, lds_clamp)
    on the same planes. The five dominant pairs put every left and every right counter, and none, above the clamp."""
    k = 21
    key = _pair_keys(k, False, 7)[dominant]
    b, o = _join(_pair_reads(key, _weights(dominant, 0xC800)))
    got, st = hip_table(b, o, k)
    assert st["max_bucket"] >= 0xC000, st["max_bucket"]
    assert_tables_equal(got, oracle_table(b, o, k), f"hot pairs, dominant {dominant}")
    check_stats(st)


@functools.lru_cache(maxsize=None)
def _ctg_case(k: int):
    b, o, seqs, depths = ctg_set(seed=700 + k)
    return b, o, seqs, depths, oracle_ctg_table(b, o, seqs, depths, k)


@pytest.mark.parametrize("cap", [0, 64])
@pytest.mark.parametrize("k", [15, 21, 63])
def test_contig_pass_reads_and_writes_the_planes(k, cap, knob):
    """ctg_apply reads a found slot's count and four extension words and overwrites them with the contig entry (the
    explicit count of a cold sweep); 64-slot tables spread a bucket's contig k-mers over several sweeps."""
    b, o, seqs, depths, exp = _ctg_case(k)
    if cap:
        knob("cap", cap)
        knob("fine_bits", 0)
    with m.KmerCounter(k) as c:
        c.add_packed_reads(b, o)
        c.add_ctgs(seqs, depths)
        c.finish()
        assert c.stats()["ctg_kmers"] > 0
        assert_tables_equal(c.fetch(), exp, f"contig pass k={k} cap={cap}")


@pytest.mark.parametrize("k", [15, 21])
def test_whole_and_partial_slots(k):
    """Fine buckets of exactly n records: the sweep's last slot mixes valid and invalid lanes (and quads that are
    valid in part), every slot before it is whole; no lane past the end may count."""
    for n in (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 76 * 256 - 1, 76 * 256 + 1):
        _run_bucket(k, n)


@pytest.mark.parametrize("k,per_bucket", [(15, 300), (15, 1500), (15, 9000), (21, 80)])
def test_misses_in_64_slot_tables(k, per_bucket, knob):
    """64-slot tables under more distinct keys than they hold: home groups fill up, claims are lost, a wave's queue
    passes its threshold and its capacity within a round (the in-place insert), and keys are deferred to later
    sweeps, from whole slots and from the partial last one. k = 15: one fine bucket per coarse bucket, 256 buckets of
    ~per_bucket records. k = 21: compact keys keep 26 key bits, so there are never fewer than 65536 fine buckets; reads
    of a 100 Mb genome, nearly every record a key of its own, put ~80 keys into each (the smallest input that
    overfills 64 slots at this k: 5 M records)."""
    if k == 15:
        b, o = synth_set(per_bucket * 256 // (150 - k - 1), 50000, 17 + k + per_bucket)
    else:
        b, o = synth_set(per_bucket * 65536 // (150 - k - 1), 100_000_000, 17 + k)
    exp = oracle_table(b, o, k)
    knob("cap", 64)
    knob("fine_bits", 0)
    got, st = hip_table(b, o, k)
    assert st["overflow_sweeps"] > 0
    assert st["max_bucket"] < 0xC000
    assert_tables_equal(got, exp, f"64-slot tables k={k}, ~{per_bucket} records per bucket")
    check_stats(st)


def _copies_set(copies, seed: int):
    """Reads over a genome far longer than they cover (nearly every k-mer occurs once per read), read i copies[i %
    len(copies)] times: tables whose slots hold exactly those counts."""
    reads = _split(*synth_set(600, 2_000_000, seed))
    out = []
    for i, r in enumerate(reads):
        out += [r] * copies[i % len(copies)]
    return _join(out)


@pytest.mark.parametrize("cap", [64, 68, 6144])
@pytest.mark.parametrize("copies", [(1,), (1, 2, 3), (2,)], ids=["count1", "around2", "count2"])
def test_finalize_pass1_edges(cap, copies, knob):
    """Pass 1 over tables that are empty (most of the 256 buckets' later sweeps and every bucket without records),
    full of slots with count 1 (nothing listed), and mixed around count 2, at table sizes that are no multiple of the
    workgroup's 4096 slots per iteration: 16 and 17 quads (one wave, the others leave at once) and 1536."""
    b, o = _copies_set(copies, 40 + len(copies))
    k = 15  # (one fine bucket per coarse bucket: ~300 records and more than 64 keys in each of the 256 buckets)
    exp = oracle_table(b, o, k)
    knob("cap", cap)
    knob("fine_bits", 0)
    got, st = hip_table(b, o, k)
    if cap < 6144:
        assert st["overflow_sweeps"] > 0
    if copies == (1,):
        assert st["distinct"] > 50000 and len(exp) < st["distinct"] // 20
    assert_tables_equal(got, exp, f"pass 1, cap={cap}, copies={copies}")
    check_stats(st)
