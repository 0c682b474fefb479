"""k_count's dynamic cold sweeps at the edges of their slot arithmetic (guided tail slots).

A cold sweep hands its records to the 16 waves in wave slots (compact keys 256 records, two-word keys 64; a round is
16 slots); each wave's first two slots are pre-assigned, the rest come from a counter, and the sweep's last TAIL_SLOTS
wave slots go out as TAIL_DIV sub-slots each. The cases below put an exact number of records into one fine bucket, at
every size where that arithmetic takes another path, and compare the whole table with the CPU oracle.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import mhm2_proxy_amd as m
from common import assert_tables_equal, hot_set, oracle_table, synth_set

pytestmark = pytest.mark.gpu


def hip_table(b, o, k):
    with m.KmerCounter(k) as c:
        c.add_packed_reads(b, o)
        c.finish()
        return c.fetch(), c.stats()


def check_stats(st):
    assert st["count_sum"] == st["owned_records"] == st["occurrences"]
    assert st["distinct"] == st["n_out"] + st["purged"]
    assert st["dropped"] == 0


NWV = 16  # waves of a k_count workgroup
# the build constants of mhm2_proxy_amd/csrc/kcount_kernels.hip (MHMKC_TAIL_DIV / _SLOTS, ...2 for two-word keys)
# (the shipped build hands out whole slots to the end, TAIL_DIV = 1: the edges below are then those of the whole slots.
# A variant library built with -DMHMKC_TAIL_DIV=d -DMHMKC_TAIL_DIV2=d, selected by MHMKC_LIB, is run with
# MHMKC_TEST_TAIL_DIV=d, which puts the sub-slot edges into the sizes)
_DIV = int(os.environ.get("MHMKC_TEST_TAIL_DIV", "1"))
TAIL_DIV = {1: _DIV, 2: _DIV}
TAIL_SLOTS = {1: 4, 2: 4}
Q31 = 31 << 3  # PackedRead quality bits


def _join(reads):
    lens = np.array([r.size for r in reads], dtype=np.uint64)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    return (np.concatenate(reads) if reads else np.zeros(0, np.uint8)).astype(np.uint8), offs


def _split(b, o):
    return [b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)]


def _homopolymer(k: int, w: int):
    """Poly-A reads that give w records in all, of one key and so of one fine bucket. A read of length L gives
    L - k - 1 records (its first and last k-mer have a neighbour on one side only and are not counted, as in the
    reference): reads of up to 400 records, and the last three records as reads N A^k N (one record each, whose
    neighbours on both sides are no countable base)."""
    singles = 3 if w >= 8 else 0
    w -= singles
    reads = []
    while w > 0:
        t = min(w, 400)
        reads.append(np.full(k + t + 1, Q31, dtype=np.uint8))
        w -= t
    one = np.full(k + 2, Q31, dtype=np.uint8)
    one[0] = one[-1] = 4 | Q31
    return reads + [one] * singles


_BG = {}
_BG_SHARE = {}  # k -> background records in the poly-A k-mer's fine bucket


def _background(k: int):
    if k not in _BG:
        _BG[k] = _split(*synth_set(2000, 20000, 40 + k))
    return _BG[k]


def _run_bucket(k: int, n: int):
    """Counts an input whose largest fine bucket holds exactly n records (asserted through max_bucket): the poly-A
    k-mer's, on top of 2000 random reads once n is far above their own buckets (~60 records)."""
    bg = _background(k) if n >= 1000 else []
    share = _BG_SHARE.get(k, 0) if bg else 0
    for _ in range(2):
        b, o = _join(bg + _homopolymer(k, n - share))
        got, st = hip_table(b, o, k)
        if st["max_bucket"] == n:
            break
        share += st["max_bucket"] - n  # the background's records in that bucket: the same for every n
    if bg:
        _BG_SHARE[k] = share
    assert st["max_bucket"] == n, (k, n, st["max_bucket"])
    assert_tables_equal(got, oracle_table(b, o, k), f"k={k} bucket of {n}")
    check_stats(st)
    assert st["overflow_sweeps"] == 0


def _edges(nl: int):
    slot = 256 if nl == 1 else 64
    rnd, sub = NWV * slot, slot // TAIL_DIV[nl]
    tb = (2 * NWV + TAIL_SLOTS[nl]) * slot  # above it the sweep has more slots than the pre-assigned ones + the tail
    n0 = 76 * slot                          # the headline's bucket: 76 wave slots
    e = {
        "first_slots": [1, 3, 4, 5, slot - 1, slot, slot + 1, rnd - 1, rnd, rnd + 1, 2 * rnd - 1, 2 * rnd, 2 * rnd + 1],
        "tail_begin": [tb - 1, tb, tb + 1, tb + sub - 1, tb + sub, tb + sub + 1, tb + slot - 1, tb + slot, tb + slot + 1],
        "tail_long": [n0 - sub - 1, n0 - sub, n0 - sub + 1, n0 - 1, n0, n0 + 1, n0 + 2, n0 + 3, n0 + sub - 1, n0 + sub + 1,
                      n0 + 2 * sub + 2, 78 * slot + 31],
    }
    return {g: list(dict.fromkeys(v)) for g, v in e.items()}  # (sub == slot gives some sizes twice)


@pytest.mark.parametrize("group", ["first_slots", "tail_begin", "tail_long"])
@pytest.mark.parametrize("k", [21, 63])
def test_exact_bucket_sizes(k, group):
    for n in _edges(1 if k <= 21 else 2)[group]:
        assert n < 0xC000
        _run_bucket(k, n)


@pytest.mark.parametrize("k", [15, 33])
def test_exact_bucket_sizes_second_k(k):
    """The same edges at the other compact / two-word k, thinned."""
    e = _edges(1 if k <= 21 else 2)
    for n in e["first_slots"][3::3] + e["tail_begin"][::2] + e["tail_long"][4:9]:
        _run_bucket(k, n)


def _periodic_reads(k: int, copies: int):
    """Reads of period 2, 3 and 5 and lengths k .. k + 5 (L - k - 1 records each, none below k + 2): every k-mer of
    a read is one of at most five keys; every second read has N as its first and last base, so that its first and last
    record have no countable neighbour on one side."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    motifs = ["AC", "AG", "CT", "ACG", "AAC", "CCG", "AGT", "ACGTT", "AACCG", "AGGCT", "ATCCA", "CAGTA"]
    reads = []
    for mo in motifs:
        for ln in range(k, k + 6):
            for ph in range(len(mo)):
                r = np.array([code[mo[(ph + i) % len(mo)]] for i in range(ln)], dtype=np.uint8) | np.uint8(Q31)
                if (ln + ph) & 1:
                    r[0] = r[-1] = 4 | Q31
                reads += [r] * copies
    return reads


@pytest.mark.parametrize("k", [15, 63])
def test_short_period_reads_in_tail_slots(k, knob):
    """Short-period reads next to random ones, with one fine bucket per coarse bucket, so that the buckets are long
    enough for a tail and its sub-slots hold several distinct keys with left-none and right-none extensions."""
    nl = 1 if k <= 21 else 2
    slot = 256 if nl == 1 else 64
    per_bucket = (2 * NWV + TAIL_SLOTS[nl] + 6) * slot
    n_reads = per_bucket * 256 // (150 - k - 1)
    rnd = np.random.default_rng(7)
    reads = _split(*synth_set(n_reads, 50000, 70 + k)) + _periodic_reads(k, 40)
    reads = [reads[i] for i in rnd.permutation(len(reads))]
    b, o = _join(reads)
    exp = oracle_table(b, o, k)
    knob("fine_bits", 0)
    got, st = hip_table(b, o, k)
    assert (2 * NWV + TAIL_SLOTS[nl]) * slot < st["max_bucket"] < 0xC000, st["max_bucket"]
    assert_tables_equal(got, exp, f"short periods k={k}")
    check_stats(st)


@pytest.mark.parametrize("k", [15, 63])
def test_deferral_through_tail_slots(k, knob):
    """64-slot tables and one fine bucket per coarse bucket: the first sweep of a bucket is long enough for a tail and
    defers most of its keys from whole slots and sub-slots alike; the spilled records come back through dynamic
    re-sweeps of a few hundred to a few thousand records, no multiple of a sub-slot."""
    nl = 1 if k <= 21 else 2
    slot = 256 if nl == 1 else 64
    per_bucket = (2 * NWV + TAIL_SLOTS[nl] + 6) * slot
    b, o = synth_set(per_bucket * 256 // (150 - k - 1), 50000, 13 + k)
    exp = oracle_table(b, o, k)
    knob("cap", 64)
    knob("fine_bits", 0)
    got, st = hip_table(b, o, k)
    assert (2 * NWV + TAIL_SLOTS[nl]) * slot < st["max_bucket"] < 0xC000, st["max_bucket"]
    assert st["overflow_sweeps"] > 0
    assert_tables_equal(got, exp, f"deferral k={k}")
    check_stats(st)


def test_hot_sweep_then_dynamic_resweeps(knob):
    """A bucket above 0xC000 records (the static, checked round loop) that overflows a 64-slot table, followed by cold
    re-sweeps: the static and the dynamic path still hand over to each other."""
    b, o = hot_set()
    exp = oracle_table(b, o, 15)
    knob("cap", 64)
    knob("fine_bits", 0)
    got, st = hip_table(b, o, 15)
    assert st["max_bucket"] >= 0xC000, st["max_bucket"]
    assert st["overflow_sweeps"] > 0
    assert_tables_equal(got, exp, "hot sweep, cold re-sweeps")
