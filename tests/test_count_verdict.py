"""k_count's group verdict for compact keys (group_verdict4 in kmer_ops.hpp).

A 4-slot probe group of 32-bit key words is examined by arithmetic: m = 0..3 the slot that holds the key, 4..7 four plus
the first empty slot when the key is absent, 8 or more a full group. The CPU part compares the function itself (through
mhmkc_debug_examine4, on the host) with a restatement of the two select chains it replaces, over every group of an
alphabet that holds every kind of slot; the GPU part runs the kernels that use it into full groups, lost claims,
deferral and re-sweeps, through partly valid last slots, through a hot sweep and, unchanged, through wider keys, and
compares the whole table with the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import mhm2_proxy_amd as m
from mhm2_proxy_amd import _native as N
from common import assert_tables_equal, hot_set, oracle_table, synth_set

EMPTY = 0xFFFFFFFF
G_FULL = -8


def _select_chains(v: np.ndarray, key: int) -> np.ndarray:
    """examine_group's two select chains for single-word keys, over the rows of v (group 0: a found key's slot is its
    index in the group): the first empty slot as -1 - i, else G_FULL; the key itself takes precedence."""
    r = np.full(v.shape[0], G_FULL, dtype=np.int64)
    for i in (3, 2, 1, 0):
        r = np.where(v[:, i] == EMPTY, -1 - i, r)
    for i in (3, 2, 1, 0):
        r = np.where(v[:, i] == key, i, r)
    return r


def _groups(key: int) -> np.ndarray:
    """All 6^4 groups over: an empty slot, the key, the key with only bit 6 flipped, with only bit 31 flipped, the key
    word 0 and the largest compact key word."""
    alphabet = [EMPTY, key, key ^ 0x40, key ^ 0x80000000, 0, 0xFFFFFFC0]
    return np.array(list(itertools.product(alphabet, repeat=4)), dtype=np.uint32)


def _keys():
    rng = np.random.default_rng(8)
    rnd = (rng.integers(0, 1 << 26, size=1000, dtype=np.uint64) << np.uint64(6)).astype(np.uint32)
    return [0, 0x40, 0x80000000, 0xFFFFFFC0, 0x7FFFFFC0] + [int(x) for x in rnd]


def test_verdict_matches_select_chains():
    f = N.lib().mhmkc_debug_examine4
    f.argtypes, f.restype = [C.c_void_p, C.c_uint32], C.c_uint32
    n_found = n_empty = n_full = 0
    for key in _keys():
        assert key & 63 == 0 and key != EMPTY
        v = np.ascontiguousarray(_groups(key))
        exp = _select_chains(v, key)
        base = v.ctypes.data
        got = np.array([f(base + 16 * i, key) for i in range(v.shape[0])], dtype=np.int64)
        # the old encoding from m, as the kernels' adapter makes it (verdict_code)
        code = np.where(got < 4, got, np.where(got < 8, 3 - got, G_FULL))
        bad = np.flatnonzero(code != exp)
        assert bad.size == 0, (hex(key), [hex(int(x)) for x in v[bad[0]]], int(got[bad[0]]), int(exp[bad[0]]))
        n_found += int((exp >= 0).sum())
        n_empty += int(((exp < 0) & (exp > G_FULL)).sum())
        n_full += int((exp == G_FULL).sum())
    assert n_found and n_empty and n_full
    # groups with an empty slot before an occupied one, and with the key behind an empty slot, are among them
    v = _groups(0x7FFFFFC0)
    assert ((v[:, 0] == EMPTY) & (v[:, 1] != EMPTY)).any() and ((v[:, 0] == EMPTY) & (v[:, 3] == 0x7FFFFFC0)).any()


def hip_table(b, o, k):
    with m.KmerCounter(k) as c:
        c.add_packed_reads(b, o)
        c.finish()
        return c.fetch(), c.stats()


def check_stats(st):
    assert st["count_sum"] == st["owned_records"] == st["occurrences"]
    assert st["distinct"] == st["n_out"] + st["purged"]
    assert st["dropped"] == 0


_SETS = {}


def _input(name, k, make):
    """(bytes, offsets, oracle table) of an input, computed once per module run and left unchanged."""
    if (name, k) not in _SETS:
        b, o = make()
        _SETS[(name, k)] = (b, o, oracle_table(b, o, k))
    return _SETS[(name, k)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [64, 128, 256])
@pytest.mark.parametrize("k", [21, 15])
def test_full_groups_and_lost_claims(k, cap, knob):
    """Tables of 64 to 256 slots under far more distinct keys than they hold, so that home groups are full, keys are
    displaced, claims are lost, records are deferred and buckets are swept again. k = 15: one fine bucket per coarse
    bucket, 4000 reads of a 600 kb genome, over 1000 distinct keys in each of the 256 buckets. k = 21: compact keys
    keep 26 key bits, so there are never fewer than 2^(2k - 26) = 65536 fine buckets; 150 000 reads of a 100 Mb genome
    (19 M records, most of them keys of their own) put ~265 distinct keys into each, more than the largest table.
    No knob makes them fewer (coarse and fine bits together are at least 2k - 26), so this is the smallest input that
    overfills a 256-slot table at k = 21; its oracle table is computed once for the three cases (measured: 7 s for the
    first k = 21 case with it, 0.15 s for each of the other two)."""
    if k == 15:
        b, o, exp = _input("full", k, lambda: synth_set(4000, 600_000, 30 + k))
    else:
        b, o, exp = _input("full", k, lambda: synth_set(150_000, 100_000_000, 30 + k))
    knob("cap", cap)
    knob("fine_bits", 0)
    got, st = hip_table(b, o, k)
    if k == 15:
        assert st["distinct"] > 4 * cap * 256, st["distinct"]
    assert st["lds_misses"] > 0
    assert st["overflow_sweeps"] > 0  # more sweeps than buckets
    assert_tables_equal(got, exp, f"full groups k={k} cap={cap}")
    check_stats(st)


Q31 = 31 << 3  # PackedRead quality bits


def _homopolymer(k: int, w: int):
    """Poly-A reads of w records in all, of one key and so of one bucket: reads of up to 400 records
    (a read of length L gives L - k - 1), and for w >= 8 the last three records as reads N A^k N, whose neighbours on
    both sides are no countable base."""
    singles = 3 if w >= 8 else 0
    w -= singles
    reads = []
    while w > 0:
        t = min(w, 400)
        reads.append(np.full(k + t + 1, Q31, dtype=np.uint8))
        w -= t
    one = np.full(k + 2, Q31, dtype=np.uint8)
    one[0] = one[-1] = 4 | Q31
    reads += [one] * singles
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([r.size for r in reads], out=offs[1:])
    return np.concatenate(reads).astype(np.uint8), offs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097])
def test_one_key_one_bucket(n):
    """Exactly n records of one key in one bucket: a partly valid last wave slot, a last quad of one to four records,
    and every record after the first finds its key (or loses the claim to it)."""
    b, o = _homopolymer(21, n)
    got, st = hip_table(b, o, 21)
    assert st["max_bucket"] == n and st["occurrences"] == n
    assert_tables_equal(got, oracle_table(b, o, 21), f"one key, {n} records")
    check_stats(st)
    assert st["overflow_sweeps"] == 0


@pytest.mark.gpu
def test_hot_sweep_shares_the_verdict():
    """One bucket of at least 0xC000 records: the static, checked round loop, whose phase A examines its groups with
    the same function."""
    b, o, exp = _input("hot", 21, hot_set)
    got, st = hip_table(b, o, 21)
    assert st["max_bucket"] >= 0xC000, st["max_bucket"]
    assert_tables_equal(got, exp, "hot sweep k=21")
    check_stats(st)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 31])
def test_wider_keys_unchanged(k):
    """64-bit key words keep the select chains: a difference here means that a shared helper moved."""
    b, o, exp = _input("wide", k, lambda: synth_set(1500, 30_000, 50 + k))
    got, st = hip_table(b, o, k)
    assert_tables_equal(got, exp, f"wider keys k={k}")
    check_stats(st)
