"""Point queries on the finished table, answered on the GPU (mhmkc_lookup / KmerCounter.lookup: the bulk form of
KmerDHT::get_local_kmer_counts and kmer_exists, src/kcount/kmer_dht.cpp:198-219).

The expected values come from the fetched table through a Python dict: GPU lookup == the same table read back (the
table itself is pinned to the oracle by test_gpu_parity.py). Everything is compared exactly.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
from common import edge_case_set, hot_set, synth_set
from mhm2_proxy_amd import _native as N
from uutig_lib import palindrome_set
from query_lib import (NO_ROW, assert_lookup, expected_lookup, mutate_keys, pack_codes, revcomp_keys, row_dict,
                       unpack_codes)

KS = [(21, 0), (22, 0), (33, 0), (63, 0), (77, 0), (99, 0), (127, 0), (21, 2)]
_reads = {}


def base_reads():
    """synth_set(3000, 20000, 5) plus a read holding a palindromic 22-mer (ACGT repeated), given twice."""
    if "b" not in _reads:
        b, o = synth_set(3000, 20000, 5)
        pal = np.array(["ACGT".index(c) for c in "ACGT" * 40], dtype=np.uint8) | np.uint8(31 << 3)
        reads = [b, pal, pal]
        offs = np.concatenate([o, o[-1] + np.array([160, 320], dtype=np.uint64)]).astype(np.uint64)
        _reads["b"] = (np.concatenate(reads).astype(np.uint8), offs)
    return _reads["b"]


class Counted:
    """A finished counter over (b, o), its fetched table and the dict of its rows."""

    def __init__(self, b, o, k, **kw):
        self.c = m.KmerCounter(k, **kw)
        self.c.add_packed_reads(b, o)
        self.c.finish()
        self.t = self.c.fetch()
        self.d = row_dict(self.t)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.close()


def check_hits(x: Counted, k: int):
    c, t = x.c, x.t
    n = len(t)
    assert n > 1000
    exp = (np.arange(n, dtype=np.uint32), t.counts, t.left, t.right)
    assert_lookup(c.lookup(t.keys), exp, f"k={k} table keys")
    rc = revcomp_keys(t.keys, k)
    assert_lookup(c.lookup(rc, canonicalize=True), exp, f"k={k} reverse complements, canonicalize")
    # as given, a reverse complement is a miss unless the key is its own reverse complement
    pal = (rc == t.keys).all(axis=1)
    got = c.lookup(rc, canonicalize=False)
    assert_lookup(got, expected_lookup(t, x.d, rc), f"k={k} reverse complements as given")
    assert ((got[0] != NO_ROW) == pal).all()
    if k == 22:
        assert pal.sum() >= 1, "the table must hold a palindromic key"
    else:
        assert k % 2 == 0 or pal.sum() == 0


def check_misses(x: Counted, b, o, k: int, n_longs: int):
    c, t = x.c, x.t
    nlo = t.keys.shape[1]
    rng = np.random.default_rng(k)
    mut = mutate_keys(t.keys, k, rng)
    assert_lookup(c.lookup(mut), expected_lookup(t, x.d, mut), f"k={k} mutants")
    assert_lookup(c.lookup(mut, True), expected_lookup(t, x.d, mut, True), f"k={k} mutants, canonicalize")
    # the oracle's distinct k-mers that the finish purged (count < 2, or no extension reaching the threshold): every
    # occurrence's key, and the table of a depth threshold of 1, minus the table's keys
    allk = np.unique(O.extract(b, o, k, n_longs=nlo)[0], axis=0)
    lowk = O.kcount(b, o, k, n_longs=nlo, dmin_thres=1).fetch()[0]
    for what, keys in (("distinct", allk), ("dmin_thres 1", lowk)):
        purged = np.array([r for r in keys if r.tobytes() not in x.d], dtype=np.uint64).reshape(-1, nlo)
        assert purged.shape[0] >= 1, f"k={k}: no purged key among the oracle's {what} keys"
        got = c.lookup(purged)
        assert (got[0] == NO_ROW).all() and not got[1].any() and not got[2].any() and not got[3].any()
    poly = pack_codes(np.array([[0] * k, [3] * k], dtype=np.uint8), nlo)
    assert_lookup(c.lookup(poly), expected_lookup(t, x.d, poly), f"k={k} all-A, all-T")
    assert_lookup(c.lookup(poly, True), expected_lookup(t, x.d, poly, True), f"k={k} all-A, all-T, canonicalize")
    # garbage in the unused low bits of the last key word is ignored
    nl = k // 32 + 1
    junk = t.keys[:500].copy()
    unused = np.uint64((1 << (64 - 2 * (k - 32 * (nl - 1)))) - 1)
    junk[:, nl - 1] |= unused & rng.integers(0, 2**63, 500).astype(np.uint64)
    assert (junk != t.keys[:500]).any()
    assert_lookup(c.lookup(junk), c.lookup(t.keys[:500]), f"k={k} junk low bits")
    mj = mut[:500].copy()
    mj[:, nl - 1] |= np.uint64(1)
    assert_lookup(c.lookup(mj, True), c.lookup(mut[:500], True), f"k={k} junk low bits, mutants")


@pytest.mark.gpu
@pytest.mark.parametrize("k,n_longs", KS)
def test_hits(k, n_longs):
    b, o = base_reads()
    with Counted(b, o, k, n_longs=n_longs) as x:
        check_hits(x, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n_longs", KS)
def test_misses(k, n_longs):
    b, o = base_reads()
    with Counted(b, o, k, n_longs=n_longs) as x:
        check_misses(x, b, o, k, n_longs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 65, 95, 97, 34, 66, 98])
def test_hits_and_mutants_at_key_word_boundaries(k):
    """31 bases in one key word, 1 and 31 bases in the third, 1 in the fourth, on a small read set; even k above 32 on a
    palindromic genome, whose centre k-mer is a multi-word key that is its own reverse complement."""
    b, o = palindrome_set(k, False, u_len=1200, read_len=160) if k % 2 == 0 else synth_set(600, 3000, 7)
    with Counted(b, o, k) as x:
        check_hits(x, k)
        if k % 2 == 0:
            assert (revcomp_keys(x.t.keys, k) == x.t.keys).all(axis=1).sum() == 1
        mut = mutate_keys(x.t.keys, k, np.random.default_rng(k))
        assert_lookup(x.c.lookup(mut), expected_lookup(x.t, x.d, mut), f"k={k} mutants")
        assert_lookup(x.c.lookup(mut, True), expected_lookup(x.t, x.d, mut, True), f"k={k} mutants, canonicalize")


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("k", [21, 63])
def test_strided_launches_give_the_same_answers(k, grid, knob):
    """The test knob query_grid caps the index build and the lookups at 1 and at 3 workgroups, so their grid-stride loops
    run many times per thread: the answers of the kernels' own grid (which test_hits and test_misses pin to the same
    expectations)."""
    b, o = base_reads()
    knob("query_grid", grid)
    with Counted(b, o, k) as x:
        assert len(x.t) > 3 * 256
        check_hits(x, k)
        check_misses(x, b, o, k, 0)


@pytest.mark.gpu
def test_lookup_accepts_strings():
    b, o = base_reads()
    with Counted(b, o, 21) as x:
        strs = m.keys_to_strings(x.t.keys[:50], 21)
        assert_lookup(x.c.lookup(strs), x.c.lookup(x.t.keys[:50]), "strings")
        rcs = [s[::-1].translate(str.maketrans("ACGT", "TGCA")) for s in strs]
        assert_lookup(x.c.lookup(rcs, canonicalize=True), x.c.lookup(x.t.keys[:50]), "strings rc")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_batch_shapes(k):
    import torch

    b, o = base_reads()
    with Counted(b, o, k) as x:
        c, t = x.c, x.t
        n_out = len(t)
        rng = np.random.default_rng(7)
        mut = mutate_keys(t.keys, k, rng)
        for n in (0, 1, 63, 64, 65, 257):
            q = np.concatenate([t.keys[:n // 2], mut[:n - n // 2]]).reshape(n, t.keys.shape[1])
            got = c.lookup(q)
            assert all(a.shape == (n,) for a in got)
            assert_lookup(got, expected_lookup(t, x.d, q), f"n={n}")
        dup = np.repeat(t.keys[17:18], 300, axis=0)
        got = c.lookup(dup)
        assert (got[0] == 17).all() and (got[1] == t.counts[17]).all()
        # 3 n_out mixed hits, reverse complements and misses in random order
        q = np.concatenate([t.keys, revcomp_keys(t.keys, k), mut])
        q = np.ascontiguousarray(q[rng.permutation(q.shape[0])])
        for canon in (False, True):
            exp = expected_lookup(t, x.d, q, canon)
            host = c.lookup(q, canon)
            assert_lookup(host, exp, f"3 n_out mixed, canonicalize={canon}")
            # the tensor variant (mhmkc_lookup_device) agrees with the host variant
            qt = torch.from_numpy(q.view(np.int64)).cuda()
            rows, counts, left, right = c.lookup_tensors(qt, canon)
            dev = (rows.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint16), left.cpu().numpy(),
                   right.cpu().numpy())
            assert_lookup(dev, host, f"tensors, canonicalize={canon}")
        # sync=False + synchronize(), and NULL outputs through the C ABI
        qt = torch.from_numpy(t.keys.view(np.int64).copy()).cuda()
        rows = c.lookup_tensors(qt, sync=False)[0]
        c.synchronize()
        assert (rows.cpu().numpy().view(np.uint32) == np.arange(n_out)).all()
        only_counts = np.empty(n_out, dtype=np.uint16)
        c._check(N.lib().mhmkc_lookup(c._h, t.keys.ctypes.data, n_out, 0, None, only_counts.ctypes.data, None, None))
        assert (only_counts == t.counts).all()
        c._check(N.lib().mhmkc_lookup(c._h, t.keys.ctypes.data, n_out, 0, None, None, None, None))


@pytest.mark.gpu
def test_empty_table():
    with m.KmerCounter(21) as c:
        c.add_packed_reads(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        assert c.finish() == 0
        q = pack_codes(np.random.default_rng(1).integers(0, 4, (70, 21)).astype(np.uint8), 1)
        rows, counts, left, right = c.lookup(q, True)
        assert (rows == NO_ROW).all() and not counts.any() and not left.any() and not right.any()
        assert c.lookup(q[:0])[0].shape == (0,)
        nxt, status = c.dbjg_links()
        assert nxt.shape == (2, 0) and status.shape == (2, 0)
        assert c.dbjg_links_device()["n_out"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_one_row_table(k):
    rng = np.random.default_rng(k)
    read = rng.integers(0, 4, k + 2).astype(np.uint8) | np.uint8(31 << 3)
    b = np.concatenate([read, read])
    o = np.array([0, k + 2, 2 * (k + 2)], dtype=np.uint64)
    with Counted(b, o, k) as x:
        assert len(x.t) == 1
        assert_lookup(x.c.lookup(x.t.keys), ([0], x.t.counts, x.t.left, x.t.right), "one row")
        assert_lookup(x.c.lookup(revcomp_keys(x.t.keys, k), True), ([0], x.t.counts, x.t.left, x.t.right), "one row rc")
        mut = mutate_keys(np.repeat(x.t.keys, 64, axis=0), k, rng)
        assert (x.c.lookup(mut)[0] == NO_ROW).all()


@pytest.mark.gpu
@pytest.mark.parametrize("setname", ["edge", "hot"])
def test_edge_and_hot_tables(setname):
    b, o = edge_case_set() if setname == "edge" else hot_set()
    with Counted(b, o, 21) as x:
        t = x.t
        exp = (np.arange(len(t), dtype=np.uint32), t.counts, t.left, t.right)
        assert_lookup(x.c.lookup(t.keys), exp, setname)
        assert_lookup(x.c.lookup(revcomp_keys(t.keys, 21), True), exp, setname + " rc")
        poly = pack_codes(np.array([[0] * 21, [3] * 21], dtype=np.uint8), 1)
        got = x.c.lookup(poly, True)
        assert got[0][0] == got[0][1] != NO_ROW  # poly-A is in both tables; poly-T canonicalises to it
        if setname == "hot":
            assert got[1][0] == 65535
        mut = mutate_keys(t.keys, 21, np.random.default_rng(3))
        assert_lookup(x.c.lookup(mut), expected_lookup(t, x.d, mut), setname + " mutants")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_probe_chains(k, knob):
    """The index at a load near 1 (the smallest power of two above n_out): long probe chains, the wrap past the last
    slot; the answers are those of the default capacity."""
    b, o = base_reads()
    with Counted(b, o, k) as x:
        n_out = len(x.t)
        v = int(n_out).bit_length()  # 2^v > n_out >= 2^(v-1)
        assert (1 << v) > n_out >= (1 << (v - 1))
        knob("query_slots_log2", v - 1)
        with pytest.raises(N.MhmkcError) as e:
            x.c.lookup(x.t.keys[:4])
        assert e.value.code == -1  # MHMKC_EINVAL: 2^v <= n_out
        knob("query_slots_log2", v)
        check_hits(x, k)
        check_misses(x, b, o, k, 0)


@pytest.mark.gpu
def test_state():
    b, o = base_reads()
    b2, o2 = synth_set(2000, 15000, 11)
    with m.KmerCounter(21) as c:
        q = np.zeros((3, 1), dtype=np.uint64)
        c.add_packed_reads(b, o)
        with pytest.raises(N.MhmkcError) as e:
            c.lookup(q)
        assert e.value.code == -5  # MHMKC_ESTATE before finish
        with pytest.raises(N.MhmkcError) as e:
            c.dbjg_links()
        assert e.value.code == -5
        c.finish()
        t = c.fetch()
        before = c.stats()["device_bytes"]
        assert (c.lookup(t.keys)[0] == np.arange(len(t))).all()
        c.dbjg_links()
        with_index = c.stats()
        assert with_index["device_bytes"] >= before + 16 * len(t)  # >= 2 n_out slots of 8 bytes
        assert with_index["device_bytes_peak"] >= with_index["device_bytes"]
        c.reset()
        assert c.stats()["device_bytes"] == before
        with pytest.raises(N.MhmkcError) as e:
            c.lookup(q)
        assert e.value.code == -5  # and after reset
        # a second count on the same handle, other reads: the answers are the new table's
        c.add_packed_reads(b2, o2)
        c.finish()
        t2 = c.fetch()
        d2 = row_dict(t2)
        assert_lookup(c.lookup(t2.keys), (np.arange(len(t2), dtype=np.uint32), t2.counts, t2.left, t2.right), "second")
        assert_lookup(c.lookup(t.keys), expected_lookup(t2, d2, t.keys), "first table's keys in the second")
        assert (c.lookup(t.keys)[0] == NO_ROW).any()


@pytest.mark.gpu
def test_links_refuse_multirank_handle():
    """mhmkc_dbjg_links is single-rank (as include/mhmkc_dbjg.hpp): EUNSUPPORTED, checked before the state."""
    L = N.lib()
    cfg = N.MhmkcConfig()
    L.mhmkc_config_init(C.byref(cfg))
    cfg.n_ranks, cfg.rank = 2, 0
    h = C.c_void_p()
    assert L.mhmkc_create(C.byref(h), C.byref(cfg)) == 0
    try:
        assert L.mhmkc_dbjg_links(h, None, None) == -7
        pn, ps = C.c_void_p(), C.c_void_p()
        assert L.mhmkc_dbjg_links_device(h, C.byref(pn), C.byref(ps)) == -7
        assert L.mhmkc_lookup(h, None, 0, 0, None, None, None, None) == -5  # lookups: local rows, but not before finish
    finally:
        L.mhmkc_destroy(h)


def test_null_handle_queries_fail_cleanly():
    """CPU only: no handle, no GPU."""
    L = N.lib()
    assert L.mhmkc_lookup(None, None, 0, 0, None, None, None, None) == -1
    assert L.mhmkc_lookup_device(None, None, 0, 0, None, None, None, None) == -1
    assert L.mhmkc_dbjg_links(None, None, None) == -1
    assert L.mhmkc_dbjg_links_device(None, None, None) == -1
    assert N.MHMKC_NO_ROW == NO_ROW == 0xFFFFFFFF
    assert L.mhmkc_debug_set(b"query_slots_log2", 0) == 0
    assert L.mhmkc_debug_set(b"query_grid", 3) == 0 and L.mhmkc_debug_set(b"query_grid", 0) == 0


def test_query_helpers_roundtrip():
    """CPU only: the tests' vectorised packing agrees with kmer_from_string / keys_to_strings."""
    rng = np.random.default_rng(0)
    for k in (21, 22, 63, 99):
        codes = rng.integers(0, 4, (20, k)).astype(np.uint8)
        nl = k // 32 + 1
        keys = pack_codes(codes, nl)
        strs = ["".join("ACGT"[c] for c in row) for row in codes]
        assert [tuple(int(x) for x in r) for r in keys] == [m.kmer_from_string(s, nl) for s in strs]
        assert (unpack_codes(keys, k) == codes).all()
        rcs = [s[::-1].translate(str.maketrans("ACGT", "TGCA")) for s in strs]
        assert m.keys_to_strings(revcomp_keys(keys, k), k) == rcs


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_larger_table(k):
    b, o = synth_set(200_000, 2_000_000, 3)
    with m.KmerCounter(k) as c:
        c.add_packed_reads(b, o)
        n_out = c.finish()
        t = c.fetch()
        assert n_out > 1_000_000
        rows, counts, left, right = c.lookup(t.keys)
        assert (rows == np.arange(n_out, dtype=np.uint32)).all()
        assert (counts == t.counts).all() and (left == t.left).all() and (right == t.right).all()
        rng = np.random.default_rng(k)
        mut = mutate_keys(t.keys[rng.integers(0, n_out, 1_000_000)], k, rng)
        rows = c.lookup(mut)[0]
        hit = rows != NO_ROW
        # np.isin on the packed keys: the first word filters, the few candidates are compared whole
        cand = np.isin(mut[:, 0], t.keys[:, 0])
        assert not (hit & ~cand).any()
        exp = np.zeros(mut.shape[0], dtype=bool)
        ci = np.flatnonzero(cand)
        if ci.size:
            if k <= 31:
                exp[ci] = True
            else:
                d = {r.tobytes() for r in t.keys[np.isin(t.keys[:, 0], mut[ci, 0])]}
                exp[ci] = [mut[i].tobytes() in d for i in ci]
        assert (hit == exp).all()
        assert (t.keys[rows[hit]] == mut[hit]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_kmer_dht_queries(k):
    """The Python KmerDHT: get_local_kmer_counts answers from the GPU what the local_kmers dict holds (no dict is
    built for it), kmer_exists canonicalises."""
    b, o = base_reads()
    dht = m.KmerDHT(k)
    try:
        m.analyze_kmers(k, 0, 33, [m.PackedReads.from_arrays(b, o)], 2, [], dht)
        t = dht.table
        strs = m.keys_to_strings(t.keys[:40], k)
        comp = str.maketrans("ACGT", "TGCA")
        for i, s in enumerate(strs):
            exp = m.KmerCounts(int(t.counts[i]), chr(int(t.left[i])), chr(int(t.right[i])))
            assert dht.get_local_kmer_counts(s) == exp
            assert dht.get_local_kmer_counts(tuple(int(x) for x in t.keys[i])) == exp
            rc = s[::-1].translate(comp)
            assert dht.kmer_exists(s) and dht.kmer_exists(rc)
            assert (dht.get_local_kmer_counts(rc) is None) == (rc != s)
        assert dht._map is None, "get_local_kmer_counts must not build the whole-table dict"
        mut = m.keys_to_strings(mutate_keys(t.keys[:200], k, np.random.default_rng(k)), k)
        got = [dht.get_local_kmer_counts(s) for s in mut]
        in_map = dht.local_kmers  # the dict, built here for the comparison only
        assert got == [in_map.get(m.kmer_from_string(s)) for s in mut]
        canon = [min(s, s[::-1].translate(comp)) for s in mut]
        assert [dht.kmer_exists(s) for s in mut] == [m.kmer_from_string(c) in in_map for c in canon]
        # without a live table on the counter (reset since) the dict answers as before
        dht.clear_stores()
        first = m.KmerCounts(int(t.counts[0]), chr(int(t.left[0])), chr(int(t.right[0])))
        assert dht.get_local_kmer_counts(strs[0]) == first
    finally:
        dht.counter.close()
