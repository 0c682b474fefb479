"""The uutigs of the finished table, built on the GPU from the de Bruijn links (mhmkc_uutigs / KmerCounter.uutigs):
traverse_debruijn_graph at one rank (src/dbjg_traversal.cpp:165-289,301-307,404-407,539-541,569-596) as list ranking,
without a visited array.

uutig_lib.uutigs_ref restates the rule of include/mhmkc.h in Python. The CPU tests pin it on the oracle's tables
against the two walkers that keep a visited array (query_lib.walk_links, and the restated traversal of
include/mhmkc_dbjg.hpp through tools/bin/libmhmkc_dbjg.so) and assert that the inputs hold every structure of the rule.
The GPU tests compare the library with it on the GPU's own fetched table, check every row against its contig's bases
independently of the restatement, and run the multi-k chain with each round's uutigs fed to the next.

NEW_CASES are small tables (one row to a few thousand) built for what random reads do not hold: contigs whose start keys
agree in their first one, two or three key words (the contig ids then rest on the later passes of the start sort), cycles
of 2^r - 1, 2^r and 2^r + 1 rows and several cycles beside a path (both branches of both parity steps of the cycle phase),
one- and two-row tables, and k at the key-word boundaries. The test knob query_grid makes the grid-stride loops stride.
"""
from __future__ import annotations

import ctypes as C
import functools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mhm2_proxy_amd as m
from mhm2_proxy_amd import _native as N
from common import edge_case_set, hot_set, oracle_table, synth_set
from query_lib import NO_ROW, links_ref, walk_links
from uutig_lib import (MULTI_CYCLES, MULTI_LINEAR, STRUCTURES, TIE_X, circular_set, common_prefix, cycle_set,
                       multi_cycle_set, order_tie_set, palindrome_set, ref_lines, revcomp, tie_set, tiny_set, uutigs_ref)

ROOT = Path(__file__).resolve().parents[1]

CPU_CASES = ([("synth", k) for k in (21, 22, 33, 63)] + [("edge", 21), ("edge", 22), ("hot", 21), ("circ", 21), ("circ", 22)]
             + [(f"pal{w}", k) for k in (6, 22, 32) for w in ("", "+")] + [("pal", 21), ("tie", 35), ("tie", 77)])
# the library takes no k % 32 == 0 (mhmkc_create), so the k = 32 palindromes stay with the CPU tests
GPU_CASES = [c for c in CPU_CASES if c[1] % 32] + [("synth", k) for k in (77, 99, 127)]

# Start keys that agree in their first `word` key words. otie<word>: six contigs whose ids are decided in word `word` (one
# to three words agree; 2, 3 and 4 sort passes); tie<word>: one contig whose two smallest keys first differ in word `word`
ORDER_TIES = [(f"otie{w}", k) for k, w in ((35, 1), (77, 1), (77, 2), (99, 2), (99, 3), (127, 3), (127, 1))]
TIES = [(f"tie{w}", k) for k, w in ((77, 2), (99, 3), (127, 3), (127, 2))]
# one cycle of 2^r - 1, 2^r, 2^r + 1 rows; several cycles of different lengths beside a path and a self-loop
CYCLE_LENGTHS = tuple(2**r + d for r in range(5, 10) for d in (-1, 0, 1))
CYCLES = [(f"cyc{n}", 21) for n in CYCLE_LENGTHS] + [("multi", 21)]
TINY = [(f"tiny{rows}", k) for k in (21, 63) for rows in (1, 2)]
# key-word boundaries: 31 bases in one word, 1 and 31 bases in the third, 1 in the fourth; even k above 32 (the palindrome's
# non-mutual port on a multi-word key) and the hairpins next to them
BOUNDARY = ([(f"pal{w}", k) for k in (34, 66, 98) for w in ("", "+")] + [("pal", k) for k in (33, 65, 97)]
            + [("circ", k) for k in (31, 65, 95, 97)])
NEW_CASES = ORDER_TIES + TIES + CYCLES + TINY + BOUNDARY
CPU_CASES = CPU_CASES + NEW_CASES


@functools.lru_cache(maxsize=None)
def case_reads(setname, k):
    if setname == "synth":
        return synth_set(3000, 20000, 5)
    if setname == "edge":
        return edge_case_set()
    if setname == "hot":
        return hot_set()
    long_reads = {"read_len": 160} if k > 90 else {}  # (a read of 100 holds too few windows of such a k for the tiling)
    if setname == "circ":
        return circular_set(**long_reads)
    if setname == "tie":
        return tie_set()
    if setname.startswith("otie"):
        return order_tie_set(int(setname[4:]))
    if setname.startswith("tie"):
        return tie_set(word=int(setname[3:]), **long_reads)
    if setname.startswith("cyc"):
        return cycle_set(int(setname[3:]))
    if setname == "multi":
        return multi_cycle_set()
    if setname.startswith("tiny"):
        return tiny_set(k, int(setname[4:]))
    return palindrome_set(k, setname.endswith("+"), **long_reads)


@functools.lru_cache(maxsize=None)
def cpu_case(setname, k):
    """The oracle's table of a case, its links and the restated uutigs (computed once, never changed)."""
    b, o = case_reads(setname, k)
    t = oracle_table(b, o, k)
    nxt, status, _ = links_ref(t)
    return t, nxt, status, uutigs_ref(t, nxt, status)


@pytest.mark.parametrize("setname,k", CPU_CASES)
def test_restated_rule_equals_the_link_walker(setname, k):
    """CPU: the rule without a visited array gives the contigs of the walker with one (canonical sequence and depth)."""
    t, nxt, status, ref = cpu_case(setname, k)
    assert ref_lines(ref) == walk_links(t, nxt, status)
    assert int(ref["n_kmers"].sum()) == ref["n_walkable"] == int((ref["row_ctg"] != NO_ROW).sum())
    assert len(ref["seqs"]) > 0
    assert [len(s) for s in ref["seqs"]] == [int(x) + k - 1 for x in ref["n_kmers"]]


def traverse_lib():
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    from mhm2_proxy_amd import build as bld

    bld.build_lib()
    N.lib()  # first, through the package's loader: it settles which HIP runtime serves the process (_native.py)
    L = C.CDLL(str(bld.build_dbjg()))
    L.mhmkc_dbjg_traverse.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p]
    L.mhmkc_dbjg_traverse.restype = C.c_int64
    return L


@pytest.mark.parametrize("setname,k", [c for c in CPU_CASES if c[1] % 32])
def test_restated_rule_equals_the_host_traversal(setname, k, tmp_path):
    """CPU: contig for contig, in the order and (for odd k) on the strand of the restated traversal of
    include/mhmkc_dbjg.hpp; its depth is Contig::get_uint16_t_depth() (src/contigs.hpp:65)."""
    t, _, _, ref = cpu_case(setname, k)
    L = traverse_lib()
    path = tmp_path / "ctgs.txt"
    keys = np.ascontiguousarray(t.keys[:, :k // 32 + 1])
    n = L.mhmkc_dbjg_traverse(k, keys.ctypes.data, np.ascontiguousarray(t.counts).ctypes.data,
                              np.ascontiguousarray(t.left).ctypes.data, np.ascontiguousarray(t.right).ctypes.data, len(t),
                              str(path).encode())
    host = [x.split() for x in path.read_text().splitlines()]
    assert n == len(host) == len(ref["seqs"])
    for c, (seq, depth) in enumerate(host):
        mine = ref["seqs"][c]
        if k % 2:
            assert mine == seq, f"contig {c}"
        else:  # (a start that is its own reverse complement may come out on the other strand)
            assert min(mine, revcomp(mine)) == min(seq, revcomp(seq)), f"contig {c}"
        assert int(min(ref["depths"][c], 65535.0)) == int(depth), f"contig {c}"


def test_inputs_hold_every_structure():
    """CPU: a path, a cycle of many rows, a cycle of one, a hairpin end, and a non-mutual port on a row that is not /
    that is its component's start; the circular genome is one cycle of 500 rows; every even-k palindrome has exactly
    one row with a non-mutual port."""
    met = set()
    for setname, k in CPU_CASES:
        ref = cpu_case(setname, k)[3]
        met |= ref["met"]
        if setname == "circ":
            assert "cycle_many" in ref["met"] and int(ref["n_kmers"].max()) == 500
        if setname == "edge":
            assert "cycle_one" in ref["met"]
        if setname == "tie":  # one contig whose two smallest keys share their first word
            strs = sorted(m.keys_to_strings(cpu_case(setname, k)[0].keys, k))
            assert len(ref["seqs"]) == 1 and strs[0][:32] == strs[1][:32] == "A" * 16 + "C" + "A" * 15
        if setname.startswith("pal"):
            if k % 2:
                assert "hairpin" in ref["met"]
            else:
                assert ("nonmutual_start" if setname.endswith("+") else "nonmutual_inner") in ref["met"]
                assert ref["n_nonmutual"] == 1
    assert met == set(STRUCTURES)


def test_new_inputs_hold_their_structure():
    """CPU: what the tie, cycle, tiny and word-boundary inputs are for, asserted on the oracle's tables, so that a change
    to a generator cannot lose it."""
    for setname, k in NEW_CASES:
        t, _, _, ref = cpu_case(setname, k)
        what = f"{setname} k={k}"
        strs = sorted(m.keys_to_strings(t.keys, k))
        if setname.startswith("otie"):  # six paths; the start keys agree in exactly their first `word` words
            word = int(setname[4:])
            assert len(ref["seqs"]) == 6 and ref["met"] == {"path"}, what
            assert all(s.startswith(TIE_X) for s in ref["start_keys"]), what
            assert ref["start_keys"] == sorted(ref["start_keys"]) == strs[:6], what
            assert common_prefix(ref["start_keys"]) == 32 * word, what
        elif setname.startswith("tie"):  # one contig; its two smallest keys agree in exactly their first `word` words
            word = int(setname[3:])
            assert len(ref["seqs"]) == 1 and strs[0].startswith(TIE_X) and common_prefix(strs[:2]) == 32 * word, what
        elif setname.startswith("cyc"):
            n = int(setname[3:])
            assert len(t) == n and ref["n_kmers"].tolist() == [n] and ref["cyclic"].tolist() == [True], what
        elif setname == "multi":
            sizes = sorted((1,) + MULTI_CYCLES + (MULTI_LINEAR - k - 1,))
            assert len(t) == sum(sizes) == 1545 and sorted(ref["n_kmers"].tolist()) == sizes, what
            assert sorted(ref["n_kmers"][ref["cyclic"]].tolist()) == sorted((1,) + MULTI_CYCLES), what
            assert ref["met"] == {"cycle_one", "cycle_many", "path"}, what
        elif setname.startswith("tiny"):
            rows = int(setname[4:])
            assert len(t) == rows and ref["n_kmers"].tolist() == [rows], what
        elif setname == "circ":
            assert ref["n_kmers"].tolist() == [500] and ref["cyclic"].all(), what
        elif k % 2:
            assert "hairpin" in ref["met"], what
        else:  # a key of two, three, four words that is its own reverse complement
            assert ("nonmutual_start" if setname.endswith("+") else "nonmutual_inner") in ref["met"], what
            assert ref["n_nonmutual"] == 1 and k > 32, what


def cycle_phase_parities(n: int, longest_path: int, longest_cycle: int):
    """The two parity-dependent steps of the cycle phase of uutigs_build (mhm2_proxy_amd/csrc/mhmkc_host.cpp) for a table
    of n rows that holds a cycle: (extra & 1 before `extra += extra & 1`, whether the closing `if (F != F0)` round runs).
      max_rounds: the smallest r >= 1 with 2^r >= 2 n, plus 1 ("int max_rounds = 1; while ((1ull << max_rounds) < 2 * n)
        max_rounds++; max_rounds++;").
      rounds of the first loop ("while (rounds < max_rounds)", left at "if (!active || active == prev) break;"): after
        round r a port is done iff its end is at most 2^r - 1 ports away, so the paths' ports, at most longest_path - 1
        from their end, are done after max(1, ceil(log2 longest_path)) rounds, and the count stands still one round later;
        a table of cycles alone stops after 2.
      extra = max(0, max_rounds - rounds) ("int extra = std::max(0, max_rounds - rounds);").
      closing rounds ("for (int x = 0; left && x <= max_rounds; x++)"): the opened cycle of L rows is a path of L rows,
        done after max(1, ceil(log2 L)) rounds; an odd number leaves F != F0."""
    max_rounds = max(1, (2 * n - 1).bit_length()) + 1
    rounds = min(max_rounds, max(1, (max(1, longest_path) - 1).bit_length()) + 1)
    extra = max(0, max_rounds - rounds)
    closing = max(1, (longest_cycle - 1).bit_length())
    return extra & 1, closing & 1


def test_cycle_inputs_reach_both_branches_of_both_parity_steps():
    """CPU: over the cycle sweep and `multi`, `extra` is odd and even before it is rounded up, and the number of closing
    rounds is odd and even (the `if (F != F0)` round runs and does not)."""
    seen = set()
    for setname, k in CYCLES:
        t, _, _, ref = cpu_case(setname, k)
        paths = ref["n_kmers"][~ref["cyclic"]]
        seen.add(cycle_phase_parities(len(t), int(paths.max()) if len(paths) else 0, int(ref["n_kmers"][ref["cyclic"]].max())))
    assert {x[0] for x in seen} == {0, 1} and {x[1] for x in seen} == {0, 1}, seen
    # the arithmetic by hand: 31 rows: max_rounds 7, extra 5, 5 closing rounds; 33 rows: max_rounds 8, extra 6, 6 closing
    assert cycle_phase_parities(31, 0, 31) == (1, 1) and cycle_phase_parities(33, 0, 33) == (0, 0)


# ---- GPU


def gpu_table(b, o, k):
    c = m.KmerCounter(k)
    c.add_packed_reads(b, o)
    c.finish()
    return c, c.fetch()


class DeviceArray:
    """A device buffer of the library as a __cuda_array_interface__ object (read through torch)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def contig_strings(offsets, seqs):
    blob = seqs.tobytes().decode("ascii")
    return [blob[int(offsets[c]):int(offsets[c + 1])] for c in range(len(offsets) - 1)]


def assert_uutigs(c, t, what):
    """The library's uutigs and row map against the restated rule over the table t, and against the rows themselves."""
    k = t.k
    nxt, status = c.dbjg_links()
    ref = uutigs_ref(t, nxt, status)
    offsets, seqs, depths, n_kmers = c.uutigs()
    row_ctg, row_pos, row_rc = c.uutig_rows()
    assert offsets.dtype == np.uint64 and (offsets == ref["offsets"]).all(), what
    assert n_kmers.dtype == np.uint32 and (n_kmers == ref["n_kmers"]).all(), what
    assert (row_ctg == ref["row_ctg"]).all() and (row_pos == ref["row_pos"]).all(), what
    got = contig_strings(offsets, seqs)
    if k % 2:
        assert got == ref["seqs"], what
        assert (row_rc == ref["row_rc"]).all(), what
    else:
        assert [min(s, revcomp(s)) for s in got] == [min(s, revcomp(s)) for s in ref["seqs"]], what
    # one IEEE division of the same integers: bit for bit
    assert depths.dtype == np.float64 and (depths.view(np.uint64) == ref["depths"].view(np.uint64)).all(), what
    # independent of the restatement: every row lies where the row map says, and the rows cover every base
    strs = m.keys_to_strings(t.keys, k)
    covered = [np.zeros(len(s), dtype=bool) for s in got]
    for i in np.flatnonzero(row_ctg != NO_ROW):
        cc, p = int(row_ctg[i]), int(row_pos[i])
        assert got[cc][p:p + k] == (revcomp(strs[i]) if row_rc[i] else strs[i]), f"{what}: row {i}"
        covered[cc][p:p + k] = True
    assert all(x.all() for x in covered), what
    assert int((row_ctg != NO_ROW).sum()) == int(n_kmers.sum())
    return ref, (offsets, seqs, depths, n_kmers), (row_ctg, row_pos, row_rc)


@pytest.mark.gpu
@pytest.mark.parametrize("setname,k", GPU_CASES)
def test_uutigs_equal_the_restated_rule(setname, k, knob):
    import torch

    b, o = case_reads(setname, k)
    c, t = gpu_table(b, o, k)
    try:
        n = len(t)
        ref, (offsets, seqs, depths, n_kmers), (row_ctg, row_pos, row_rc) = assert_uutigs(c, t, f"{setname} k={k}")
        assert len(depths) > 0
        # the device arrays hold the same as the fetch
        dev = c.uutigs_device()
        nc, nb = dev["n_ctgs"], dev["n_bases"]
        assert (nc, nb, dev["n_out"]) == (len(depths), len(seqs), n)
        c.synchronize()

        def read(name, count, typestr, dtype):
            return torch.as_tensor(DeviceArray(dev[name], count, typestr), device="cuda").cpu().numpy().view(dtype)

        assert (read("offsets", 2 * (nc + 1), "<i4", np.uint64) == offsets).all()
        assert (read("seqs", nb, "|u1", np.uint8) == seqs).all()
        assert (read("depths", 2 * nc, "<i4", np.uint64) == depths.view(np.uint64)).all()
        assert (read("row_ctg", n, "<i4", np.uint32) == row_ctg).all()
        assert (read("row_pos", n, "<i4", np.uint32) == row_pos).all()
        assert (read("row_rc", n, "|u1", np.uint8) == row_rc).all()
        # a second count on the same handle, the index at a load near 1: the same contigs
        first = (contig_strings(offsets, seqs), depths.copy(), n_kmers.copy())
        c.reset()
        knob("query_slots_log2", int(n).bit_length())
        c.add_packed_reads(b, o)
        c.finish()
        _, (o2, s2, d2, m2), _ = assert_uutigs(c, c.fetch(), f"{setname} k={k} second count")
        assert contig_strings(o2, s2) == first[0] and (d2 == first[1]).all() and (m2 == first[2]).all()
    finally:
        c.close()


def assert_start_order(c, t, what):
    """Independent of the restatement: the contigs' smallest keys, read from the row map and the table as strings,
    increase strictly with the contig id, and for odd k the row that holds a contig's smallest key lies forward in it."""
    k = t.k
    strs = m.keys_to_strings(t.keys, k)
    row_ctg, _, row_rc = c.uutig_rows()
    n_ctgs = len(c.uutigs()[2])
    smallest = [None] * n_ctgs
    for i in np.flatnonzero(row_ctg != NO_ROW):
        cc = int(row_ctg[i])
        if smallest[cc] is None or strs[i] < smallest[cc][0]:
            smallest[cc] = (strs[i], int(i))
    assert all(x is not None for x in smallest), what
    keys = [x[0] for x in smallest]
    assert all(a < b for a, b in zip(keys, keys[1:])), f"{what}: contig ids do not follow the start keys: {keys}"
    if k % 2:
        assert all(row_rc[i] == 0 for _, i in smallest), what
    return keys


def assert_cycle_info(c, ref, what):
    """uutigs_info of the build against the restated rule: the ports on cycles, and what uutigs_build fixes about the
    cycle phase's rounds (none without a cycle; an even number with one: `extra` is rounded up to even and the closing
    rounds come in pairs)."""
    info = c.uutigs_info()
    on_cycles = int(ref["n_kmers"][ref["cyclic"]].sum())
    assert info["cycle_ports"] == 2 * on_cycles, what
    assert (info["cycle_rounds"] > 0) == (on_cycles > 0) and info["cycle_rounds"] % 2 == 0, f"{what}: {info}"
    if on_cycles:
        assert info["rounds"] >= 2, what
    assert (info["n_ctgs"], info["n_bases"]) == (len(ref["seqs"]), int(ref["offsets"][-1])), what


@pytest.mark.gpu
@pytest.mark.parametrize("setname,k", NEW_CASES)
def test_new_cases_equal_the_restated_rule(setname, k):
    """One small count per case: the start keys that agree in one, two and three key words, the cycle lengths around
    the powers of two, several cycles beside a path, tables of one and two rows, and the key-word boundaries."""
    b, o = case_reads(setname, k)
    c, t = gpu_table(b, o, k)
    try:
        what = f"{setname} k={k}"
        ref = assert_uutigs(c, t, what)[0]
        assert len(t) == len(cpu_case(setname, k)[0]) and len(ref["seqs"]) == len(cpu_case(setname, k)[3]["seqs"]), what
        assert_cycle_info(c, ref, what)
        if "tie" in setname:
            keys = assert_start_order(c, t, what)
            word = int(setname[-1])
            tied = keys if setname.startswith("otie") else sorted(m.keys_to_strings(t.keys, k))[:2]
            assert len(keys) == (6 if setname.startswith("otie") else 1) and common_prefix(tied) == 32 * word, what
    finally:
        c.close()


STRIDED = [("synth", 21), ("multi", 21), ("otie3", 99), ("pal+", 22)]


@pytest.mark.gpu
@pytest.mark.parametrize("setname,k", STRIDED)
def test_strided_launches_give_the_same_uutigs(setname, k, knob):
    """The test knob query_grid caps every query and uutig kernel at 1 and at 3 workgroups (256 and 768 threads, which
    divide neither the ports nor each other's strides evenly), so every grid-stride loop runs many times per thread and
    the lanes of k_uutig_jump leave it at different iterations before the wave's sum: the same contigs as the kernels'
    own grid gives."""
    b, o = case_reads(setname, k)
    c, t = gpu_table(b, o, k)
    try:
        assert 2 * len(t) > 2 * 256  # one workgroup strides over the ports at least twice
        _, (offsets, seqs, depths, n_kmers), _ = assert_uutigs(c, t, f"{setname} k={k}")
        first = (contig_strings(offsets, seqs), depths.copy(), n_kmers.copy())
        for grid in (1, 3):
            c.reset()
            knob("query_grid", grid)
            c.add_packed_reads(b, o)
            c.finish()
            what = f"{setname} k={k} query_grid={grid}"
            t2 = c.fetch()
            ref, (o2, s2, d2, m2), _ = assert_uutigs(c, t2, what)
            assert contig_strings(o2, s2) == first[0] and (d2 == first[1]).all() and (m2 == first[2]).all(), what
            assert_cycle_info(c, ref, what)
            if setname.startswith("otie"):
                assert_start_order(c, t2, what)
    finally:
        c.close()


@pytest.mark.gpu
def test_state_empty_table_and_accounting():
    """Before finish: MHMKC_ESTATE; an empty table: no contigs, offsets = [0]; the kept buffers are counted in
    device_bytes (9 bytes per row, 1 per base, 20 per contig + 8) and the ranking's scratch is not; reset gives all back."""
    b, o = synth_set(3000, 20000, 5)
    c = m.KmerCounter(21)
    try:
        c.add_packed_reads(b, o)
        for call in (c.uutigs, c.uutig_rows, c.uutigs_device):
            with pytest.raises(N.MhmkcError) as e:
                call()
            assert e.value.code == -5  # MHMKC_ESTATE
        n = c.finish()
        plain = c.stats()["device_bytes"]  # a handle without queries
        c.dbjg_links()
        before = c.stats()["device_bytes"]
        offsets, seqs, depths, n_kmers = c.uutigs()
        after = c.stats()
        kept = 9 * n + len(seqs) + 20 * len(depths) + 8
        assert after["device_bytes"] >= before + kept
        assert after["device_bytes"] < before + kept + kept // 8 + 64 * 1024  # (the ranking's 128 bytes per row are gone)
        assert after["device_bytes_peak"] >= before + 128 * n
        info = c.uutigs_info()
        assert (info["n_ctgs"], info["n_bases"]) == (len(depths), len(seqs)) and info["rounds"] >= 2
        assert info["kept_bytes"] == after["device_bytes"] - before and info["scratch_bytes"] >= 128 * n
        strs, d = c.uutig_strings()
        assert [len(s) for s in strs] == [int(x) + 20 for x in n_kmers] and (d == depths).all()
        assert c.stats()["device_bytes"] == after["device_bytes"]  # built once per finish
        c.reset()
        assert c.stats()["device_bytes"] == plain
        with pytest.raises(N.MhmkcError) as e:
            c.uutigs()
        assert e.value.code == -5  # and after reset
        c.add_packed_reads(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        assert c.finish() == 0  # no reads: an empty table
        offsets, seqs, depths, n_kmers = c.uutigs()
        assert offsets.tolist() == [0] and len(seqs) == len(depths) == len(n_kmers) == 0
        assert all(len(x) == 0 for x in c.uutig_rows())
        assert c.uutig_strings()[0] == []
    finally:
        c.close()


def build_dbjg_test(tmp: Path) -> Path:
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    from mhm2_proxy_amd import build as bld

    bld.build_lib()
    bld.build_oracle()
    exe = tmp / "dbjg_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/dbjg_test.cpp"),
                    f"-L{ROOT / 'mhm2_proxy_amd'}", "-lmhmkc", f"-L{ROOT / 'oracle'}", "-loracle", "-lz",
                    f"-Wl,-rpath,{ROOT / 'mhm2_proxy_amd'}", f"-Wl,-rpath,{ROOT / 'oracle'}", "-o", str(exe)],
                   check=True)
    return exe


@pytest.mark.gpu
def test_multik_chain_on_device_uutigs(tmp_path):
    """End to end: the rounds k = 21, 33, 55, each round's uutig_strings() fed to the next round's add_ctgs, equal round
    by round what tests/cpp/dbjg_test.cpp prints in gpu mode (the host traversal over the adapter's KmerMap)."""
    exe = build_dbjg_test(tmp_path)
    b, o = synth_set(3000, 20000, 5)
    pr = m.PackedReads.from_arrays(b, o)
    rf = tmp_path / "reads.txt"
    with open(rf, "w") as f:
        for i in range(pr.get_local_num_reads()):
            _, s, q = pr.get_read(i)
            f.write(f"{s} {q}\n")
    out = subprocess.run([str(exe), "gpu", str(rf), "21,33,55"], capture_output=True, text=True, check=True).stdout
    exp, k = {}, None
    for line in out.splitlines():
        if line.startswith("K "):
            k = int(line.split()[1])
            exp[k] = []
        else:
            exp[k].append(line)
    assert list(exp) == [21, 33, 55]
    ctgs, depths = [], np.zeros(0)
    for k in (21, 33, 55):
        c = m.KmerCounter(k)
        try:
            c.add_packed_reads(b, o)
            if ctgs:  # Contig::get_uint16_t_depth() (src/contigs.hpp:65)
                c.add_ctgs(ctgs, np.minimum(depths, 65535.0).astype(np.uint16))
            c.finish()
            ctgs, depths = c.uutig_strings()
        finally:
            c.close()
        got = sorted(f"{min(s, revcomp(s))} {d:.6f}" for s, d in zip(ctgs, depths))
        assert len(got) == len(exp[k]) > 0, f"k={k}"
        assert got == exp[k], f"k={k}"


@pytest.mark.gpu
def test_uutigs_refuse_multirank_handle():
    """mhmkc_uutigs is single-rank, as the links it is built from: EUNSUPPORTED, checked before the state."""
    L = N.lib()
    cfg = N.MhmkcConfig()
    L.mhmkc_config_init(C.byref(cfg))
    cfg.n_ranks, cfg.rank = 2, 0
    h = C.c_void_p()
    assert L.mhmkc_create(C.byref(h), C.byref(cfg)) == 0
    try:
        nc, nb = C.c_uint64(), C.c_uint64()
        assert L.mhmkc_uutigs(h, C.byref(nc), C.byref(nb)) == -7
        assert L.mhmkc_uutigs_fetch(h, None, None, None, None) == -7
        assert L.mhmkc_uutigs_device(h, None, None, None, None, None) == -7
        assert L.mhmkc_uutig_rows(h, None, None, None) == -7
        assert L.mhmkc_uutig_rows_device(h, None, None, None) == -7
    finally:
        L.mhmkc_destroy(h)


def test_null_handle_uutig_calls_fail_cleanly():
    """CPU only: no handle, no GPU."""
    L = N.lib()
    assert L.mhmkc_uutigs(None, None, None) == -1
    assert L.mhmkc_uutigs_fetch(None, None, None, None, None) == -1
    assert L.mhmkc_uutigs_device(None, None, None, None, None, None) == -1
    assert L.mhmkc_uutig_rows(None, None, None, None) == -1
    assert L.mhmkc_uutig_rows_device(None, None, None, None) == -1
    assert L.mhmkc_uutigs_info(None, None) == -1
