"""The de Bruijn links of every row (mhmkc_dbjg_links / KmerCounter.dbjg_links): the lookup of get_next_step
(src/dbjg_traversal.cpp:165-239) done once for all rows and both directions, on the GPU.

query_lib.links_ref restates the rules of include/mhmkc.h over a KmerTable with a Python dict. The CPU test runs it on
the oracle's tables and asserts that the inputs reach every case of the rules; the GPU tests compare
mhmkc_dbjg_links with it on the GPU's own fetched table (exact equality), and a walker that follows only the links
reproduces the contigs of the restated traversal (include/mhmkc_dbjg.hpp) with no k-mer lookup on the host.
"""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mhm2_proxy_amd as m
from common import edge_case_set, hot_set, oracle_table, synth_set
from query_lib import CONFLICT, DEADEND, FORK, NO_ROW, OK, RC, WHY, links_ref, walk_links
from uutig_lib import palindrome_set

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("k", [21, 22, 33, 63])
def test_rules_are_all_reached_on_the_oracle_table(k):
    """CPU: the synthetic set's table holds, in both directions, every case of the link rules."""
    b, o = synth_set(3000, 20000, 5)
    t = oracle_table(b, o, k)
    nxt, status, why = links_ref(t)
    for d in (0, 1):
        seen = {WHY[w] for w in np.unique(why[d])}
        assert seen == set(WHY), f"k={k} direction {d}: missing {set(WHY) - seen}"
    # the arrays are consistent with each other
    assert ((status & ~np.uint8(RC)) <= CONFLICT).all()
    assert ((nxt == NO_ROW) == np.isin(why, [2, 3, 5])).all()
    assert (((status & RC) != 0) <= ((status & ~np.uint8(RC)) == OK)).all()
    assert {int(s) for s in np.unique(status)} == {OK, OK | RC, DEADEND, FORK, CONFLICT}


def test_poly_a_links_to_itself():
    """CPU: edge_case_set holds the poly-A k-mer, whose neighbour in both directions is itself."""
    b, o = edge_case_set()
    t = oracle_table(b, o, 21)
    nxt, status, _ = links_ref(t)
    strs = m.keys_to_strings(t.keys, 21)
    i = strs.index("A" * 21)
    assert nxt[0, i] == i and nxt[1, i] == i
    assert (chr(t.left[i]), chr(t.right[i])) == ("A", "A") and status[0, i] == OK and status[1, i] == OK


def test_walker_follows_a_hand_made_chain():
    """CPU: the link walker on a table made by hand: one chain ACGGT -> CGGTC -> GGTCA (k = 5), entered from its
    middle row; CGGTC is stored as its reverse complement's canonical form."""
    k = 5
    kmers = {"ACGGT": (3, "T", "C"), "CGGTC": (4, "A", "A"), "GGTCA": (5, "C", "G")}
    comp = str.maketrans("ACGT", "TGCA")
    rows = []
    for s, (cnt, l, r) in kmers.items():
        rc = s[::-1].translate(comp)
        if rc < s:
            s, l, r = rc, r.translate(comp), l.translate(comp)
        rows.append((m.kmer_from_string(s, 1), cnt, ord(l), ord(r)))
    t = m.KmerTable(k, np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 1),
                    np.array([r[1] for r in rows], dtype=np.uint16), np.array([r[2] for r in rows], dtype=np.uint8),
                    np.array([r[3] for r in rows], dtype=np.uint8))
    nxt, status, _ = links_ref(t)
    lines = walk_links(t, nxt, status)
    # the start k-mer's depth counts in both walks: 3 + 4 + 5 + the start's again
    assert len(lines) == 1
    seq, depth = lines[0].split()
    assert seq in ("ACGGTCA", "TGACCGT") and seq == min("ACGGTCA", "TGACCGT")
    start = min(m.keys_to_strings(t.keys, k))
    start_cnt = int(t.counts[m.keys_to_strings(t.keys, k).index(start)])
    assert float(depth) == pytest.approx((3 + 4 + 5 + start_cnt) / (7 - k + 2), abs=1e-6)


def gpu_table(b, o, k):
    c = m.KmerCounter(k)
    c.add_packed_reads(b, o)
    c.finish()
    return c, c.fetch()


def assert_links(got, exp, what):
    for name, g, e in zip(("next", "status"), got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {name} {g.shape} {g.dtype}"
        bad = np.argwhere(g != e)
        first = tuple(bad[0]) if bad.size else None
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} entries, first {first}: {g[first]} vs {e[first]}"


class DeviceArray:
    """A device buffer of the library as a __cuda_array_interface__ object (read through torch)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


CASES = [("synth", k) for k in (21, 22, 33, 63, 77, 99, 127)] + [("edge", 21), ("hot", 21)]
# key-word boundaries (31 bases in one word; 1 and 31 bases in the third word; 1 in the fourth) on a small read set, and
# even k above 32 on the palindromes, whose centre row is its own reverse complement: a multi-word key whose neighbour in
# both directions is the same row
BOUNDARY = [("small", k) for k in (31, 65, 95, 97)] + [(f"pal{w}", k) for k in (34, 66, 98) for w in ("", "+")]
CASES += BOUNDARY
STRIDED = [("synth", 21), ("synth", 77)]


def case_reads(setname, k=0):
    if setname.startswith("pal"):
        return palindrome_set(k, setname.endswith("+"), read_len=160)
    return {"synth": lambda: synth_set(3000, 20000, 5), "small": lambda: synth_set(600, 3000, 7), "edge": edge_case_set,
            "hot": hot_set}[setname]()


@pytest.mark.gpu
@pytest.mark.parametrize("setname,k", CASES)
def test_links_equal_the_restated_rules(setname, k, knob):
    import torch

    b, o = case_reads(setname, k)
    c, t = gpu_table(b, o, k)
    try:
        n = len(t)
        exp = links_ref(t)[:2]
        assert_links(c.dbjg_links(), exp, f"{setname} k={k}")
        if setname == "small":  # links that are followed, onto both strands
            assert n > 1000 and {OK, OK | RC} <= {int(x) for x in np.unique(exp[1])}
        if setname.startswith("pal"):  # exactly one row, the genome's centre, is its own reverse complement
            comp = str.maketrans("ACGT", "TGCA")
            assert sum(s == s[::-1].translate(comp) for s in m.keys_to_strings(t.keys, k)) == 1
        # the device arrays hold the same
        dev = c.dbjg_links_device()
        assert dev["n_out"] == n
        c.synchronize()
        dn = torch.as_tensor(DeviceArray(dev["next"], 2 * n, "<i4"), device="cuda").cpu().numpy().view(np.uint32)
        ds = torch.as_tensor(DeviceArray(dev["status"], 2 * n, "|u1"), device="cuda").cpu().numpy()
        assert_links((dn.reshape(2, n), ds.reshape(2, n)), exp, f"{setname} k={k} device arrays")
        if setname == "edge":
            i = m.keys_to_strings(t.keys, k).index("A" * k)
            assert exp[0][0, i] == i and exp[0][1, i] == i
        # once more with the index at a load near 1 (a second count on the handle: the links are per finish)
        c.reset()
        knob("query_slots_log2", int(n).bit_length())
        c.add_packed_reads(b, o)
        c.finish()
        t2 = c.fetch()
        assert_links(c.dbjg_links(), links_ref(t2)[:2], f"{setname} k={k} high load")
    finally:
        c.close()


def link_lines(t, nxt, status):
    """The links by key instead of by row (the rows' order may differ from count to count), sorted."""
    strs = m.keys_to_strings(t.keys, t.k)
    return sorted((strs[i], d, strs[int(nxt[d, i])] if nxt[d, i] != NO_ROW else "", int(status[d, i]))
                  for d in (0, 1) for i in range(len(t)))


@pytest.mark.gpu
@pytest.mark.parametrize("setname,k", STRIDED)
def test_strided_launches_give_the_same_links(setname, k, knob):
    """The test knob query_grid caps the index build and k_dbjg_links at 1 and at 3 workgroups, so their grid-stride loops
    run many times per thread: the links of the kernels' own grid."""
    b, o = case_reads(setname, k)
    c, t = gpu_table(b, o, k)
    try:
        assert 2 * len(t) > 3 * 256
        nxt, status = c.dbjg_links()
        assert_links((nxt, status), links_ref(t)[:2], f"{setname} k={k}")
        first = link_lines(t, nxt, status)
        for grid in (1, 3):
            c.reset()
            knob("query_grid", grid)
            c.add_packed_reads(b, o)
            c.finish()
            t2 = c.fetch()
            n2, s2 = c.dbjg_links()
            assert_links((n2, s2), links_ref(t2)[:2], f"{setname} k={k} query_grid={grid}")
            assert link_lines(t2, n2, s2) == first, f"{setname} k={k} query_grid={grid}"
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
@pytest.mark.parametrize("k", [21, 63])
def test_walk_over_links_equals_the_traversal(k, tmp_path):
    """End to end: a walker that follows only next / status and a visited array (query_lib.walk_links) produces the
    contig list that tests/cpp/dbjg_test.cpp prints in gpu mode (the restated traversal over the host KmerMap)."""
    exe = build_dbjg_test(tmp_path)
    b, o = synth_set(3000, 20000, 5)
    pr = m.PackedReads.from_arrays(b, o)
    rf = tmp_path / "reads.txt"
    with open(rf, "w") as f:
        for i in range(pr.get_local_num_reads()):
            _, s, q = pr.get_read(i)
            f.write(f"{s} {q}\n")
    out = subprocess.run([str(exe), "gpu", str(rf), str(k)], capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert lines[0].split()[:2] == ["K", str(k)]
    exp = lines[1:]
    assert len(exp) == int(lines[0].split()[2]) > 0
    c, t = gpu_table(b, o, k)
    try:
        nxt, status = c.dbjg_links()
    finally:
        c.close()
    got = walk_links(t, nxt, status)
    assert [x.split()[0] for x in got] == [x.split()[0] for x in exp]
    assert got == exp
