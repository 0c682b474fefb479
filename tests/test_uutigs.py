"""The uutigs of the finished table, built on the GPU from the de Bruijn links (mhmkc_uutigs / KmerCounter.uutigs):
traverse_debruijn_graph at one rank (src/dbjg_traversal.cpp:165-289,301-307,404-407,539-541,569-596) as list ranking,
without a visited array.

uutig_lib.uutigs_ref restates the rule of include/mhmkc.h in Python. The CPU tests pin it on the oracle's tables
against the two walkers that keep a visited array (query_lib.walk_links, and the restated traversal of
include/mhmkc_dbjg.hpp through tools/bin/libmhmkc_dbjg.so) and assert that the inputs hold every structure of the rule.
The GPU tests compare the library with it on the GPU's own fetched table, check every row against its contig's bases
independently of the restatement, and run the multi-k chain with each round's uutigs fed to the next.
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
from uutig_lib import STRUCTURES, circular_set, palindrome_set, ref_lines, revcomp, tie_set, uutigs_ref

ROOT = Path(__file__).resolve().parents[1]

CPU_CASES = ([("synth", k) for k in (21, 22, 33, 63)] + [("edge", 21), ("edge", 22), ("hot", 21), ("circ", 21), ("circ", 22)]
             + [(f"pal{w}", k) for k in (6, 22, 32) for w in ("", "+")] + [("pal", 21), ("tie", 35), ("tie", 77)])
# the library takes no k % 32 == 0 (mhmkc_create), so the k = 32 palindromes stay with the CPU tests
GPU_CASES = [c for c in CPU_CASES if c[1] % 32] + [("synth", k) for k in (77, 99, 127)]


@functools.lru_cache(maxsize=None)
def case_reads(setname, k):
    if setname == "synth":
        return synth_set(3000, 20000, 5)
    if setname == "edge":
        return edge_case_set()
    if setname == "hot":
        return hot_set()
    if setname == "circ":
        return circular_set()
    if setname == "tie":
        return tie_set()
    return palindrome_set(k, setname.endswith("+"))


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
