"""Device contigs on handles of several ranks (mhmkc_add_ctgs_device / mhmkc_add_ctgs_from with n_ranks > 1 and
MHMKC_OWNER_MINIMIZER; mhmkc_ctgs_ranks_info; kcount_ctgx.hip): every rank adds its own contigs locally
and mhmkc_finish gathers the contigs of all ranks on the device, in rank order.

The GPU tests run 2 and 3 ranks (processes sharing the one GPU, exchanging over gloo) and 2 ranks over RCCL; one spawn per
world serves all of that world's cases and its chain (module-scoped fixtures, tests/mr_ctgs_worker.py). Every comparison
is bit-exact table equality with the CPU oracle given the concatenation of the ranks' contigs in rank order. The CPU tests
pin the ABI, the host half of the wire format, and that the inputs can show a wrong order.
"""
from __future__ import annotations

import ctypes as C
import functools
import shutil
import socket
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mhm2_proxy_amd as m
from mhm2_proxy_amd import _native as N
from common import assert_tables_equal, ctg_set, oracle_ctg_table
from mr_ctgs_worker import EDGES, case_data, case_file, split_contiguous

ROOT = Path(__file__).resolve().parents[1]
CPP = ROOT / "tests" / "cpp"
EINVAL, ESTATE, EBADCHAR, EUNSUPPORTED = -1, -5, -6, -7

KS = (21, 33, 63)
CHAIN_KS = [21, 33, 55]
ORDER = [f"order:{k}" for k in KS]
ORDER_HOST = [f"order_host:{k}" for k in KS]
MIXED = ["mixed:a", "mixed:b"]
EDGE_CASES = [f"edge:{e}" for e in EDGES] + [f"edge:{e}@{g}" for e in ("e1", "e4", "e8") for g in (1, 3)]
CASES = ORDER + ORDER_HOST + MIXED + EDGE_CASES + ["errors:"]
RCCL_CASES = ["order:33", "mixed:a", "edge:e4", "edge:e8@3"]
INFO_FIELDS = [f for f, _ in N.MhmkcCtgRanksInfo._fields_]


# ---- CPU: the ABI, the wire format's host half, the inputs -------------------------------------------------------

def test_new_symbol_is_exported_and_refuses_null():
    from mhm2_proxy_amd import build

    build.build_lib()
    L = N.lib()
    assert hasattr(L, "mhmkc_ctgs_ranks_info") and "mhmkc_ctgs_ranks_info" in N.ABI_SYMBOLS
    info = N.MhmkcCtgRanksInfo()
    assert L.mhmkc_ctgs_ranks_info(None, C.byref(info)) == EINVAL and L.mhmkc_ctgs_ranks_info(None, None) == EINVAL
    assert L.mhmkc_abi_version() == 14
    assert L.mhmkc_debug_set(b"ctgx_grid", 3) == 0 and L.mhmkc_debug_set(b"ctgx_grid", 0) == 0


def test_header_with_the_new_struct_is_plain_c_and_matches_ctypes(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    src = tmp_path / "t.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mhmkc.h"', "int main(void) {",
             "  mhmkc_ctg_ranks_info info;", "  if (mhmkc_ctgs_ranks_info(0, &info) != MHMKC_EINVAL) return 1;",
             '  printf("sizeof %zu\\n", sizeof(mhmkc_ctg_ranks_info));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mhmkc_ctg_ranks_info, {f}));' for f in INFO_FIELDS]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    from mhm2_proxy_amd import build

    build.build_lib()
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(src), f"-L{ROOT / 'mhm2_proxy_amd'}", "-lmhmkc",
                    f"-Wl,-rpath,{ROOT / 'mhm2_proxy_amd'}", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env={"MHMKC_NO_TORCH": "1"})
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(ln.split() for ln in out.stdout.strip().split("\n"))
    assert int(got["sizeof"]) == C.sizeof(N.MhmkcCtgRanksInfo)
    for f in INFO_FIELDS:
        assert int(got[f]) == getattr(N.MhmkcCtgRanksInfo, f).offset, f


def test_nibble_pack_helper_on_the_host(tmp_path):
    """CPU: ctg_nib8 / ctg_nib4 (kmer_ops.hpp) for every pair of the ten contig byte values in every lane position, and
    the round trip through the expand rule; built with the address and undefined-behaviour sanitizers."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path / "ctg_nib_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(CPP / "ctg_nib_check.cpp"), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-2000:] + out.stderr[-2000:]


def revcomp(s: str) -> str:
    return s.upper()[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def test_rank_major_split_keeps_order_dependent_contigs_apart():
    """CPU, on the oracle: contiguous shards of ctg_set() put the two members of a duplicated pair with different depths
    (contigs that share every k-mer, so that one rank's contig folds into another's) on different ranks for 2 and for 3
    ranks. (Measured on the oracle: ctg_set()'s final table is the same with the shards applied in the reverse order,
    since the fold's min and its purge of disagreeing contig k-mers commute for these contigs. The GPU tests therefore
    pin the table the contract names, and the cross-rank folding, not the order by itself.)"""
    b, o, seqs, depths = ctg_set()
    canon = [min(s.upper(), revcomp(s)) for s in seqs]
    for world in (2, 3):
        cuts = split_contiguous(len(seqs), list(range(world)), world)
        rank_of = np.concatenate([np.full(hi - lo, r) for r, (lo, hi) in enumerate(cuts)])
        first = {}
        apart = 0
        for i, cs in enumerate(canon):
            j = first.setdefault(cs, i)
            apart += j != i and rank_of[i] != rank_of[j] and int(depths[i]) != int(depths[j]) and len(cs) >= 63 + 2
        assert apart >= 1, f"world {world}: no duplicated contig pair across ranks"
        # what the pair changes: the oracle's table with only the first shard's contigs differs from the full one, so
        # a rank whose contigs are lost, or land on another rank's bytes, shows
        for k in KS:
            lo, hi = cuts[0]
            a = oracle_ctg_table(b, o, seqs, depths, k)
            z = oracle_ctg_table(b, o, seqs[lo:hi], depths[lo:hi], k)
            assert len(a) != len(z) or (a.counts != z.counts).any(), f"world {world} k={k}"


# ---- GPU: the spawns -----------------------------------------------------------------------------------------------

def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn(world, plan, out_dir, opts):
    """`world` worker processes (with this one at most 4 hold the GPU at a time)."""
    import torch.multiprocessing as mp

    import mr_ctgs_worker as W

    mp.spawn(W.serve, args=(world, free_port(), plan, str(out_dir), opts), nprocs=world, join=True)


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    d = tmp_path_factory.mktemp("cranks_w2")
    spawn(2, {"cases": CASES, "chain": CHAIN_KS}, d, {})
    return d


@pytest.fixture(scope="module")
def world3(tmp_path_factory):
    d = tmp_path_factory.mktemp("cranks_w3")
    spawn(3, {"cases": CASES, "chain": CHAIN_KS}, d, {})
    return d


@pytest.fixture(scope="module")
def rccl2(tmp_path_factory):
    d = tmp_path_factory.mktemp("cranks_rccl2")
    spawn(2, {"cases": RCCL_CASES, "chain": CHAIN_KS}, d, {"rccl": True})
    return d


@pytest.fixture(scope="module")
def single_chain():
    """The single-rank device chain (add_ctgs_from): per k its table and the number of its uutigs. Computed once."""
    from mr_uutig_worker import case_reads

    b, o = case_reads("synth", 21)
    out, prev = {}, None
    for k in CHAIN_KS:
        c = m.KmerCounter(k)
        c.add_packed_reads(b, o)
        if prev is not None:
            c.add_ctgs_from(prev)
            prev.close()
        c.finish()
        out[k] = (c.fetch(), len(c.uutigs()[2]))
        prev = c
    prev.close()
    return out


def load(out_dir, world, name):
    return [dict(np.load(case_file(out_dir, name, r))) for r in range(world)]


def union(parts, k) -> m.KmerTable:
    return m.KmerTable(k, np.concatenate([p["keys"] for p in parts]), np.concatenate([p["counts"] for p in parts]),
                       np.concatenate([p["left"] for p in parts]), np.concatenate([p["right"] for p in parts]))


@functools.lru_cache(maxsize=None)
def expected(name: str, world: int):
    """The oracle's table of a case: all reads, the ranks' contigs concatenated in rank order (computed once)."""
    k, b, o, per_rank, _ = case_data(name, world)
    seqs = [s for r in per_rank for s in r[0]]
    depths = np.concatenate([np.asarray(r[1], dtype=np.uint16) for r in per_rank])
    return oracle_ctg_table(b, o, seqs, depths, k)


def check_info(parts, name, world, device_route: int):
    """mhmkc_ctg_ranks_info of every rank against the sizes computed here."""
    k, _, _, per_rank, _ = case_data(name, world)
    what = f"{name} world {world}"
    lens = [[len(s) for s in r[0]] if r[2] != "none" else [] for r in per_rank]
    n_r = [len(x) for x in lens]
    b_r = [sum(x) for x in lens]
    windows = sum(L - k - 1 for x in lens for L in x if L >= k + 2)
    for r, p in enumerate(parts):
        assert (p["zeros"] == 0).all() and (p["cleared"] == 0).all(), f"{what}: info not zero before a finish / after reset"
        assert int(p["info_device_route"]) == device_route, what
        assert (int(p["info_n_ctgs"]), int(p["info_n_bases"])) == (n_r[r], b_r[r]), f"{what}: rank {r}"
        assert (int(p["info_n_ctgs_all"]), int(p["info_n_bases_all"]), int(p["info_windows_all"])) == \
            (sum(n_r), sum(b_r), windows), f"{what}: rank {r}"
        if device_route:
            assert int(p["info_bytes_sent"]) == (world - 1) * (6 * n_r[r] + (b_r[r] + 1) // 2), f"{what}: rank {r}"
            assert int(p["info_bytes_recv"]) == sum(6 * n_r[q] + (b_r[q] + 1) // 2 for q in range(world) if q != r), what
            # the gathered copy: the bytes, two u64 arrays and the u16 depths at least; it was live at the peak
            assert int(p["info_gathered_bytes"]) >= sum(b_r) + 18 * sum(n_r), what
            assert int(p["device_bytes_peak"]) >= int(p["info_gathered_bytes"]), what
            assert float(p["info_ms_total"]) > 0 and float(p["info_ms_total"]) >= float(p["info_ms_move"]) >= 0, what
        else:
            for f in ("bytes_sent", "bytes_recv", "gathered_bytes", "ms_pack", "ms_move", "ms_assemble", "ms_total"):
                assert float(p["info_" + f]) == 0, f"{what}: {f} on the host route"
        # the second round on the counter leaves the device memory where it found it
        assert int(p["after"]) == int(p["before"]), f"{what}: rank {r}: device_bytes {p['before']} -> {p['after']}"
    assert sum(int(p["info_bytes_sent"]) for p in parts) == sum(int(p["info_bytes_recv"]) for p in parts), what


def check_device_case(out_dir, world, name):
    k = case_data(name, world)[0]
    parts = load(out_dir, world, name)
    assert_tables_equal(union(parts, k), expected(name, world), f"{name} world {world}")
    check_info(parts, name, world, 1)
    return parts


# ---- GPU: order ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("world", [2, 3])
def test_rank_order_is_the_original_order(request, world, k):
    """ctg_set in contiguous shards, every rank by two device adds (float64, then uint16): the union equals the oracle's
    table of all contigs in their order, and the same ranks' result through host add_ctgs, which takes the host route."""
    d = request.getfixturevalue(f"world{world}")
    parts = check_device_case(d, world, f"order:{k}")
    assert sum(int(p["ctg_kmers"]) for p in parts) > 0
    host = load(d, world, f"order_host:{k}")
    assert_tables_equal(union(host, k), union(parts, k), f"host route against device route, k={k} world {world}")
    for p, q in zip(parts, host):  # rank by rank too: a k-mer's owner does not depend on the route
        assert len(p["keys"]) == len(q["keys"]) and int(p["ctg_kmers"]) == int(q["ctg_kmers"])
    check_info(host, f"order_host:{k}", world, 0)


# ---- GPU: mixed routes ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_mix_host_and_device_adds(request, world, which):
    """a: rank 0 adds on the host only, rank 1 on the device only, rank 2 (of three) nothing; b: the last rank alone has
    contigs. The route is the device's on every rank, the table the oracle's."""
    check_device_case(request.getfixturevalue(f"world{world}"), world, f"mixed:{which}")


# ---- GPU: edges of pack, expand and scan ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", EDGE_CASES)
@pytest.mark.parametrize("world", [2, 3])
def test_pack_expand_and_scan_edges(request, world, name):
    check_device_case(request.getfixturevalue(f"world{world}"), world, name)


def test_edge_cases_cover_what_they_name():
    """CPU: the per-rank byte counts and the landing offsets of ranks 1 and 2 that EDGES is there for."""
    bytes_seen, lands = set(), set()
    for lists in EDGES.values():
        b = [sum(x) for x in lists]
        bytes_seen |= set(b)
        for off in (b[0], b[0] + b[1]):
            lands.add("odd" if off % 2 else "aligned" if off % 16 == 0 else "even")
    assert {0, 1, 2, 15, 16, 17, 31, 32, 33, 4097} <= bytes_seen and lands == {"odd", "even", "aligned"}
    assert any(all(L < 21 + 2 for L in x) and x for lists in EDGES.values() for x in lists)
    assert any(x and all(L == 0 for L in x) for lists in EDGES.values() for x in lists)
    assert any(not lists[0] and not lists[1] and len(lists[2]) == 1 for lists in EDGES.values())


# ---- GPU: errors on a handle of several ranks ----------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_refused_adds_leave_the_round_as_it_was(request, world):
    """A bad character, decreasing offsets and a NaN depth after each rank's good adds: the single-rank codes, and the
    finish gives the table of the good contigs alone."""
    parts = check_device_case(request.getfixturevalue(f"world{world}"), world, "errors:")
    for p in parts:
        assert p["codes"].tolist() == [EBADCHAR, EINVAL, EINVAL]


def raw_handle(n_ranks, owner):
    L = N.lib()
    cfg = N.MhmkcConfig()
    L.mhmkc_config_init(C.byref(cfg))
    cfg.n_ranks, cfg.rank, cfg.output_owner = n_ranks, 0, owner
    h = C.c_void_p()
    assert L.mhmkc_create(C.byref(h), C.byref(cfg)) == 0
    return L, h


@pytest.mark.gpu
def test_refusals_and_local_adds_without_a_transport():
    """Raw handles without a transport: no call below reaches a collective. MHMKC_OWNER_HASH with two ranks refuses both
    calls before the pointers and the state; MHMKC_OWNER_MINIMIZER checks its arguments as a single rank does and takes a
    good add locally."""
    from mr_ctgs_worker import dev_tensors

    L, h = raw_handle(2, m.MHMKC_OWNER_HASH)
    try:
        assert L.mhmkc_add_ctgs_device(h, None, None, None, N.MHMKC_DEPTH_F64, 1, 1) == EUNSUPPORTED
        assert L.mhmkc_add_ctgs_device(h, None, None, None, 7, 1, 1) == EUNSUPPORTED
        assert L.mhmkc_add_ctgs_from(h, h) == EUNSUPPORTED
    finally:
        L.mhmkc_destroy(h)
    L, h = raw_handle(2, m.MHMKC_OWNER_MINIMIZER)
    try:
        seqs, depths = ["ACGTTGCATTGACCATGACCATTTGACGGATCAGGATC", "TTGACCATGACCATTTGACGGATCAGGATCAAC"], np.array([3, 4], np.uint16)
        bases, offs, d = dev_tensors(seqs, depths, True)
        nc, total = 2, int(offs[-1])
        import torch

        torch.cuda.synchronize()

        def add(bases_, offs_, d_, kind=N.MHMKC_DEPTH_F64):
            torch.cuda.synchronize()
            return L.mhmkc_add_ctgs_device(h, bases_.data_ptr(), offs_.data_ptr(), d_.data_ptr(), kind, nc, total)

        assert L.mhmkc_add_ctgs_device(h, None, None, None, N.MHMKC_DEPTH_F64, 1, 1) == EINVAL
        assert add(bases, offs, d, 7) == EINVAL
        info = N.MhmkcCtgRanksInfo()
        assert L.mhmkc_ctgs_ranks_info(h, C.byref(info)) == 0 and info.n_ctgs_all == 0 and info.device_route == 0
        assert add(bases, offs, d) == 0  # a good add is local
        bad = bases.clone()
        bad[7] = ord("X")
        assert add(bad, offs, d) == EBADCHAR and b"position 7" in L.mhmkc_last_error(h)
        o2 = offs.clone()
        o2[1] = o2[2] + 1
        assert add(bases, o2, d) == EINVAL and b"contig 1" in L.mhmkc_last_error(h)
        d2 = d.clone()
        d2[1] = float("nan")
        assert add(bases, offs, d2) == EINVAL and b"contig 1" in L.mhmkc_last_error(h)
        assert add(bases, offs, d) == 0
        # a multi-rank source without a ranks build keeps its own refusal
        with m.KmerCounter(21) as a:
            assert L.mhmkc_add_ctgs_from(a._h, h) == EUNSUPPORTED
        assert L.mhmkc_add_ctgs_from(h, h) == EUNSUPPORTED
    finally:
        L.mhmkc_destroy(h)


# ---- GPU: the chain ------------------------------------------------------------------------------------------------

def check_chain(out_dir, world, single_chain):
    for k in CHAIN_KS:
        parts = [dict(np.load(Path(out_dir) / f"chain_k{k}_rank{r}.npz")) for r in range(world)]
        exp, n_exp = single_chain[k]
        assert_tables_equal(union(parts, k), exp, f"chain k={k} world {world}")
        assert sum(int(p["n_ctgs"]) for p in parts) == int(parts[0]["n_ctgs_all"]) == n_exp > 0, f"chain k={k}"
        if k != CHAIN_KS[0]:
            prev = [dict(np.load(Path(out_dir) / f"chain_k{CHAIN_KS[CHAIN_KS.index(k) - 1]}_rank{r}.npz")) for r in range(world)]
            for p, q in zip(parts, prev):  # every rank handed over its own part of the round before
                assert int(p["info_device_route"]) == 1 and int(p["info_n_ctgs"]) == int(q["n_ctgs"])
                assert int(p["info_n_ctgs_all"]) == int(q["n_ctgs_all"]) and int(p["ctg_kmers"]) >= 0
            assert sum(int(p["ctg_kmers"]) for p in parts) > 0
            assert sum(int(p["info_bytes_sent"]) for p in parts) == sum(int(p["info_bytes_recv"]) for p in parts) > 0
        else:
            assert all(int(p["info_n_ctgs_all"]) == 0 and int(p["info_device_route"]) == 0 for p in parts)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_chain_21_33_55_stays_on_the_devices(request, world, single_chain):
    """k = 21 -> 33 -> 55 by uutigs_ranks() and add_ctgs_from(prev) on every rank: each round's union table equals the
    single-rank device chain's, and the ranks' contig counts add up to its count."""
    check_chain(request.getfixturevalue(f"world{world}"), world, single_chain)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_over_rccl(rccl2, single_chain):
    for name in RCCL_CASES:
        check_device_case(rccl2, 2, name)
    check_chain(rccl2, 2, single_chain)
