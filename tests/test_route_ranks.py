"""Lookups answered by the rank that owns the key, and every row's de Bruijn links with neighbours on any rank
(mhmkc_lookup_ranks / mhmkc_dbjg_links_ranks, KmerCounter.lookup_ranks / dbjg_links_ranks): get_kmer_target_rank + the rpc
of the reference's traversal (src/dbjg_traversal.cpp:228-236,260-274, src/kcount/kmer_dht.cpp:193-219), collective over the
ranks of a finished MHMKC_OWNER_MINIMIZER counter.

The GPU tests run 2, 3 and 5 ranks (processes sharing the one GPU, exchanging over gloo, and 2 ranks over RCCL). One spawn
per world serves all its cases (module-scoped fixtures); the parent joins the ranks with a deadline and ends them when it
passes. The expected values come from the ranks' own fetched tables, concatenated in rank order as u, which must equal the
oracle's table of all reads: a dict over u and the oracle's owner function (O.target_ranks) give every lookup's answer,
links_ref(u) every link. The CPU test asserts on the oracle's tables alone that the inputs put the cases of the link rules
on different ranks.
"""
from __future__ import annotations

import ctypes as C
import functools
import socket
import time

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
from mhm2_proxy_amd import _native as N
from common import assert_tables_equal, oracle_table
from mr_route_worker import CHUNKS, case_file, size_plan
from mr_uutig_worker import case_reads
from query_lib import COMP, NO_ROW, WHY, expected_lookup, links_ref

NO_RANK = 0xFF
SYNTH = [("synth", k) for k in (21, 33, 63, 77, 99)]
CASES = SYNTH + [("pal", 22), ("pal+", 34), ("tiny1", 21), ("tiny2", 63), ("cyc257", 21), ("hot", 21)]
WORLD5_CASES = [("synth", 21)]
RCCL_CASES = [("synth", 21), ("synth", 63)]
WORLDS = (2, 3)
NEW_SYMBOLS = ["mhmkc_lookup_ranks", "mhmkc_lookup_ranks_device", "mhmkc_dbjg_links_ranks",
               "mhmkc_dbjg_links_ranks_fetch", "mhmkc_dbjg_links_ranks_device", "mhmkc_route_info"]
OWN_ENDS = (WHY.index("dead_own_x"), WHY.index("fork_own"))  # entries that ask nothing


@functools.lru_cache(maxsize=None)
def cpu_case(setname, k):
    """The oracle's table of all reads of a case and its links (computed once, never changed)."""
    b, o = case_reads(setname, k)
    t = oracle_table(b, o, k)
    return (t,) + links_ref(t)


def table_ranks(t, world):
    if not len(t):
        return np.zeros(0, dtype=np.int64)
    return np.asarray(O.target_ranks(np.ascontiguousarray(t.keys[:, :t.k // 32 + 1]), t.k, world)).astype(np.int64)


def asking_ports(t, why, world):
    """Every port that asks for its neighbour (its own extensions are bases): (d, i, the owner of row i, the owner of the
    canonical neighbour, found or not), as arrays."""
    k, nl = t.k, t.k // 32 + 1
    strs = m.keys_to_strings(t.keys, k) if len(t) else []
    ds, rows, nbs = [], [], []
    for d in (0, 1):
        for i in np.flatnonzero(~np.isin(why[d], OWN_ENDS)):
            s = strs[i]
            nb = s[1:] + chr(int(t.right[i])) if d else chr(int(t.left[i])) + s[:-1]
            ds.append(d)
            rows.append(int(i))
            nbs.append(min(nb, nb[::-1].translate(COMP)))
    ds, rows = np.array(ds, dtype=np.int64), np.array(rows, dtype=np.int64)
    if not len(rows):
        return ds, rows, rows.copy(), rows.copy()
    keys = np.array([O.kmer_from_string(s, nl) for s in nbs], dtype=np.uint64).reshape(len(nbs), nl)
    return ds, rows, table_ranks(t, world)[rows], np.asarray(O.target_ranks(keys, k, world)).astype(np.int64)


def cross_counts(t, why, world):
    """Per kind of the link rules, the asking ports whose neighbour's owner is another rank."""
    ds, rows, own, nb_own = asking_ports(t, why, world)
    kinds = why[ds, rows] if len(rows) else np.zeros(0, dtype=np.uint8)
    return {name: int(((kinds == WHY.index(name)) & (own != nb_own)).sum()) for name in WHY}


# ---- CPU


def test_new_symbols_are_exported_and_refuse_a_null_handle():
    L = N.lib()
    for name in NEW_SYMBOLS:
        assert name in N.ABI_SYMBOLS and hasattr(L, name), name
    assert L.mhmkc_lookup_ranks(None, None, 0, 0, None, None, None, None, None) == -1
    assert L.mhmkc_lookup_ranks_device(None, None, 0, 0, None, None, None, None, None) == -1
    assert L.mhmkc_dbjg_links_ranks(None) == -1
    assert L.mhmkc_dbjg_links_ranks_fetch(None, None, None, None) == -1
    assert L.mhmkc_dbjg_links_ranks_device(None, None, None, None) == -1
    assert L.mhmkc_route_info(None, None) == -1
    assert N.MHMKC_NO_RANK == NO_RANK and C.sizeof(N.MhmkcRouteInfo) == 8 * (9 + len(N.ROUTE_STAGES) + 3)


def test_route_info_struct_matches_the_header():
    import shutil
    import subprocess
    import tempfile
    from pathlib import Path

    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    root = Path(__file__).resolve().parents[1]
    lines = ['printf("sizeof %zu\\n", sizeof(mhmkc_route_info_t));']
    lines += [f'printf("{f} %zu\\n", offsetof(mhmkc_route_info_t, {f}));' for f, _ in N.MhmkcRouteInfo._fields_]
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "t.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmkc.h"\nint main(void){' + "".join(lines) +
                       "return 0;}\n")
        exe = Path(d) / "t"
        subprocess.run(["gcc", "-std=c99", f"-I{root / 'include'}", str(src), "-o", str(exe)], check=True)
        got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                           text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(N.MhmkcRouteInfo)
    for f, _ in N.MhmkcRouteInfo._fields_:
        assert int(got[f]) == getattr(N.MhmkcRouteInfo, f).offset, f


def test_inputs_spread_the_cases_over_the_ranks():
    """CPU, the reference alone (the oracle's tables, O.target_ranks, links_ref's WHY): in worlds 2 and 3 every kind of
    the link rules that looks a neighbour up has a port whose neighbour's owner is another rank (dead_missing: the owner
    of the missing canonical neighbour); the longer keys have the common kinds across ranks; the tiny cases leave a rank
    empty in every world; the palindrome cases hold a row that is its own reverse complement."""
    all_kinds = ("ok", "ok_rc", "dead_nb_x", "fork_nb", "conflict", "dead_missing")
    need = {("synth", 21): all_kinds, ("synth", 33): all_kinds, ("synth", 63): all_kinds[:3], ("synth", 99): all_kinds[:3],
            ("synth", 77): all_kinds[:2]}
    for world in WORLDS:
        for (setname, k), kinds in need.items():
            t, _, _, why = cpu_case(setname, k)
            got = cross_counts(t, why, world)
            for kind in kinds:
                assert got[kind] >= 1, f"{setname} k={k} world {world}: no {kind} port across ranks ({got})"
        for setname, k in (("tiny1", 21), ("tiny2", 63)):
            t = cpu_case(setname, k)[0]
            assert len(t) > 0 and len(set(table_ranks(t, world).tolist())) < world, f"{setname} world {world}"
    for setname, k in (("pal", 22), ("pal+", 34)):
        strs = m.keys_to_strings(cpu_case(setname, k)[0].keys, k)
        assert sum(s == s[::-1].translate(COMP) for s in strs) >= 1, setname
    for chunk in CHUNKS:  # the batch sizes of the GPU tests: different numbers of rounds, a batch equal to the chunk
        for world in WORLDS + (5,):
            plans = [size_plan(r, world, chunk) for r in range(world)]
            rounds = [[-(-s // chunk) for s in p] for p in plans]
            assert any(len({r[j] for r in rounds}) > 1 for j in range(len(plans[0])))
            assert any(chunk in [p[j] for p in plans] for j in range(len(plans[0])))
            assert all(p[0] == 0 for p in plans) and [p[1] for p in plans].count(0) == 1


# ---- GPU


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn(fn, world, arg, out_dir, opts, deadline_s=270):
    """The ranks as processes, joined with a deadline: when it passes (a collective the ranks did not all enter), the
    children are ended and the test fails instead of hanging."""
    import torch.multiprocessing as mp

    ctx = mp.spawn(fn, args=(world, free_port(), arg, str(out_dir), opts), nprocs=world, join=False)
    end = time.monotonic() + deadline_s
    try:
        while not ctx.join(timeout=1.0):  # (returns as soon as a rank ends; raises when one failed)
            if time.monotonic() > end:
                raise TimeoutError(f"{world} ranks did not finish within {deadline_s} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()


def load(out_dir, world, setname, k):
    return [dict(np.load(case_file(out_dir, setname, k, r))) for r in range(world)]


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    import mr_route_worker as W

    d = tmp_path_factory.mktemp("route_w2")
    spawn(W.run, 2, CASES, d, {})
    return d


@pytest.fixture(scope="module")
def world3(tmp_path_factory):
    import mr_route_worker as W

    d = tmp_path_factory.mktemp("route_w3")
    spawn(W.run, 3, CASES, d, {})
    return d


@pytest.fixture(scope="module")
def world5(tmp_path_factory):
    import mr_route_worker as W

    d = tmp_path_factory.mktemp("route_w5")
    spawn(W.run, 5, WORLD5_CASES, d, {})
    return d


@pytest.fixture(scope="module")
def rccl2(tmp_path_factory):
    import mr_route_worker as W

    d = tmp_path_factory.mktemp("route_rccl2")
    spawn(W.run, 2, RCCL_CASES, d, {"rccl": True})
    return d


class Union:
    """The ranks' tables in rank order, with what the expected answers need."""

    def __init__(self, parts, k, suffix=""):
        self.k, self.world = k, len(parts)
        f = [np.concatenate([p[name + suffix] for p in parts]) for name in ("keys", "counts", "left", "right")]
        self.t = m.KmerTable(k, *f)
        self.bases = np.concatenate([[0], np.cumsum([len(p["keys" + suffix]) for p in parts])]).astype(np.int64)
        self.index = {self.t.keys[i].tobytes(): i for i in range(len(self.t))}

    def place(self, gi):
        """Union rows -> (rank, row on that rank); NO_ROW -> (NO_RANK, NO_ROW)."""
        gi = np.asarray(gi).astype(np.int64)
        hit = gi != NO_ROW
        rank = np.searchsorted(self.bases, np.where(hit, gi, 0), side="right") - 1
        row = np.where(hit, gi - self.bases[rank], NO_ROW).astype(np.uint32)
        return np.where(hit, rank, NO_RANK).astype(np.uint8), row

    def expect(self, q, canonicalize):
        """The five outputs of lookup_ranks(q)."""
        k, nl = self.k, self.k // 32 + 1
        q = np.array(q, dtype=np.uint64).reshape(-1, self.t.keys.shape[1])
        if not len(q):
            z = np.zeros(0, dtype=np.uint8)
            return z, z.astype(np.uint32), z.astype(np.uint16), z, z
        q[:, nl - 1] &= np.uint64((2**64 - 1) ^ ((1 << (64 - 2 * (k - 32 * (nl - 1)))) - 1))
        q[:, nl:] = 0
        owner = np.asarray(O.target_ranks(np.ascontiguousarray(q[:, :nl]), k, self.world)).astype(np.uint8)
        gi, counts, left, right = expected_lookup(self.t, self.index, q, canonicalize)
        rank, row = self.place(gi)
        assert (rank[gi != NO_ROW] == owner[gi != NO_ROW]).all(), "a row lies on another rank than its owner"
        return owner, row, counts, left, right


def assert_answers(p, name, exp, what):
    for f, e in zip(("ranks", "rows", "counts", "left", "right"), exp):
        g = p[f"{name}_{f}"]
        assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {name}_{f} {g.shape} {g.dtype} vs {e.shape} {e.dtype}"
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what}: {name}_{f} differs at {bad.size} queries, first {bad[0]}: {g[bad[0]]} vs {e[bad[0]]}"


def assert_traffic(parts, prefix, sent_exp, nl, what):
    """queries_local + queries_sent == queries; the sum of sent == the sum of received; bytes == 8 NL per query sent and 8
    per reply; queries_sent == the CPU's count of queries whose owner is another rank."""
    for r, p in enumerate(parts):
        q, loc, sent, recv = (int(p[f"{prefix}_{f}"]) for f in ("queries", "queries_local", "queries_sent", "queries_recv"))
        assert loc + sent == q and sent == sent_exp[r], f"{what} rank {r}: {loc} + {sent} of {q}, expected {sent_exp[r]} sent"
        assert int(p[f"{prefix}_bytes_sent"]) == 8 * nl * sent + 8 * recv, f"{what} rank {r}"
        assert int(p[f"{prefix}_bytes_recv"]) == 8 * nl * recv + 8 * sent, f"{what} rank {r}"
    assert sum(int(p[f"{prefix}_queries_sent"]) for p in parts) == sum(int(p[f"{prefix}_queries_recv"]) for p in parts), what


def check_lookups(parts, setname, k):
    world, nl = len(parts), k // 32 + 1
    what = f"{setname} k={k} world {world}"
    t = cpu_case(setname, k)[0]
    u = Union(parts, k)
    assert_tables_equal(u.t, t, what)
    if setname.startswith("pal"):  # a key that is its own reverse complement: its "reverse complement as given" is a hit
        strs = m.keys_to_strings(u.t.keys, k)
        assert any(s == s[::-1].translate(COMP) for s in strs), what
    for r, p in enumerate(parts):
        w = f"{what} rank {r}"
        assert p["code_before_finish"].tolist() == [-5, -5], w
        # mhmkc_lookup still answers for the local rows only
        exp_local = np.full(len(u.t), NO_ROW, dtype=np.uint32)
        exp_local[u.bases[r]:u.bases[r + 1]] = np.arange(len(p["keys"]), dtype=np.uint32)
        assert (p["local_rows"] == exp_local).all(), w
        exp_a, exp_c = u.expect(p["qa"], False), u.expect(p["qc"], True)
        assert_answers(p, "a", exp_a, w)
        assert_answers(p, "c", exp_c, w)
        if len(u.t):  # hits and misses both occur, and hits on other ranks
            assert (exp_a[1] != NO_ROW).any() and (exp_a[1] == NO_ROW).any(), w
        assert int(p["null_ok"]) == 1 and int(p["tensors_ok"]) == 1, w
        assert_answers(p, "h", u.expect(p["qh"], False), w)
        assert int(p["ih_queries_local"]) == (len(p["qh"]) if r == 0 else 0), w
        assert int(p["ih_queries_recv"]) == ((world - 1) * len(p["qh"]) if r == 0 else 0), w
        assert int(p["ia_rounds"]) == 1 and int(p["ia_entries"]) == int(p["ia_queries"]) == len(p["qa"]), w
    assert_traffic(parts, "ia", [int((u.expect(p["qa"], False)[0] != r).sum()) for r, p in enumerate(parts)], nl, what)
    # batch sizes around the chunk: the rounds are the largest need over the ranks
    for chunk in CHUNKS:
        plans = [size_plan(r, world, chunk) for r in range(world)]
        for j in range(len(plans[0])):
            rounds = max(-(-pl[j] // chunk) for pl in plans)
            for r, p in enumerate(parts):
                name, w = f"s{chunk}_{j}", f"{what} rank {r} chunk {chunk} scenario {j}"
                assert len(p[name + "_q"]) == plans[r][j], w
                assert_answers(p, name, u.expect(p[name + "_q"], bool(j & 1)), w)
                info = p[name + "_info"].tolist()
                assert info[:4] == [rounds, chunk, plans[r][j], plans[r][j]] and info[4] + info[5] == info[3], w
            assert sum(int(p[f"s{chunk}_{j}_info"][5]) for p in parts) == sum(int(p[f"s{chunk}_{j}_info"][6]) for p in parts)


def check_links(parts, setname, k):
    world, nl = len(parts), k // 32 + 1
    what = f"{setname} k={k} world {world}"
    t = cpu_case(setname, k)[0]
    for suffix, prefix in (("", "il"), ("2", "i64")):
        u = Union(parts, k, suffix)
        assert_tables_equal(u.t, t, what)
        nxt, status, why = links_ref(u.t)
        ds, rows, own, nb_own = asking_ports(u.t, why, world)
        for r, p in enumerate(parts):
            w = f"{what} rank {r} {prefix}"
            sl = slice(int(u.bases[r]), int(u.bases[r + 1]))
            exp_rank, exp_row = u.place(nxt[:, sl].reshape(-1))
            n_r = sl.stop - sl.start
            for name, e in (("next_rank", exp_rank), ("next_row", exp_row), ("status", status[:, sl].reshape(-1))):
                g = p[name + ("64" if suffix else "")]
                assert g.shape == (2, n_r) and g.dtype == e.dtype, w
                bad = np.flatnonzero(g.reshape(-1) != e)
                assert bad.size == 0, f"{w}: {name} differs at {bad.size} entries, first {bad[0]}"
            assert int(p[prefix + "_entries"]) == 2 * n_r and int(p[prefix + "_queries"]) == int((own == r).sum()), w
            if suffix:
                assert int(p["i64_chunk"]) == 64, w
                assert int(p["i64_rounds"]) == max(-(-2 * (int(u.bases[q + 1]) - int(u.bases[q])) // 64) for q in range(world)), w
            else:
                assert int(p["il_rounds"]) == (1 if len(u.t) else 0), w
        # the queries sent are the asking ports whose neighbour's owner is another rank
        assert_traffic(parts, prefix, [int(((own == r) & (nb_own != r)).sum()) for r in range(world)], nl, what)
    for r, p in enumerate(parts):
        w = f"{what} rank {r}"
        n_r = len(p["keys"])
        assert int(p["links_again_ok"]) == 1 and int(p["links_device_ok"]) == 1, w
        assert int(p["links1_code_before"]) == int(p["links1_code_after"]) == -7, w
        kept = int(p["il_kept_bytes"])
        assert int(p["bytes1"]) - int(p["bytes0"]) == kept and kept >= 12 * n_r and (kept > 0) == (n_r > 0), w
        assert int(p["bytes2"]) <= int(p["bytes0"]) and (n_r == 0 or int(p["bytes2"]) < int(p["bytes1"])), w
        assert p["code_after_reset"].tolist() == [-5, -5, -5], w


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", CASES)
def test_two_ranks_lookups(world2, setname, k):
    check_lookups(load(world2, 2, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", CASES)
def test_two_ranks_links(world2, setname, k):
    check_links(load(world2, 2, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", CASES)
def test_three_ranks_lookups(world3, setname, k):
    check_lookups(load(world3, 3, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", CASES)
def test_three_ranks_links(world3, setname, k):
    check_links(load(world3, 3, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_five_ranks(world5):
    setname, k = WORLD5_CASES[0]
    parts = load(world5, 5, setname, k)
    check_lookups(parts, setname, k)
    check_links(parts, setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", RCCL_CASES)
def test_two_ranks_over_rccl(rccl2, setname, k):
    parts = load(rccl2, 2, setname, k)
    check_lookups(parts, setname, k)
    check_links(parts, setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_tiny_cases_leave_a_rank_without_rows(world3):
    """A rank with no rows takes part in every round, answers every query with a miss and keeps no links."""
    empty = 0
    for setname, k in (("tiny1", 21), ("tiny2", 63)):
        for p in load(world3, 3, setname, k):
            if len(p["keys"]) == 0:
                empty += 1
                assert p["next_rank"].shape == (2, 0) and int(p["il_kept_bytes"]) == 0 and int(p["il_queries"]) == 0
    assert empty > 0


def raw_handle(n_ranks, owner):
    L = N.lib()
    cfg = N.MhmkcConfig()
    L.mhmkc_config_init(C.byref(cfg))
    cfg.n_ranks, cfg.rank, cfg.output_owner = n_ranks, 0, owner
    h = C.c_void_p()
    assert L.mhmkc_create(C.byref(h), C.byref(cfg)) == 0
    return L, h


@pytest.mark.gpu
def test_refusals_come_before_any_collective():
    """MHMKC_OWNER_HASH with two ranks: MHMKC_EUNSUPPORTED; before finish: MHMKC_ESTATE; in that order, on handles that
    have no transport and no peer, so neither has reached a collective."""
    key = (C.c_uint64 * 1)(0)
    out = (C.c_uint8 * 1)()
    ptrs = [C.c_void_p() for _ in range(3)]
    for owner, code in ((m.MHMKC_OWNER_HASH, -7), (m.MHMKC_OWNER_MINIMIZER, -5)):
        L, h = raw_handle(2, owner)
        try:
            assert L.mhmkc_lookup_ranks(h, key, 1, 0, out, None, None, None, None) == code
            assert L.mhmkc_lookup_ranks(h, None, 0, 0, None, None, None, None, None) == code
            assert L.mhmkc_lookup_ranks_device(h, None, 0, 0, None, None, None, None, None) == code
            assert L.mhmkc_dbjg_links_ranks(h) == code
            assert L.mhmkc_dbjg_links_ranks_fetch(h, None, None, None) == code
            assert L.mhmkc_dbjg_links_ranks_device(h, *[C.byref(p) for p in ptrs]) == code
            assert L.mhmkc_dbjg_links(h, None, None) == -7  # (the single-rank call stays refused)
            info = N.MhmkcRouteInfo()
            assert L.mhmkc_route_info(h, C.byref(info)) == 0 and info.rounds == 0 and info.queries == 0
        finally:
            L.mhmkc_destroy(h)


@pytest.mark.gpu
def test_one_rank_is_the_single_rank_call():
    """n_ranks == 1: lookup_ranks is lookup with rank 0, dbjg_links_ranks is dbjg_links with rank 0 (MHMKC_NO_RANK where
    there is no row); before finish MHMKC_ESTATE; the kept bytes fall back after reset."""
    import torch

    from mr_route_worker import device_array, lookup_batches

    b, o = case_reads("synth", 33)
    c = m.KmerCounter(33)
    try:
        c.add_packed_reads(b, o)
        for call in (c.dbjg_links_ranks, lambda: c.lookup_ranks(np.zeros((1, 2), np.uint64))):
            with pytest.raises(N.MhmkcError) as e:
                call()
            assert e.value.code == -5
        c.finish()
        t = c.fetch()
        qa, qc = lookup_batches(t.keys, 33, 0)
        for q, canon in ((qa, False), (qc, True), (qa[:0], False)):
            got = c.lookup_ranks(q, canonicalize=canon)
            exp = c.lookup(q, canonicalize=canon)
            assert (got[0] == 0).all() and got[0].dtype == np.uint8 and len(got[0]) == len(q)
            assert all((g == e).all() for g, e in zip(got[1:], exp))
        dev = c.lookup_ranks_tensors(torch.from_numpy(qa.view(np.int64)).cuda())
        assert (dev[0].cpu().numpy() == 0).all() and (dev[1].cpu().numpy().view(np.uint32) == c.lookup(qa)[0]).all()
        bytes0 = c.stats()["device_bytes"]
        nxt, status = c.dbjg_links()
        bytes1 = c.stats()["device_bytes"]
        next_rank, next_row, status_r = c.dbjg_links_ranks()
        assert (next_row == nxt).all() and (status_r == status).all()
        assert (next_rank == np.where(nxt == NO_ROW, NO_RANK, 0)).all() and (nxt == NO_ROW).any() and (nxt != NO_ROW).any()
        info = c.route_info()
        assert info["rounds"] == 0 and info["queries_sent"] == 0 and info["entries"] == 2 * len(t)
        assert c.stats()["device_bytes"] - bytes1 >= 2 * len(t) and bytes1 > bytes0
        dv = c.dbjg_links_ranks_device()
        c.synchronize()
        assert (device_array(dv["next_rank"], 2 * len(t), "|u1") == next_rank.reshape(-1)).all()
        assert (device_array(dv["next_row"], 2 * len(t), "<i4").view(np.uint32) == nxt.reshape(-1)).all()
        assert (device_array(dv["status"], 2 * len(t), "|u1") == status.reshape(-1)).all()
        c.reset()
        assert c.stats()["device_bytes"] < bytes1
        with pytest.raises(N.MhmkcError) as e:
            c.dbjg_links_ranks()
        assert e.value.code == -5
    finally:
        c.close()
