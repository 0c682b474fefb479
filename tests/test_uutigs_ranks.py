"""The uutigs of a table that lies on several ranks (mhmkc_uutigs_ranks / KmerCounter.uutigs_ranks): traverse_debruijn_graph
at rank_n() > 1 (src/dbjg_traversal.cpp:291-335,517-567,569-596), collective over the ranks of a finished
MHMKC_OWNER_MINIMIZER counter.

The result is defined independently of the number of ranks: a contig is what mhmkc_uutigs gives for the union table at one
rank; it belongs to the rank that holds its start row; a rank's contigs are in start-key order; the global id is the prefix
over the lower ranks plus the local index. The GPU tests run 2, 3 and 5 ranks (processes sharing the one GPU, exchanging
over gloo, and 2 ranks over RCCL) on the small sets of tests/test_uutigs.py and compare with links_ref / uutigs_ref over the
oracle's table of all reads. One spawn per world serves all its cases (module-scoped fixtures). The CPU test asserts on the
oracle's tables that the inputs put on different ranks what the collective has to join.
"""
from __future__ import annotations

import ctypes as C
import functools
import socket

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
from mhm2_proxy_amd import _native as N
from common import assert_tables_equal, oracle_ctg_table, oracle_table
from mr_uutig_worker import case_file, case_reads
from query_lib import NO_ROW, links_ref
from uutig_lib import revcomp, uutigs_ref

SYNTH = [("synth", k) for k in (21, 33, 63, 99)]
CYCLES = [("circ", 21), ("circ", 22)] + [(f"cyc{n}", 21) for n in (33, 64, 257)] + [("multi", 21)]
TINY = [(f"tiny{rows}", k) for k in (21, 63) for rows in (1, 2)]
PALS = [(f"pal{w}", k) for k in (22, 34) for w in ("", "+")]
TIES = [("otie1", 35), ("tie2", 77), ("otie3", 127)]
CASES = SYNTH + CYCLES + [("hot", 21)] + TINY + PALS + TIES
WORLD5_CASES = [("synth", 21)]
RCCL_CASES = [("synth", 21), ("synth", 63), ("cyc257", 21)]
WORLDS = (2, 3)


@functools.lru_cache(maxsize=None)
def cpu_case(setname, k):
    """The oracle's table of all reads of a case, its links and the restated uutigs (computed once, never changed)."""
    b, o = case_reads(setname, k)
    t = oracle_table(b, o, k)
    nxt, status, _ = links_ref(t)
    return t, nxt, status, uutigs_ref(t, nxt, status)


def key_array(strs, k):
    nl = k // 32 + 1
    return np.array([O.kmer_from_string(s, nl) for s in strs], dtype=np.uint64).reshape(len(strs), nl)


def ranks_of(strs, k, world):
    """get_kmer_target_rank of k-mers given as strings."""
    if not len(strs):
        return np.zeros(0, dtype=np.int64)
    return np.asarray(O.target_ranks(key_array(strs, k), k, world)).astype(np.int64)


def table_ranks(t, world):
    return np.asarray(O.target_ranks(np.ascontiguousarray(t.keys[:, :t.k // 32 + 1]), t.k, world)).astype(np.int64)


# ---- CPU: the inputs put apart what the collective has to join


def test_inputs_spread_their_structures_over_the_ranks():
    """CPU, on the oracle's tables with the reference's owner (O.target_ranks) for the worlds used: every cycle has rows on
    at least two ranks; a tie case has its tied candidates on different ranks; a row that is its own reverse complement
    has a neighbour on another rank; a contig has rows on another rank than its start's; a tiny case leaves a rank empty;
    and the contig pass of the next k does not depend on the order of the k = 21 uutigs (start order against the
    rank-major order the ranks add them in)."""
    for world in WORLDS:
        for setname, k in CYCLES:
            t, _, _, ref = cpu_case(setname, k)
            owner = table_ranks(t, world)
            for c in np.flatnonzero(ref["cyclic"]):
                rows = np.flatnonzero(ref["row_ctg"] == c)
                if len(rows) > 1:
                    assert len(set(owner[rows].tolist())) >= 2, f"{setname} k={k} world {world}: cycle {c} on one rank"
    tied_apart = selfrc_apart = foreign_rows = empty_rank = 0
    for world in WORLDS:
        for setname, k in TIES:
            t, _, _, ref = cpu_case(setname, k)
            strs = sorted(m.keys_to_strings(t.keys, k))
            tied = ref["start_keys"] if setname.startswith("otie") else strs[:2]
            tied_apart += len(set(ranks_of(tied, k, world).tolist())) >= 2
        for setname, k in PALS:
            t, nxt, status, _ = cpu_case(setname, k)
            strs = m.keys_to_strings(t.keys, k)
            owner = table_ranks(t, world)
            for i in (i for i, s in enumerate(strs) if s == revcomp(s)):
                nb = [int(nxt[d, i]) for d in (0, 1) if int(nxt[d, i]) != NO_ROW]
                selfrc_apart += any(owner[j] != owner[i] for j in nb)
        t, _, _, ref = cpu_case("synth", 21)
        owner = table_ranks(t, world)
        start_owner = ranks_of(ref["start_keys"], 21, world)
        in_ctg = np.flatnonzero(ref["row_ctg"] != NO_ROW)
        foreign_rows += int((owner[in_ctg] != start_owner[ref["row_ctg"][in_ctg]]).sum())
        for setname, k in TINY:
            t = cpu_case(setname, k)[0]
            empty_rank += len(set(table_ranks(t, world).tolist())) < world
    assert tied_apart and selfrc_apart and foreign_rows and empty_rank, (tied_apart, selfrc_apart, foreign_rows, empty_rank)
    # the chain: the contig pass gives one table for the contigs in start order and in rank-major order
    b, o = case_reads("synth", 21)
    ref = cpu_case("synth", 21)[3]
    d16 = np.minimum(ref["depths"], 65535.0).astype(np.uint16)
    by_rank = np.argsort(ranks_of(ref["start_keys"], 21, 2), kind="stable")
    assert (by_rank != np.arange(len(by_rank))).any()
    a = oracle_ctg_table(b, o, ref["seqs"], d16, 33)
    z = oracle_ctg_table(b, o, [ref["seqs"][i] for i in by_rank], d16[by_rank], 33)
    assert_tables_equal(a, z, "k=33 after the k=21 uutigs in start order and in rank-major order")


# ---- GPU


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn(fn, world, arg, out_dir, opts):
    import torch.multiprocessing as mp

    mp.spawn(fn, args=(world, free_port(), arg, str(out_dir), opts), nprocs=world, join=True)


def load(out_dir, world, setname, k):
    return [dict(np.load(case_file(out_dir, setname, k, r))) for r in range(world)]


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    import mr_uutig_worker as W

    d = tmp_path_factory.mktemp("uranks_w2")
    spawn(W.run, 2, CASES, d, {})
    return d


@pytest.fixture(scope="module")
def world3(tmp_path_factory):
    import mr_uutig_worker as W

    d = tmp_path_factory.mktemp("uranks_w3")
    spawn(W.run, 3, CASES, d, {})
    return d


@pytest.fixture(scope="module")
def world5(tmp_path_factory):
    import mr_uutig_worker as W

    d = tmp_path_factory.mktemp("uranks_w5")
    spawn(W.run, 5, WORLD5_CASES, d, {})
    return d


@pytest.fixture(scope="module")
def rccl2(tmp_path_factory):
    import mr_uutig_worker as W

    d = tmp_path_factory.mktemp("uranks_rccl2")
    spawn(W.run, 2, RCCL_CASES, d, {"rccl": True})
    return d


def contig_strings(offsets, seqs):
    blob = seqs.tobytes().decode("ascii")
    return [blob[int(offsets[c]):int(offsets[c + 1])] for c in range(len(offsets) - 1)]


def start_key(seq: str, k: int) -> str:
    """The smallest canonical k-mer of a contig (string order is Kmer::operator< order)."""
    return min(min(seq[p:p + k], revcomp(seq[p:p + k])) for p in range(len(seq) - k + 1))


def check_case(parts, setname, k):
    """Everything the contract fixes, for the ranks' results of one case; returns the global contig list."""
    world = len(parts)
    what = f"{setname} k={k} world {world}"
    t, _, _, ref = cpu_case(setname, k)
    # the union of the ranks' tables is the oracle's table
    u = m.KmerTable(k, np.concatenate([p["keys"] for p in parts]), np.concatenate([p["counts"] for p in parts]),
                    np.concatenate([p["left"] for p in parts]), np.concatenate([p["right"] for p in parts]))
    assert_tables_equal(u, t, what)
    glob, first = [], 0  # (sequence, n_kmers, depth bits, start key) by global id
    for r, p in enumerate(parts):
        seqs = contig_strings(p["offsets"], p["seqs"])
        assert p["offsets"].dtype == np.uint64 and p["n_kmers"].dtype == np.uint32 and p["depths"].dtype == np.float64
        assert len(seqs) == len(p["depths"]) == len(p["n_kmers"]) == int(p["n_ctgs"]), what
        assert int(p["n_bases"]) == len(p["seqs"]) == int(p["offsets"][-1]), what
        assert [len(s) for s in seqs] == [int(x) + k - 1 for x in p["n_kmers"]], what
        # first_id is the prefix of the lower ranks' counts, n_ctgs_all the total
        assert int(p["first_id"]) == first and int(p["n_ctgs_all"]) == len(ref["seqs"]), f"{what}: rank {r}"
        first += len(seqs)
        starts = [start_key(s, k) for s in seqs]
        # each rank's own list is in start-key order, and every contig is on the target rank of its start
        assert all(a < b for a, b in zip(starts, starts[1:])), f"{what}: rank {r} not in start-key order"
        assert (ranks_of(starts, k, world) == r).all(), f"{what}: rank {r} holds a contig whose start is elsewhere"
        glob += list(zip(seqs, p["n_kmers"].tolist(), p["depths"].view(np.uint64).tolist(), starts))
        # the kept build answers the other getters too, and is built once
        assert int(p["same_again"]) == 1 and int(p["dev_n_ctgs"]) == len(seqs) and int(p["dev_n_bases"]) == len(p["seqs"])
        assert int(p["dev_n_out"]) == len(p["keys"]) and int(p["uinfo_n_ctgs"]) == len(seqs), what
        assert int(p["info_n_ctgs"]) == len(seqs) and int(p["info_first_id"]) == int(p["first_id"]), what
        assert int(p["info_n_rows"]) == len(p["keys"]) and int(p["info_n_rows_all"]) == len(t), what
        # after reset the getters refuse the multi-rank handle again
        assert p["reset_codes"].tolist() == [-7, -7, -7], what
    assert first == len(ref["seqs"]), what
    # the ranks' contigs, concatenated in rank order and sorted by start key, are the single-rank list
    merged = sorted(glob, key=lambda x: x[3])
    assert [x[3] for x in merged] == ref["start_keys"], what
    if k % 2:
        assert [x[0] for x in merged] == ref["seqs"], what
    else:  # (a start that is its own reverse complement may come out on the other strand, include/mhmkc.h)
        assert [min(x[0], revcomp(x[0])) for x in merged] == [min(s, revcomp(s)) for s in ref["seqs"]], what
    assert [x[1] for x in merged] == ref["n_kmers"].tolist(), what
    assert [x[2] for x in merged] == ref["depths"].view(np.uint64).tolist(), what
    # every row lies where its row map says, in the contig its global id names, on whichever rank that contig is
    placed = 0
    for r, p in enumerate(parts):
        strs = m.keys_to_strings(p["keys"], k) if len(p["keys"]) else []
        walkable = np.isin(p["left"].view(np.uint8), np.frombuffer(b"ACGT", np.uint8)) & \
            np.isin(p["right"].view(np.uint8), np.frombuffer(b"ACGT", np.uint8))
        assert len(p["row_ctg"]) == len(p["row_pos"]) == len(p["row_rc"]) == len(strs), what
        assert ((p["row_ctg"] != NO_ROW) == walkable).all(), f"{what}: rank {r}: a row with an X or F has a contig, or a walkable row none"
        for i in np.flatnonzero(walkable):
            g, pos = int(p["row_ctg"][i]), int(p["row_pos"][i])
            assert g < len(glob), f"{what}: rank {r} row {i}"
            assert glob[g][0][pos:pos + k] == (revcomp(strs[i]) if p["row_rc"][i] else strs[i]), f"{what}: rank {r} row {i}"
            placed += 1
    assert placed == int(ref["n_kmers"].sum()), what
    # info: what left the ranks arrived, and the cycle ports are two per cycle row of the union
    sent = sum(int(p["info_routed_bytes_sent"].sum()) for p in parts)
    recv = sum(int(p["info_routed_bytes_recv"].sum()) for p in parts)
    assert sent == recv and (sent > 0) == (len(t) > 0), what
    assert sum(int(p["info_routed_records_sent"].sum()) for p in parts) == \
        sum(int(p["info_routed_records_recv"].sum()) for p in parts) == (world - 1) * len(t), what
    on_cycles = int(ref["n_kmers"][ref["cyclic"]].sum())
    for p in parts:
        assert int(p["info_cycle_ports"]) == 2 * on_cycles, what
        assert (int(p["info_cycle_rounds"]) > 0) == (on_cycles > 0) and int(p["info_rounds"]) >= 1, what
        assert int(p["info_kept_bytes"]) > 0 and int(p["info_scratch_bytes"]) >= 128 * len(t), what
    return [(x[0] if k % 2 else min(x[0], revcomp(x[0])), x[1], x[2]) for x in merged]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", CASES)
def test_two_ranks_equal_the_restated_rule(world2, setname, k):
    check_case(load(world2, 2, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", CASES)
def test_three_ranks_equal_the_restated_rule(world3, setname, k):
    check_case(load(world3, 3, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_three_and_five_ranks_give_the_same_list(world2, world3, world5):
    setname, k = WORLD5_CASES[0]
    lists = [check_case(load(d, w, setname, k), setname, k) for d, w in ((world2, 2), (world3, 3), (world5, 5))]
    assert lists[0] == lists[1] == lists[2] and len(lists[0]) > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", RCCL_CASES)
def test_two_ranks_over_rccl(rccl2, setname, k):
    check_case(load(rccl2, 2, setname, k), setname, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_tiny_cases_leave_a_rank_without_rows(world3):
    """A rank with no rows takes part in every collective and keeps an empty list."""
    empty = 0
    for setname, k in TINY:
        for p in load(world3, 3, setname, k):
            if len(p["keys"]) == 0:
                empty += 1
                assert int(p["n_ctgs"]) == 0 and p["offsets"].tolist() == [0] and len(p["row_ctg"]) == 0
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
    """MHMKC_OWNER_HASH: MHMKC_EUNSUPPORTED; before finish: MHMKC_ESTATE; both on a handle that has no transport, so
    neither has reached a collective. Without a build the getters stay MHMKC_EUNSUPPORTED."""
    out = [C.c_uint64() for _ in range(4)]
    L, h = raw_handle(2, m.MHMKC_OWNER_HASH)
    try:
        assert L.mhmkc_uutigs_ranks(h, *[C.byref(x) for x in out]) == -7
    finally:
        L.mhmkc_destroy(h)
    L, h = raw_handle(2, m.MHMKC_OWNER_MINIMIZER)
    try:
        assert L.mhmkc_uutigs_ranks(h, *[C.byref(x) for x in out]) == -5
        assert L.mhmkc_uutigs_ranks(h, None, None, None, None) == -5
        assert L.mhmkc_uutigs(h, None, None) == -7 and L.mhmkc_uutig_rows(h, None, None, None) == -7
        info = N.MhmkcUutigRanksInfo()
        assert L.mhmkc_uutigs_ranks_info(h, C.byref(info)) == 0 and info.n_ctgs_all == 0
    finally:
        L.mhmkc_destroy(h)
    assert L.mhmkc_uutigs_ranks(None, None, None, None, None) == -1
    assert L.mhmkc_uutigs_ranks_info(None, None) == -1


@pytest.mark.gpu
def test_one_rank_is_mhmkc_uutigs():
    """n_ranks == 1: mhmkc_uutigs's result with first_id 0 (whatever the owner); before finish MHMKC_ESTATE."""
    b, o = case_reads("multi", 21)
    c = m.KmerCounter(21)
    try:
        c.add_packed_reads(b, o)
        with pytest.raises(N.MhmkcError) as e:
            c.uutigs_ranks()
        assert e.value.code == -5
        c.finish()
        r = c.uutigs_ranks()
        offsets, seqs, depths, n_kmers = c.uutigs()
        ref = cpu_case("multi", 21)[3]
        assert r == {"n_ctgs": len(depths), "n_bases": len(seqs), "first_id": 0, "n_ctgs_all": len(depths)}
        assert contig_strings(offsets, seqs) == ref["seqs"] and (n_kmers == ref["n_kmers"]).all()
        info = c.uutigs_ranks_info()
        assert info["cycle_ports"] == 2 * int(ref["n_kmers"][ref["cyclic"]].sum()) and info["n_ctgs_all"] == len(depths)
        assert sum(info["routed_bytes_sent"].values()) == sum(info["routed_bytes_recv"].values()) == 0
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_multik_chain_over_two_ranks(tmp_path):
    """k = 21 -> 33 -> 55 on two ranks, each rank passing its own uutig_strings() to the next counter's add_ctgs: every
    round's union table equals the single-rank device chain's (add_ctgs_from). This rests on the contig pass not depending
    on the order of the contigs (the uutigs of one table share no k'-mer for k' > k; the CPU test above pins it)."""
    import mr_uutig_worker as W

    ks = [21, 33, 55]
    spawn(W.run_chain, 2, ks, tmp_path, {})
    b, o = case_reads("synth", 21)
    prev = None
    for k in ks:
        c = m.KmerCounter(k)
        c.add_packed_reads(b, o)
        if prev is not None:
            c.add_ctgs_from(prev)
            prev.close()
        c.finish()
        exp = c.fetch()
        n_exp = len(c.uutigs()[2])
        prev = c
        parts = [dict(np.load(tmp_path / f"chain_k{k}_rank{r}.npz")) for r in range(2)]
        u = m.KmerTable(k, np.concatenate([p["keys"] for p in parts]), np.concatenate([p["counts"] for p in parts]),
                        np.concatenate([p["left"] for p in parts]), np.concatenate([p["right"] for p in parts]))
        assert_tables_equal(u, exp, f"chain k={k}")
        assert sum(int(p["n_ctgs"]) for p in parts) == int(parts[0]["n_ctgs_all"]) == n_exp > 0, f"chain k={k}"
    prev.close()
