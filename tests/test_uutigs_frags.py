"""The uutigs of a table on several ranks, built from rank-local fragments (mhmkc_uutigs_frags / KmerCounter.uutigs_frags,
DESIGN.md §3.12c): the contract of mhmkc_uutigs_ranks reached without a replicated union.

CPU: the decomposition (ufrag_lib.frags_ref + layout_ref, stages 1-2 and 4-6 restated in Python over the oracle's table
with the reference's owner) reproduces uutigs_ref for every case at 2, 3 and 5 ranks; the inputs hold every shape the
build can get wrong; the ABI. GPU: 2, 3 and 5 ranks (processes sharing the one GPU over gloo, and 2 ranks over RCCL)
against uutigs_ref and frags_ref; the kept state; equality with the replicated build; the step to the next k; the codes.
One spawn per world serves all its cases (module-scoped fixtures).
"""
from __future__ import annotations

import ctypes as C
import re
import shutil
import socket
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
from mhm2_proxy_amd import _native as N
from common import assert_tables_equal, oracle_ctg_table
from query_lib import NO_ROW
from ufrag_lib import EXTRA_CASES, case_reads, cpu_case, frags_ref, layout_ref, table_ranks
from uutig_lib import revcomp

ROOT = Path(__file__).resolve().parents[1]
SYNTH = [("synth", k) for k in (21, 33, 63, 99)]
CYCLES = [("circ", 21), ("circ", 22)] + [(f"cyc{n}", 21) for n in (33, 64, 257)] + [("multi", 21)]
TINY = [(f"tiny{rows}", k) for k in (21, 63) for rows in (1, 2)]
PALS = [(f"pal{w}", k) for k in (22, 34) for w in ("", "+")]
TIES = [("otie1", 35), ("tie2", 77), ("otie3", 127)]
CASES = SYNTH + CYCLES + [("hot", 21)] + TINY + PALS + TIES + EXTRA_CASES  # test_uutigs_ranks.py's and the two added
WORLD5_CASES = [("synth", 21)]
RCCL_CASES = [("synth", 21), ("synth", 63), ("cyc257", 21), ("circ23", 21)]
EQUAL_CASES = [("synth", 21), ("multi", 21)]
MOVING = ("claims", "gather", "ids", "bases")

_frags = {}


def cpu_frags(setname, k, world):
    """frags_ref of a case at a world (computed once, never changed)."""
    key = (setname, k, world)
    if key not in _frags:
        t, nxt, status, _ = cpu_case(setname, k)
        _frags[key] = frags_ref(t, nxt, status, table_ranks(t, world), world)
    return _frags[key]


def ranks_of(strs, k, world):
    if not len(strs):
        return np.zeros(0, dtype=np.int64)
    nl = k // 32 + 1
    keys = np.array([O.kmer_from_string(s, nl) for s in strs], dtype=np.uint64).reshape(len(strs), nl)
    return np.asarray(O.target_ranks(keys, k, world)).astype(np.int64)


# ---- CPU


@pytest.mark.parametrize("world", [2, 3, 5])
def test_fragments_laid_out_by_the_stages_give_the_single_rank_uutigs(world):
    """Stages 1-2 (frags_ref) and 4-6 (layout_ref) in Python reproduce uutigs_ref's row map, sequences, rows and depth
    bits for every case: the decomposition and the cycle rotation, without a GPU."""
    for setname, k in CASES:
        t, _, _, ref = cpu_case(setname, k)
        fr = cpu_frags(setname, k, world)
        lay = layout_ref(t, fr)
        what = f"{setname} k={k} world {world}"
        assert lay["seqs"] == ref["seqs"], what
        assert (lay["n_kmers"] == ref["n_kmers"]).all(), what
        assert (lay["depths"].view(np.uint64) == ref["depths"].view(np.uint64)).all(), what
        for name in ("row_ctg", "row_pos", "row_rc"):
            assert (lay[name] == ref[name]).all(), f"{what}: {name}"
        assert [c["key"] for c in fr["contigs"]] == ref["start_keys"], what
        assert [c["cyclic"] for c in fr["contigs"]] == ref["cyclic"].tolist(), what


def cross_cycles(setname, k, world):
    """(rows, fragments, the start fragment's rows, the start row's position in it, reversed fragments) per cross-rank cycle"""
    out = []
    for c in cpu_frags(setname, k, world)["contigs"]:
        if c["cross"] and c["cyclic"]:
            sf = next(f for f, _, _ in c["frags"] if f["start"] == c["start"])
            out.append((c["rows"], len(c["frags"]), sf["m"], sf["lp_start"], sum(x for _, x, _ in c["frags"])))
    return out


def test_inputs_hold_every_shape_the_build_can_get_wrong():
    """Asserted on the oracle's tables with the reference's owner; the worlds named are those where the shape was found.
    (Of the issue's list, cyc257 has its start strictly inside its fragment at 2 ranks but at its fragment's end at 3, and
    circ k = 21 has it strictly inside at 5 ranks, at the end at 2 and 3: the shapes are asserted where they are.)"""
    for world in (2, 3):  # one cycle of 23 rows in exactly two fragments
        assert [(x[0], x[1]) for x in cross_cycles("circ23", 21, world)] == [(23, 2)], world
    inside = [("circ", 21, 5), ("cyc33", 21, 2), ("cyc33", 21, 3), ("cyc64", 21, 2), ("cyc257", 21, 2)]
    for setname, k, world in inside:  # a cross-rank cycle whose start lies strictly inside its fragment
        (_, _, ms, lp, _), = cross_cycles(setname, k, world)
        assert 0 < lp < ms - 1, (setname, k, world, ms, lp)
    at_end = [("circ", 22, 2), ("circ", 22, 3), ("circ", 22, 5), ("cyc257", 21, 3), ("cyc257", 21, 5)]
    for setname, k, world in at_end:  # and one whose start lies at its fragment's end
        (_, _, ms, lp, _), = cross_cycles(setname, k, world)
        assert lp in (0, ms - 1), (setname, k, world, ms, lp)
    for world in (2, 3, 5):
        fr = cpu_frags("synth", 21, world)
        paths = [c for c in fr["contigs"] if c["cross"] and not c["cyclic"]]
        assert any(frc for c in paths for _, frc, _ in c["frags"]), "no fragment reversed in a path"
        assert any(x[4] for x in cross_cycles("cyc257", 21, world)), "no fragment reversed in a cycle"
        assert any(f["m"] == 1 for r in fr["ranks"] for f in r["open"]), "no open fragment of one row"
        assert any(not c["cross"] for c in fr["contigs"]) and paths, "no contig complete on one rank beside cross-rank ones"
        # a cycle wholly on one rank: the tandem repeat's five rows (the other ranks empty), multi's poly-A row
        fr = cpu_frags("tandem", 21, world)
        assert sorted((len(r["closed"]), r["local_cycles"]) for r in fr["ranks"]) == [(0, 0)] * (world - 1) + [(1, 1)]
        assert fr["contigs"][0]["rows"] == 5 and fr["contigs"][0]["cyclic"] and not fr["n_cross"]
        t = cpu_case("tandem", 21)[0]
        assert len(set(table_ranks(t, world).tolist())) == 1 < world
        fr = cpu_frags("multi", 21, world)
        assert sum(r["local_cycles"] for r in fr["ranks"]) == 1 and fr["cycles_cross"] == 4
        assert [c["rows"] for c in fr["contigs"] if c["cyclic"] and not c["cross"]] == [1]
    for setname, k in TINY:  # a rank left empty
        t = cpu_case(setname, k)[0]
        assert all(len(set(table_ranks(t, world).tolist())) < world for world in (2, 3))
    # recorded values of frags_ref: a change of the restated rule shows
    fr = cpu_frags("synth", 21, 2)
    assert sum(len(r["open"]) for r in fr["ranks"]) == 2645 and sum(len(r["closed"]) for r in fr["ranks"]) == 42
    assert sum(1 for r in fr["ranks"] for f in r["open"] if f["m"] == 1) == 368
    assert [r["cross_links"] for r in fr["ranks"]] == [2604, 2604]


def test_abi_declares_and_mirrors_the_fragment_calls(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mhmkc.h").read_text(), flags=re.S)
    for name in ("mhmkc_uutigs_frags", "mhmkc_uutigs_frags_info"):
        assert re.search(rf"\bint {name}\s*\(", text) and name in N.ABI_SYMBOLS, name
    assert "#define MHMKC_ABI_VERSION 14" in text
    for name, value in (("CLAIM_BYTES", N.UFRAG_RECORD_BYTES["claims"]), ("ID_BYTES", N.UFRAG_RECORD_BYTES["ids"]),
                        ("BASE_BYTES", N.UFRAG_RECORD_BYTES["bases"]), ("SCRATCH_ROW", N.UFRAG_SCRATCH_ROW),
                        ("SCRATCH_FRAG", N.UFRAG_SCRATCH_FRAG), ("SCRATCH_CTG", N.UFRAG_SCRATCH_CTG)):
        assert re.search(rf"#define MHMKC_UFRAG_{name} {value}\b", text), name
    assert all(t in (C.c_uint64, C.c_double) or t._type_ in (C.c_uint64, C.c_double) for _, t in N.MhmkcUutigFragsInfo._fields_)
    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    py, cname = N.MhmkcUutigFragsInfo, "mhmkc_uutig_frags_info"
    lines = [f'printf("sizeof %zu\\n", sizeof({cname}));', f'printf("stages %d\\n", (int)MHMKC_UFRAGS_STAGES);',
             'printf("record %d\\n", (int)MHMKC_UFRAG_RECORD_BYTES(2));', 'printf("fixed %d\\n", (int)MHMKC_UFRAG_SCRATCH_FIXED);']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmkc.h"\nint main(void){' + "".join(lines) + "return 0;}\n")
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {line.split()[0]: int(line.split()[1]) for line in out if line}
    assert got["sizeof"] == C.sizeof(py) and got["stages"] == len(N.UFRAGS_STAGES)
    assert got["record"] == N.UFRAG_RECORD_BYTES["gather"] + 16 and got["fixed"] == N.UFRAG_SCRATCH_FIXED
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset, f


def test_abi_version_stays_14():
    from mhm2_proxy_amd import build

    build.build_lib()
    lib = N.lib()
    assert lib.mhmkc_abi_version() == 14 and hasattr(lib, "mhmkc_uutigs_frags") and hasattr(lib, "mhmkc_uutigs_frags_info")


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
    from mr_ufrag_worker import case_file

    return [dict(np.load(case_file(out_dir, setname, k, r))) for r in range(world)]


def spawned(tmp_path_factory, name, world, cases, opts):
    import mr_ufrag_worker as W

    d = tmp_path_factory.mktemp(name)
    spawn(W.run, world, cases, d, opts)
    return d


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    return spawned(tmp_path_factory, "ufrags_w2", 2, CASES, {"hash": True})


@pytest.fixture(scope="module")
def world3(tmp_path_factory):
    return spawned(tmp_path_factory, "ufrags_w3", 3, CASES, {})


@pytest.fixture(scope="module")
def world5(tmp_path_factory):
    return spawned(tmp_path_factory, "ufrags_w5", 5, WORLD5_CASES, {})


@pytest.fixture(scope="module")
def rccl2(tmp_path_factory):
    return spawned(tmp_path_factory, "ufrags_rccl2", 2, RCCL_CASES, {"rccl": True})


@pytest.fixture(scope="module")
def equal2(tmp_path_factory):
    return spawned(tmp_path_factory, "ufrags_eq2", 2, EQUAL_CASES, {"equal": True})


def contig_strings(offsets, seqs):
    blob = seqs.tobytes().decode("ascii")
    return [blob[int(offsets[c]):int(offsets[c + 1])] for c in range(len(offsets) - 1)]


def start_key(seq: str, k: int) -> str:
    return min(min(seq[p:p + k], revcomp(seq[p:p + k])) for p in range(len(seq) - k + 1))


def check_case(parts, setname, k):
    """Everything the contract fixes, for the ranks' results of one case; returns the global contig list."""
    world = len(parts)
    what = f"{setname} k={k} world {world}"
    t, _, _, ref = cpu_case(setname, k)
    fr = cpu_frags(setname, k, world)
    nl = k // 32 + 1
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
        assert int(p["first_id"]) == first and int(p["n_ctgs_all"]) == len(ref["seqs"]), f"{what}: rank {r}"
        first += len(seqs)
        starts = [start_key(s, k) for s in seqs]
        assert all(a < b for a, b in zip(starts, starts[1:])), f"{what}: rank {r} not in start-key order"
        assert (ranks_of(starts, k, world) == r).all(), f"{what}: rank {r} holds a contig whose start is elsewhere"
        glob += list(zip(seqs, p["n_kmers"].tolist(), p["depths"].view(np.uint64).tolist(), starts))
        # the kept build: a second call of either function returns it and runs no collective
        assert int(p["same_again"]) == 1 and int(p["quiet"]) == 1, f"{what}: rank {r}"
        assert int(p["dev_n_ctgs"]) == len(seqs) and int(p["dev_n_bases"]) == len(p["seqs"]), what
        assert int(p["dev_n_out"]) == len(p["keys"]) and int(p["uinfo_n_ctgs"]) == len(seqs), what
        assert int(p["uinfo_n_bases"]) == len(p["seqs"]), what
        assert int(p["info_n_ctgs"]) == len(seqs) and int(p["info_first_id"]) == int(p["first_id"]), what
        assert int(p["info_n_rows"]) == len(p["keys"]) and int(p["info_n_rows_all"]) == len(t), what
        # mhmkc_uutigs_ranks_info after a fragment build: the seven shared fields, the rest zero
        for name in ("n_ctgs", "n_bases", "first_id", "n_ctgs_all", "n_rows", "n_rows_all", "kept_bytes"):
            assert int(p["rinfo_" + name]) == int(p["info_" + name]), f"{what}: ranks info {name}"
        for name in ("rounds", "cycle_rounds", "cycle_ports", "scratch_bytes", "ms_total", "routed_bytes_sent", "ms_stage"):
            assert not np.asarray(p["rinfo_" + name]).any(), f"{what}: ranks info {name}"
        assert p["reset_codes"].tolist() == [-7, -7, -7], what
    assert first == len(ref["seqs"]), what
    merged = sorted(glob, key=lambda x: x[3])
    assert [x[3] for x in merged] == ref["start_keys"], what
    exact = [x[0] for x in merged] == ref["seqs"]
    if k % 2:
        assert exact, what
    else:  # (a start that is its own reverse complement may come out on the other strand, include/mhmkc.h)
        assert [min(x[0], revcomp(x[0])) for x in merged] == [min(s, revcomp(s)) for s in ref["seqs"]], what
    assert [x[1] for x in merged] == ref["n_kmers"].tolist(), what
    assert [x[2] for x in merged] == ref["depths"].view(np.uint64).tolist(), what
    # the reference's contig c (start-key order) has the global id of its place in the rank-major order
    owner_of_ctg = ranks_of(ref["start_keys"], k, world)
    gid_of = np.zeros(len(ref["seqs"]), dtype=np.int64)
    gid_of[np.argsort(owner_of_ctg, kind="stable")] = np.arange(len(gid_of))
    row_of = {t.keys[i, :nl].tobytes(): i for i in range(len(t))}
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
            j = row_of[np.ascontiguousarray(p["keys"][i, :nl]).tobytes()]
            assert g == gid_of[ref["row_ctg"][j]], f"{what}: rank {r} row {i}: global id"
            if exact:
                assert pos == ref["row_pos"][j] and p["row_rc"][i] == ref["row_rc"][j], f"{what}: rank {r} row {i}"
            placed += 1
    assert placed == int(ref["n_kmers"].sum()), what
    # the info: the fragments and contigs are frags_ref's, exactly
    opens_all = sum(len(x["open"]) for x in fr["ranks"])
    mine = np.bincount(ranks_of([c["key"] for c in fr["contigs"] if c["cross"]], k, world), minlength=world)
    for r, p in enumerate(parts):
        exp = fr["ranks"][r]
        got = {name: int(p["info_" + name]) for name in ("frags_open", "frags_open_all", "frags_closed", "local_cycles",
                                                         "cross_links", "ctgs_cross_all", "cycles_cross_all", "ctgs_cross_mine")}
        assert got == {"frags_open": len(exp["open"]), "frags_open_all": opens_all, "frags_closed": len(exp["closed"]),
                       "local_cycles": exp["local_cycles"], "cross_links": exp["cross_links"],
                       "ctgs_cross_all": fr["n_cross"], "cycles_cross_all": fr["cycles_cross"],
                       "ctgs_cross_mine": int(mine[r])}, f"{what}: rank {r}"
        # what a stage moved: its records times the header's bytes per record
        stage = dict(zip(N.UFRAGS_STAGES, range(len(N.UFRAGS_STAGES))))
        for name in N.UFRAGS_STAGES:
            per = N.UFRAG_RECORD_BYTES.get(name, 0) + (8 * nl if name == "gather" else 0)
            for way in ("sent", "recv"):
                rec, byt = int(p[f"info_records_{way}"][stage[name]]), int(p[f"info_bytes_{way}"][stage[name]])
                assert byt == rec * per and (name in MOVING or rec == 0), f"{what}: rank {r} {name} {way}"
        # (a claim that is not mutual cross-links nothing: a row that is its own reverse complement, even k)
        assert int(p["info_records_recv"][stage["claims"]]) >= exp["cross_links"], f"{what}: rank {r}: claims"
        assert k % 2 == 0 or int(p["info_records_sent"][stage["claims"]]) == exp["cross_links"], f"{what}: rank {r}: claims"
        assert int(p["info_records_sent"][stage["gather"]]) == len(exp["open"]) * (world - 1), what
        assert int(p["info_records_recv"][stage["gather"]]) == opens_all - len(exp["open"]), what
        assert (int(p["info_rounds_frags"]) > 0) == (opens_all > 0) and (int(p["info_cycle_rounds_frags"]) > 0) == (fr["cycles_cross"] > 0)
        bound = N.UFRAG_SCRATCH_ROW * len(p["keys"]) + N.UFRAG_SCRATCH_FRAG * opens_all + \
            (k + N.UFRAG_SCRATCH_CTG) * fr["n_cross"] + int(p["n_bases"]) + N.UFRAG_SCRATCH_FIXED + 16 * world * world
        assert 0 < int(p["info_scratch_bytes"]) <= bound and int(p["info_kept_bytes"]) > 0, f"{what}: rank {r}: scratch"
    for name in MOVING:
        x = N.UFRAGS_STAGES.index(name)
        assert sum(int(p["info_bytes_sent"][x]) for p in parts) == sum(int(p["info_bytes_recv"][x]) for p in parts), f"{what}: {name}"
        assert sum(int(p["info_records_sent"][x]) for p in parts) == sum(int(p["info_records_recv"][x]) for p in parts), what
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
def test_ranks_without_rows_take_part(world3):
    """A rank with no rows takes part in every collective and keeps an empty list."""
    empty = 0
    for setname, k in TINY + [("tandem", 21)]:
        for p in load(world3, 3, setname, k):
            if len(p["keys"]) == 0:
                empty += 1
                assert int(p["n_ctgs"]) == 0 and p["offsets"].tolist() == [0] and len(p["row_ctg"]) == 0
                assert int(p["info_frags_open"]) == int(p["info_frags_closed"]) == 0
    assert empty > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("setname,k", EQUAL_CASES)
def test_fragment_build_equals_the_replicated_build(equal2, setname, k):
    """On a second counter over the same shard uutigs_ranks() gives identical fetched arrays, and identical row maps; there a later
    uutigs_frags() returns the kept replicated build, and its info holds the seven shared fields alone."""
    for r, p in enumerate(load(equal2, 2, setname, k)):
        assert int(p["rep_same_ids"]) == 1 and int(p["rep_frags_again"]) == 1, (setname, k, r)
        # (two handles may hold the same rows in another order: the row maps are compared row by row of equal key)
        nl = k // 32 + 1
        oa = np.lexsort([p["keys"][:, w] for w in reversed(range(nl))])
        ob = np.lexsort([p["rep_keys"][:, w] for w in reversed(range(nl))])
        assert (p["keys"][oa] == p["rep_keys"][ob]).all(), (setname, k, r)
        for name in ("offsets", "seqs", "depths", "n_kmers", "row_ctg", "row_pos", "row_rc"):
            a, b = p[name], p["rep_" + name]
            if name.startswith("row_"):
                a, b = a[oa], b[ob]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (setname, k, r, name)
        assert int(p["rep_finfo_n_ctgs"]) == int(p["n_ctgs"]) and int(p["rep_finfo_n_ctgs_all"]) == int(p["n_ctgs_all"])
        assert int(p["rep_finfo_frags_open_all"]) == 0 and int(p["rep_finfo_scratch_bytes"]) == 0
        assert len(p["seqs"]) > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_chain_to_the_next_k_over_two_ranks(tmp_path):
    """k = 21 -> 33 at 2 ranks: uutigs_frags() on the k = 21 counter, add_ctgs_from into the k = 33 counter. The ranks' k = 33
    tables together equal oracle_ctg_table over the reference contigs in rank-major order (the comparison
    test_uutigs_ranks.py justifies: the contig pass does not depend on the order of the contigs)."""
    import mr_ufrag_worker as W

    spawn(W.run_chain, 2, [21, 33], tmp_path, {})
    b, o = case_reads("synth", 21)
    ref = cpu_case("synth", 21)[3]
    d16 = np.minimum(ref["depths"], 65535.0).astype(np.uint16)
    by_rank = np.argsort(ranks_of(ref["start_keys"], 21, 2), kind="stable")
    exp = oracle_ctg_table(b, o, [ref["seqs"][i] for i in by_rank], d16[by_rank], 33)
    parts = [dict(np.load(tmp_path / f"chain_k33_rank{r}.npz")) for r in range(2)]
    u = m.KmerTable(33, np.concatenate([p["keys"] for p in parts]), np.concatenate([p["counts"] for p in parts]),
                    np.concatenate([p["left"] for p in parts]), np.concatenate([p["right"] for p in parts]))
    assert_tables_equal(u, exp, "k=33 after uutigs_frags at k=21")
    assert sum(int(p["n_ctgs"]) for p in parts) == int(parts[0]["n_ctgs_all"]) == len(ref["seqs"]) > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_hash_owner_is_refused_after_finish(world2):
    """A finished MHMKC_OWNER_HASH counter at 2 ranks: MHMKC_EUNSUPPORTED, and no collective has run for it."""
    for r in range(2):
        p = dict(np.load(Path(world2) / f"hash_rank{r}.npz"))
        assert int(p["code"]) == -7 and int(p["quiet"]) == 1 and int(p["n_out"]) >= 0


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
    """MHMKC_OWNER_HASH at 2 ranks: MHMKC_EUNSUPPORTED (after a finish too: test_hash_owner_is_refused_after_finish); the
    minimizer owner before finish: MHMKC_ESTATE; both on handles without a transport, so neither has reached a collective."""
    out = [C.c_uint64() for _ in range(4)]
    L, h = raw_handle(2, m.MHMKC_OWNER_HASH)
    try:
        assert L.mhmkc_uutigs_frags(h, *[C.byref(x) for x in out]) == -7
        assert L.mhmkc_uutigs_frags(h, None, None, None, None) == -7
    finally:
        L.mhmkc_destroy(h)
    L, h = raw_handle(2, m.MHMKC_OWNER_MINIMIZER)
    try:
        assert L.mhmkc_uutigs_frags(h, *[C.byref(x) for x in out]) == -5
        assert L.mhmkc_uutigs(h, None, None) == -7 and L.mhmkc_uutig_rows(h, None, None, None) == -7
        info = N.MhmkcUutigFragsInfo()
        assert L.mhmkc_uutigs_frags_info(h, C.byref(info)) == 0 and info.n_ctgs_all == 0 and info.frags_open_all == 0
    finally:
        L.mhmkc_destroy(h)
    assert L.mhmkc_uutigs_frags(None, None, None, None, None) == -1
    assert L.mhmkc_uutigs_frags_info(None, None) == -1


@pytest.mark.gpu
def test_one_rank_is_mhmkc_uutigs():
    """n_ranks == 1: mhmkc_uutigs's result with first_id 0; before finish MHMKC_ESTATE."""
    b, o = case_reads("multi", 21)
    c = m.KmerCounter(21)
    try:
        c.add_packed_reads(b, o)
        with pytest.raises(N.MhmkcError) as e:
            c.uutigs_frags()
        assert e.value.code == -5
        c.finish()
        r = c.uutigs_frags()
        offsets, seqs, depths, n_kmers = c.uutigs()
        ref = cpu_case("multi", 21)[3]
        assert r == {"n_ctgs": len(depths), "n_bases": len(seqs), "first_id": 0, "n_ctgs_all": len(depths)}
        assert r == c.uutigs_ranks()
        assert contig_strings(offsets, seqs) == ref["seqs"] and (n_kmers == ref["n_kmers"]).all()
        assert (depths.view(np.uint64) == ref["depths"].view(np.uint64)).all()
        info = c.uutigs_frags_info()
        assert info["n_ctgs_all"] == len(depths) and info["n_rows"] == info["n_rows_all"] == len(c.fetch())
        assert sum(info["bytes_sent"].values()) == sum(info["bytes_recv"].values()) == info["frags_open_all"] == 0
    finally:
        c.close()
