"""The supermer exchange (MHMKC_OWNER_MINIMIZER, several ranks, keys of two or more words) at its tile,
word, flank and rank edges: the cases of tests/supermer_cases.py through k_smer_owner, k_smer_pack, the host's splice of
the received spans and k_smer_extract, against the oracle's table and the plain reference of supermer formation.
One process group per (k, world) runs every case (tests/mr_smer_worker.py)."""
import socket

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
import supermer_cases as S
from common import assert_tables_equal, oracle_table

pytestmark = pytest.mark.gpu


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_cases(k, world, tmp_path, names, env=None):
    """{case: [rank's saved table and stats]} of one spawn over the named cases."""
    import torch.multiprocessing as mp

    import mr_smer_worker

    cases = []
    for name in names:
        batches, _ = S.built(name, k, world)
        case = S.CASES.get(name) or S.EXTRA_CASES[name]
        arrays = {}
        for r, bl in batches.items():
            for i, (b, o, _) in enumerate(bl):
                arrays[f"r{r}_b{i}_bytes"], arrays[f"r{r}_b{i}_offs"] = b, np.asarray(o, dtype=np.uint64)
        np.savez(tmp_path / f"in_{name}.npz", **arrays)
        cases.append({"name": name, "kinds": {r: [kind for _, _, kind in bl] for r, bl in batches.items()},
                      "env": dict(env or {}), "env_by_rank": case.env_by_rank})
    mp.spawn(mr_smer_worker.run, args=(world, free_port(), k, str(tmp_path), cases), nprocs=world, join=True)
    return {name: [dict(np.load(tmp_path / f"{name}_rank{r}.npz")) for r in range(world)] for name in names}


def check_case(name, k, world, parts):
    """The six checks of one case; returns the oracle's table of all its reads."""
    batches, refs = S.built(name, k, world)
    case = S.CASES.get(name) or S.EXTRA_CASES[name]
    what = f"{name}, k={k}, {world} ranks"
    st = [{key[3:]: int(v) for key, v in p.items() if key.startswith("st_")} for p in parts]
    # 1. the union of the ranks' tables is the oracle's table of all the case's reads
    exp = oracle_table(*S.all_reads(batches), k)
    u = m.KmerTable(k, *(np.concatenate([p[f] for p in parts]) for f in ("keys", "counts", "left", "right")))
    assert_tables_equal(u, exp, what)
    # 2. disjoint key sets
    assert len({tuple(r) for r in u.keys.tolist()}) == len(u.keys), f"{what}: the ranks' key sets overlap"
    # 3. every row on its target rank
    nl = S.n_longs(k)
    for r, p in enumerate(parts):
        if len(p["keys"]):
            own = O.target_ranks(np.ascontiguousarray(p["keys"][:, :nl]), k, world)
            assert (own == r).all(), f"{what}: rank {r} holds {(own != r).sum()} rows of other ranks"
    # 4. no hand-off, bytes and records conserved
    assert all(s["handoff_sent"] == 0 for s in st), f"{what}: hand-off records sent"
    assert sum(s["bytes_sent"] for s in st) == sum(s["bytes_recv"] for s in st), what
    assert sum(s["owned_records"] for s in st) == sum(s["occurrences"] for s in st), what
    # 5. every rank received exactly the windows the reference gives it; a rank that owns none has an empty table
    tot = S.rank_totals(refs, world)
    for r in range(world):
        assert st[r]["occurrences"] == tot[r]["windows"], f"{what}: rank {r} counted {st[r]['occurrences']} windows"
        assert st[r]["owned_records"] == tot[r]["owned"], \
            f"{what}: rank {r} owns {st[r]['owned_records']} records, the reference gives it {tot[r]['owned']}"
        if tot[r]["owned"] == 0:
            assert len(parts[r]["keys"]) == 0, f"{what}: rank {r} owns no window but returns rows"
    # 6. supermers: at least the maximal runs whatever the tile size; on single-slab batches exactly the runs cut at
    #    the tile edges and their words
    T = S.tile_of(k)
    for r in range(world):
        assert st[r]["smer_count"] >= tot[r]["runs"], \
            f"{what}: rank {r} made {st[r]['smer_count']} supermers, fewer than its {tot[r]['runs']} maximal runs"
        if r in case.multi_slab_ranks:
            continue
        got, want = (st[r]["smer_count"], st[r]["smer_words"]), (tot[r]["cut"], tot[r]["words"])
        assert got == want, (f"{what}: rank {r} made (supermers, words) {got}, the reference cut at {T} windows gives "
                             f"{want}; every other check passed, so compare supermer_cases.TILE with TILE_BASES in "
                             f"kcount_launch.hpp")
    return exp, st


def check_all(k, world, results):
    failures = []
    for name, parts in results.items():
        try:
            check_case(name, k, world, parts)
        except AssertionError as e:
            failures.append(f"[{name}] {e}")
    assert not failures, f"{len(failures)} of {len(results)} cases failed:\n" + "\n".join(failures)


@pytest.mark.parametrize("k,world", [(33, 3), (63, 2), (65, 2), (95, 3), (97, 2), (127, 4)])
def test_supermer_edges(k, world, tmp_path):
    """Every case of supermer_cases.CASES at one and 31 bases in the last key word for 2, 3 and 4 words (k = 127 takes
    the supermer path nowhere else): the union of the ranks' tables equals the oracle's, the key sets are disjoint and on
    their target ranks, nothing is handed off, every rank receives exactly the windows the reference gives it, and the
    supermers and words sent are the reference's runs cut at the tile edges."""
    check_all(k, world, run_cases(k, world, tmp_path, list(S.CASES)))


@pytest.mark.parametrize("k,world", [(63, 2), (97, 2)])
def test_tile_straddle_in_three_passes(k, world, tmp_path):
    """tile_straddle with MHMKC_PASSES=3: every finish pass extracts the received supermers again and keeps its coarse
    bins only (the bin_lo / bin_hi filter of k_smer_extract), over runs of a whole tile."""
    res = run_cases(k, world, tmp_path, ["tile_straddle"], env={"MHMKC_PASSES": "3"})
    _, st = check_case("tile_straddle", k, world, res["tile_straddle"])
    assert [s["finish_passes"] for s in st] == [3] * world


@pytest.mark.parametrize("k,world", [(63, 2), (99, 2)])
def test_hot_owner(k, world, tmp_path):
    """common.hot_set() dealt to the ranks (at k = 99 with 1400 poly-A reads instead of 800, so that the poly-A k-mer
    passes 65535 there too: supermer_cases.hot_owner): its windows all arrive on its owner, in one coarse bucket of the
    received slab. The capped extraction of smer_records gives each of the bucket's 8 segments
    the expected share of the slab's windows + 4 % + 1024 records (mhmkc::extract: a few thousand records here), far
    below the hot k-mer's tens of thousands, so the default caps overflow and no knob is set: the slab is extracted
    again with exact sizes inside smer_records (exact_reruns >= 1 on that rank), and the union still equals the oracle,
    whose table holds the saturated count 65535."""
    res = run_cases(k, world, tmp_path, ["hot_owner"])
    exp, st = check_case("hot_owner", k, world, res["hot_owner"])
    assert (exp.counts == 65535).any()
    hot = O.kmer_from_string("A" * k, S.n_longs(k))  # poly-A: the canonical form of poly-A / poly-T
    owner = int(O.target_ranks(hot[None, :], k, world)[0])
    assert st[owner]["exact_reruns"] >= 1, f"rank {owner} owns the poly-A k-mer: {[s['exact_reruns'] for s in st]}"
