"""Assembly statistics and the one FASTA file of several ranks (mhmkc_uutigs_stats, mhmkc_uutigs_fasta, mhmkc_fasta_write
and the generic calls on multi-rank handles): 2 and 3 ranks as processes sharing the GPU over gloo, 2 ranks over RCCL. One
spawn per world serves all its cases (module-scoped fixtures); the single-rank list is the restated rule's (uutigs_ref on
the oracle's table), computed once per case."""
from __future__ import annotations

import json
import socket
import struct

import numpy as np
import pytest

import fasta_cases as F
from ufrag_lib import cpu_case

pytestmark = pytest.mark.gpu

CASES = [("synth", 21), ("synth", 63), ("tandem", 21)]
RCCL_CASES = [("synth", 21)]
EINVAL, ESTATE, EUNSUPPORTED, ETRANSPORT, EIO = -1, -5, -7, -8, -9
INT_FIELDS = ("n_ctgs", "tot_len", "max_len", "n_ns", "len_sums", "n50", "l50")


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawned(tmp_path_factory, name, world, cases, opts):
    import torch.multiprocessing as mp

    import mr_fasta_worker as W

    d = tmp_path_factory.mktemp(name)
    mp.spawn(W.run, args=(world, free_port(), cases, str(d), opts), nprocs=world, join=True)
    return d


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    return spawned(tmp_path_factory, "fasta_w2", 2, CASES, {"generic": True})


@pytest.fixture(scope="module")
def world3(tmp_path_factory):
    return spawned(tmp_path_factory, "fasta_w3", 3, CASES, {"generic": True})


@pytest.fixture(scope="module")
def rccl2(tmp_path_factory):
    return spawned(tmp_path_factory, "fasta_rccl2", 2, RCCL_CASES, {"rccl": True, "generic": True})


def load(out_dir, world, setname, k):
    from mr_fasta_worker import case_file

    parts = []
    for r in range(world):
        p = dict(np.load(case_file(out_dir, setname, k, r)))
        p["results"] = json.loads(str(p["results"]))
        parts.append(p)
    return parts


def contigs_of(p):
    blob = p["seqs"].tobytes()
    return tuple(blob[int(p["offsets"][c]):int(p["offsets"][c + 1])] for c in range(len(p["depths"]))), tuple(p["depths"].tolist())


def records(text: bytes):
    lines = text.split(b"\n")[:-1]
    return [(h.split()[0], h.split()[1], s) for h, s in zip(lines[0::2], lines[1::2])]


def check_case(out_dir, world, setname, k):
    from mr_fasta_worker import fasta_file, min_lens

    what = f"{setname} k={k} world {world}"
    parts = load(out_dir, world, setname, k)
    ref = cpu_case(setname, k)[3]
    one_seqs, one_depths = tuple(s.encode() for s in ref["seqs"]), tuple(ref["depths"].tolist())
    assert sum(len(p["depths"]) for p in parts) == len(one_seqs) == int(parts[0]["n_ctgs_all"]), what
    for p in parts:  # before the ranks build: refused, and no collective ran
        assert p["early"].tolist() == [EUNSUPPORTED, EUNSUPPORTED] and int(p["quiet"]) == 1, what
    for mn in min_lens(k):
        exp_all = F.stats_ref(one_seqs, one_depths, mn)
        texts, off, depth_sum = [], 0, 0.0
        for r, p in enumerate(parts):
            seqs, depths = contigs_of(p)
            res = p["results"]
            mine, allr, fa = res[f"stats{mn}"]["mine"], res[f"stats{mn}"]["all"], res[f"fasta{mn}"]
            exp_mine = F.stats_ref(seqs, depths, mn)
            kept = [d for s, d in zip(seqs, depths) if len(s) >= mn]
            print(f"{what} min_len={mn} rank {r}: mine n_ctgs={mine['n_ctgs']} tot_depth={mine['tot_depth']!r} "
                  f"fsum={exp_mine['tot_depth']!r}; all tot_depth={allr['tot_depth']!r} fsum={exp_all['tot_depth']!r}")
            for f in INT_FIELDS:
                assert mine[f] == exp_mine[f], f"{what} min_len={mn} rank {r}: mine.{f}"
                assert allr[f] == exp_all[f], f"{what} min_len={mn} rank {r}: all.{f}"
            assert abs(mine["tot_depth"] - exp_mine["tot_depth"]) <= F.depth_bound(kept), what
            assert allr == parts[0]["results"][f"stats{mn}"]["all"], f"{what}: all differs between ranks"
            depth_sum += mine["tot_depth"]
            text = F.fasta_ref(seqs, depths, int(p["first_id"]), mn)
            got = np.load(out_dir / f"{setname}_k{k}_min{mn}_rank{r}.text.npy").tobytes()
            assert got == text, f"{what} min_len={mn} rank {r}: the kept text"
            assert (fa["n_bytes"], fa["file_offset"]) == (len(text), off), f"{what} min_len={mn} rank {r}"
            info = res[f"info{mn}"]
            assert info["n_written"] == len(kept) and info["file_offset"] == off
            assert info["write_chunks"] == (1 if text else 0)  # a rank without bytes writes nothing
            texts.append(text)
            off += len(text)
        kept_all = [d for s, d in zip(one_seqs, one_depths) if len(s) >= mn]
        assert bits(parts[0]["results"][f"stats{mn}"]["all"]["tot_depth"]) == bits(depth_sum), f"{what}: not in rank order"
        assert abs(depth_sum - exp_all["tot_depth"]) <= F.depth_bound(kept_all), what
        assert all(p["results"][f"fasta{mn}"]["n_bytes_all"] == off for p in parts), what
        # the one file: the ranks' texts in rank order
        whole = fasta_file(out_dir, setname, k, mn).read_bytes()
        assert whole == b"".join(texts), f"{what} min_len={mn}: the file"
        recs, one = records(whole), records(F.fasta_ref(one_seqs, one_depths, 0, mn))
        if mn == 0:
            assert [h for h, _, _ in recs] == [b">Contig%d" % i for i in range(len(one_seqs))], what
        assert sorted((s, d) for _, d, s in recs) == sorted((s, d) for _, d, s in one), f"{what} min_len={mn}: the records"
    return parts


@pytest.mark.parametrize("setname,k", CASES)
def test_two_ranks_over_gloo(world2, setname, k):
    check_case(world2, 2, setname, k)


@pytest.mark.parametrize("setname,k", CASES)
def test_three_ranks_over_gloo(world3, setname, k):
    parts = check_case(world3, 3, setname, k)
    if setname == "tandem":  # a rank that owns no contig takes part, writes nothing and gets the right `all`
        empty = [p for p in parts if len(p["depths"]) == 0]
        assert len(empty) == 2
        for p in empty:
            assert p["results"]["fasta0"]["n_bytes"] == 0 and p["results"]["stats0"]["mine"]["n_ctgs"] == 0
            assert p["results"]["stats0"]["all"]["n_ctgs"] == 1


@pytest.mark.parametrize("setname,k", RCCL_CASES)
def test_two_ranks_over_rccl(rccl2, setname, k):
    check_case(rccl2, 2, setname, k)


def test_tandem_leaves_a_rank_without_contigs_at_two_ranks(world2):
    parts = load(world2, 2, "tandem", 21)
    assert sorted(len(p["depths"]) for p in parts) == [0, 1]


@pytest.mark.parametrize("world_name,world", [("world2", 2), ("world3", 3), ("rccl2", 2)])
def test_generic_calls_and_one_failing_rank(world_name, world, request):
    """A bad depth on rank 1 only fails every rank (MHMKC_EINVAL there, MHMKC_ETRANSPORT elsewhere) and leaves no text; the
    good call after it gives the file of all ranks' texts at the prefix sums, and the reduced figures with the exact N50."""
    from mr_fasta_worker import generic_case

    out_dir = request.getfixturevalue(world_name)
    parts = []
    for r in range(world):
        p = dict(np.load(out_dir / f"generic_rank{r}.npz"))
        p["results"] = json.loads(str(p["results"]))
        parts.append(p)
    cases = [generic_case(r) for r in range(world)]
    texts = [F.fasta_ref(c.seqs, c.depths, c.first_id, 0) for c in cases]
    all_seqs = tuple(s for c in cases for s in c.seqs)
    all_depths = tuple(d for c in cases for d in c.depths)
    exp_all = F.stats_ref(all_seqs, all_depths, 0)
    off = 0
    for r, p in enumerate(parts):
        assert int(p["code"]) == (EINVAL if r == 1 else ETRANSPORT) and int(p["gone"]) == ESTATE, r
        assert int(p["missing"]) == (EIO if r == 0 else ETRANSPORT), r  # rank 0 could not create the file
        assert p["text"].tobytes() == texts[r]
        fa, st = p["results"]["fasta"], p["results"]["stats"]
        assert fa == {"n_bytes": len(texts[r]), "file_offset": off, "n_bytes_all": sum(map(len, texts))}
        off += len(texts[r])
        exp_mine = F.stats_ref(cases[r].seqs, cases[r].depths, 0)
        for f in INT_FIELDS:
            assert st["mine"][f] == exp_mine[f] and st["all"][f] == exp_all[f], (r, f)
        assert st["mine"]["tot_depth"] == exp_mine["tot_depth"]  # (a few quarters: exact)
        assert st["all"]["tot_depth"] == exp_all["tot_depth"]
    assert (out_dir / "generic.fasta").read_bytes() == b"".join(texts)
