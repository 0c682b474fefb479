"""The reference of supermer formation (tests/supermer_cases.py) against the oracle, and every case's proof that it has
its edge: no GPU. tests/test_supermer_edges.py runs the same cases through the supermer exchange on the GPU."""
import numpy as np
import pytest

import oracle_lib as O
import supermer_cases as S

KW = [(k, w) for k in S.KS for w in (2, 3, 4)]


@pytest.mark.parametrize("name", list(S.CASES) + list(S.EXTRA_CASES))
@pytest.mark.parametrize("k", S.KS)
def test_windows_equal_oracle_extract(name, k):
    """The reference's windows are oracle_lib.extract's: same number, same keys and ext codes in the same order (the
    flank bits gl / gr are what make the ext codes)."""
    batches, _ = S.built(name, k, 2)
    for r in sorted(batches):
        for i, (b, o, _) in enumerate(batches[r]):
            x = S.windows(b, o, k)
            keys, exts = O.extract(b, o, k)
            assert x.pos.size == keys.shape[0], f"{name} k={k} rank {r} batch {i}: {x.pos.size} vs {keys.shape[0]} windows"
            bad = np.flatnonzero((x.keys != keys).any(axis=1))
            assert bad.size == 0, f"{name} k={k} rank {r} batch {i}: {bad.size} keys differ, first at window {bad[:1]}"
            bad = np.flatnonzero(x.ext != exts)
            assert bad.size == 0, f"{name} k={k} rank {r} batch {i}: {bad.size} ext codes differ, first at {bad[:1]}"


@pytest.mark.parametrize("k,world", KW)
def test_cases_have_their_edges(k, world):
    """Every case's predicate holds; the message names the figure that is missing."""
    for name in list(S.CASES) + list(S.EXTRA_CASES):
        case = S.CASES.get(name) or S.EXTRA_CASES[name]
        batches, refs = S.built(name, k, world)
        assert sorted(batches) == list(range(world)), f"{name}: ranks {sorted(batches)}"
        fig = case.figures(k, world, batches, refs)
        missing = [what for what, ok in fig.items() if not ok]
        assert not missing, f"{name} k={k} world={world}: {missing} (all figures: {fig})"
        if name in S.CASES and name != "long_ragged":  # (the common sets are taken as they are)
            for r in sorted(batches):
                assert all(b.size <= 120_000 for b, _, _ in batches[r]), f"{name}: a batch of rank {r} is large"


@pytest.mark.parametrize("k,world", KW)
def test_cut_runs_partition_the_windows(k, world):
    """Every window lies in exactly one cut run; a cut run never spans two reads, two tiles or two owners; the maximal
    runs are the cut runs joined across tile edges."""
    T = S.tile_of(k)
    for name in S.CASES:
        _, refs = S.built(name, k, world)
        for r in sorted(refs):
            for x in refs[r]:
                first, n, d = x.runs(True)
                assert int(n.sum()) == x.pos.size and (n > 0).all() and (n <= T).all(), f"{name}: TILE_BASES {T}"
                assert np.array_equal(first, np.cumsum(n) - n)
                run_of = np.repeat(np.arange(first.size), n)
                for what, v in (("read", x.read), ("tile", x.pos // T), ("owner", x.owner)):
                    assert np.array_equal(v, v[first][run_of]), f"{name} k={k}: a cut run spans two {what}s (TILE_BASES {T})"
                assert np.array_equal(x.pos, x.pos[first][run_of] + np.arange(x.pos.size) - first[run_of])
                # adjacent cut runs of one read and owner meet only at a tile edge
                same = (x.read[first[1:]] == x.read[first[:-1]]) & (d[1:] == d[:-1]) if first.size > 1 else np.zeros(0, bool)
                assert (x.pos[first[1:]][same] % T == 0).all(), f"{name} k={k}: a cut inside a tile (TILE_BASES {T})"
                assert x.n_runs() == x.n_cut() - int(same.sum())
                cnt, words = x.per_dest()
                assert int(cnt.sum()) == x.n_cut() and int(words.sum()) == x.words()
                assert np.array_equal(np.bincount(d, weights=n, minlength=world).astype(np.int64), x.owned())


@pytest.mark.skipif(O.kcountref() is None, reason="oracle/_ref not built (the reference tree is absent)")
@pytest.mark.parametrize("k,world", KW)
def test_owners_equal_reference_build(k, world):
    """The owners of a sample of every case's keys equal the reference's own get_kmer_target_rank."""
    R = O.RefKmer(k)
    for name in S.CASES:
        _, refs = S.built(name, k, world)
        for r in sorted(refs):
            for x in refs[r]:
                if not x.pos.size:
                    continue
                sel = np.unique(np.linspace(0, x.pos.size - 1, 300).astype(np.int64))
                got, _ = R.target_ranks(x.keys[sel], world)
                assert np.array_equal(got.astype(np.int64), x.owner[sel]), f"{name} k={k} world={world} rank {r}"
