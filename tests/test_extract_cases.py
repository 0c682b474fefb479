"""The reference of read extraction (tests/extract_cases.py) against the oracle, every case's proof that it has its
edge, and the proof that every counted window of a case is decisive: no GPU. tests/test_extract_edges.py runs the same
cases through KmerCounter on the GPU."""
import numpy as np
import pytest

import extract_cases as E
import oracle_lib as O

NAMES_KS = [(name, k) for k in E.KS for name in E.cases_for(k)]
FLIP_SITES, INERT_SITES, FULL_TABLE_SITES = 200, 60, 4


def test_constants_match_the_source():
    """The geometry the cases aim at is the sources': tile, threads and stage capacity by key words."""
    src = E.source_constants()
    assert src["TILE_BASES"] == E.TILE, "TILE_BASES moved: the tile_edges, data_end and rounds cases aim at the old tile"
    assert src["E_THREADS_NL"] == E.THREADS, "E_THREADS_NL moved: span_phases aims at the old span W = T / threads"
    assert src["E_CAP"] == E.E_CAP, "E_CAP moved: the rounds case aims at the old stage capacity"
    assert all(E.SPAN[nl] * E.THREADS[nl] == E.TILE[nl] and E.SPAN[nl] <= 32 for nl in E.TILE)
    assert E.round_counts(2) == [2559, 2560, 2561] and E.round_counts(3) == [1023, 1024, 1025]
    assert E.round_counts(4) == [767, 768, 769, 1536, 1537]


def test_every_walk_has_its_k():
    nl = [E.n_longs(k) for k in E.KS]
    assert [nl.count(n) for n in (1, 2, 3, 4)] == [7, 6, 3, 3]
    assert {21, 33, 55, 63, 77, 99} <= set(E.KS), "the k compiled into the walks"
    assert all(10 <= k <= 127 and k % 32 for k in E.KS)


def _table_equals_oracle(w, name, k, qcut):
    keys, counts, left, right, st = E.oracle(name, k, qcut)
    t = E.table(w)
    what = f"{name} k={k} qcut={qcut}"
    assert {key: st[key] for key in ("occurrences", "distinct", "purged", "n_out")} == t.stats, what
    assert np.array_equal(t.keys, keys), what
    assert np.array_equal(t.counts, counts) and np.array_equal(t.left, left.view(np.uint8)) \
        and np.array_equal(t.right, right.view(np.uint8)), what


@pytest.mark.parametrize("name,k", NAMES_KS)
def test_reference_equals_oracle(name, k):
    """The reference's windows are oracle_lib.extract's (same keys and ext codes in the same order), batch by batch and
    at every quality cutoff of the case, and its table and stats are oracle_lib.kcount's."""
    bu = E.built(name, k)
    for qcut in E.CASES[name].qcuts:
        for i, bt in enumerate(bu.batches):
            w = E.windows(bt.b, bt.o, k, qcut)
            keys, exts = O.extract(bt.b, bt.o, k, qual_cutoff=qcut)
            what = f"{name} k={k} qcut={qcut} batch {i}"
            assert w.pos.size == keys.shape[0], f"{what}: {w.pos.size} vs {keys.shape[0]} windows"
            bad = np.flatnonzero((w.keys != keys).any(axis=1))
            assert bad.size == 0, f"{what}: {bad.size} keys differ, first at window {bad[:1]}"
            bad = np.flatnonzero(w.ext != exts)
            assert bad.size == 0, f"{what}: {bad.size} ext codes differ, first at window {bad[:1]}"
        a = bu.all_reads()
        _table_equals_oracle(E.windows(a.b, a.o, k, qcut), name, k, qcut)


@pytest.mark.parametrize("k", E.KS)
def test_cases_have_their_edges(k):
    """Every case's figures and its decisiveness conditions hold; the message names what is missing."""
    for name in E.cases_for(k):
        bu = E.built(name, k)
        fig = {**E.decisive(k, bu), **E.CASES[name].figures(k, bu)}
        missing = [what for what, ok in fig.items() if not ok]
        assert not missing, f"{name} k={k}: {missing} (all figures: {fig})"
        assert sum(bt.b.size for bt in bu.batches) <= 70_000, f"{name} k={k}: the case grew large"


def _flip(b, x):
    """The byte array with base x's quality moved to the other side of the cutoff."""
    out = b.copy()
    out[x] = (out[x] & 7) | ((E.LOWQ if (out[x] >> 3) >= E.QCUT else E.GOODQ) << 3)
    return out


@pytest.mark.parametrize("name,k", NAMES_KS)
def test_every_counted_window_is_decisive(name, k):
    """Flip the quality of one base of a first copy across the cutoff. If the base is the neighbour of a counted window
    whose key occurs exactly twice (every key at k >= 16) and is not N, the reference's table changes; if it is nobody's
    neighbour, or N, the table stays. FLIP_SITES and INERT_SITES sampled bases (all the inert ones, where the case has
    fewer), the rows of the keys the base touches compared (a row depends on its own key's windows alone); for
    FULL_TABLE_SITES of each, the whole table."""
    a = E.built(name, k).all_reads()
    w = E.windows(a.b, a.o, k)
    rng = np.random.default_rng(k)
    twice = np.bincount(w.inv, minlength=w.ukeys.shape[0])[w.inv] == 2
    nb_l, nb_r = w.pos - 1, w.pos + k
    touched = np.zeros(a.b.size, bool)
    touched[nb_l] = touched[nb_r] = True
    sure = np.zeros(a.b.size, bool)  # a neighbour of a window whose key occurs exactly twice
    sure[nb_l[twice]] = sure[nb_r[twice]] = True
    isn = (a.b & 7) == 4
    sites = np.flatnonzero(sure & a.first & ~isn)
    inert = np.flatnonzero(a.first & (~touched | isn))
    assert sites.size >= FLIP_SITES and inert.size > 0, f"{name} k={k}: {sites.size} decisive, {inert.size} inert bases"
    by_left = {int(p): i for i, p in enumerate(nb_l)}
    by_right = {int(p): i for i, p in enumerate(nb_r)}
    full0 = E.table(w)

    def rows_of(x):
        return [int(w.inv[d[x]]) for d in (by_left, by_right) if x in d]

    def changed(x, whole):
        left, right = E.ext_codes(w, E.good_bits(_flip(a.b, x)))
        if whole:
            return not E.table(w, left, right).same(full0)
        rows = rows_of(x)
        return bool(rows) and not E.table(w, left, right, rows=rows).same(E.table(w, rows=rows))

    pick = rng.permutation(sites)[:FLIP_SITES]
    missed = [int(x) for i, x in enumerate(pick) if not changed(int(x), i < FULL_TABLE_SITES)]
    assert not missed, f"{name} k={k}: flips at {missed[:5]} ({len(missed)} of {pick.size}) leave the table unchanged"
    pick = rng.permutation(inert)[:INERT_SITES]
    seen = [int(x) for i, x in enumerate(pick) if changed(int(x), i < FULL_TABLE_SITES)]
    assert not seen, f"{name} k={k}: flips at {seen[:5]}, bases that are nobody's neighbour or N, change the table"


@pytest.mark.parametrize("k", [10, 21, 63, 77, 127])
def test_reference_checks_fail_when_broken(k):
    """The comparisons above are sharp: hand the reference an input in which one neighbour base is another letter (a
    wrong flank base), or one read start is dropped (two reads run together), and its ext codes, windows and table no
    longer equal the oracle's of the true input."""
    name = "tile_edges"
    bt = E.built(name, k).batches[0]
    keys, exts = O.extract(bt.b, bt.o, k)
    t = O.kcount(bt.b, bt.o, k)
    okeys, _, oleft, oright = t.fetch()
    w = E.windows(bt.b, bt.o, k)
    assert np.array_equal(w.ext, exts)
    rng = np.random.default_rng(k)
    good = E.good_bits(bt.b)
    # a wrong flank base: the good left neighbour of a counted window takes another letter
    lens = np.diff(bt.o.astype(np.int64))
    for wi in rng.permutation(w.pos.size)[:20]:
        x = int(w.pos[wi]) - 1
        if not (good[x] and bt.first[x]):
            continue
        b2 = bt.b.copy()
        b2[x] = ((int(b2[x]) & 3) ^ 1) | (int(b2[x]) & 0xF8)
        w2 = E.windows(b2, bt.o, k)
        assert not np.array_equal(w2.ext, exts), f"k={k}: a wrong flank base at {x} went unseen in the ext codes"
        t2 = E.table(w2)
        assert not (np.array_equal(t2.keys, okeys) and np.array_equal(t2.left, oleft.view(np.uint8))
                    and np.array_equal(t2.right, oright.view(np.uint8))), f"k={k}: a wrong flank base at {x}: same table"
    # an ignored read start: two countable neighbours become one read
    pairs = np.flatnonzero((lens[:-1] >= k + 2) & (lens[1:] >= k + 2))
    assert pairs.size
    for r in rng.permutation(pairs)[:10]:
        o2 = np.delete(bt.o, r + 1)
        w2 = E.windows(bt.b, o2, k)
        assert w2.pos.size == w.pos.size + k + 1, "the joined read counts the k + 1 windows over the dropped start"
        # (the k + 1 extra windows are singletons and purged, so the rows can be the same: the stats are compared too,
        # here and in the GPU rows)
        st2, st = E.table(w2).stats, t.stats()
        assert st2["occurrences"] == st["occurrences"] + k + 1, f"k={k}: a dropped read start at read {r + 1}"
        assert (st2["distinct"], st2["purged"]) != (st["distinct"], st["purged"]), f"k={k}: read {r + 1}: same stats"


def test_host_chunks_rule():
    """host_chunks on a hand-made batch: the byte path ends a chunk at the first read boundary `chunk` bytes on, the
    nibble path takes a quarter for the first chunk and at most max(64, chunk / 32) reads a chunk."""
    o = np.concatenate([[0], np.cumsum([100] * 30)])
    assert E.host_chunks(o, 250, 0) == [0, 3, 6, 9, 12, 15, 18, 21, 24, 27]
    assert E.host_chunks(o, 400, 1) == [0, 1, 5, 9, 13, 17, 21, 25, 29]
    assert E.host_chunks(o, 10, 0) == list(range(30)), "a chunk is at least 64 bytes and one read"
    o = np.concatenate([np.zeros(200, np.int64), [50, 5000, 5100]])  # 199 empty reads, then 50, 4950 and 100 bases
    assert E.host_chunks(o, 1000, 0) == [0, 201] and E.host_chunks(o, 1000, 1) == [0, 64, 128, 192, 201]
    assert E.chunk_heads([0, 17, 81, 152, 300], 64, 0) == [0, 1, 8]


@pytest.mark.skipif(O.kcountref() is None, reason="oracle/_ref not built (the reference tree is absent)")
@pytest.mark.parametrize("k", [21, 63, 77, 127])
def test_reference_equals_reference_build(k):
    """One k per key width: the reference's table of every case equals the table of MetaHipMer2's own analyze_kmers."""
    for name in E.cases_for(k):
        a = E.built(name, k).all_reads()
        r = O.ref_analyze_kmers(a.b, a.o, k)
        assert (r.warnings, r.dropped) == (0, 0)
        order = np.lexsort(tuple(r.keys[:, i] for i in range(r.keys.shape[1] - 1, -1, -1)))
        t = E.table(E.windows(a.b, a.o, k))
        what = f"{name} k={k}"
        assert np.array_equal(t.keys, r.keys[order]), what
        assert np.array_equal(t.counts, r.counts[order]), what
        assert np.array_equal(t.left, r.left[order].view(np.uint8)), what
        assert np.array_equal(t.right, r.right[order].view(np.uint8)), what
