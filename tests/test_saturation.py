"""Extension decisions at counter saturation, for every kind of threshold the library accepts.

k_count keeps a k-mer's eight extension counters as 16-bit halves and clamps a half that reaches 0xC000 back to 0x8000;
the reference keeps 16-bit counters that saturate at 65535 and compares them with max((int)((1 - dyn_min_depth) count),
dmin_thres), which passes 0x8000 once dyn_min_depth < 0.5. saturation_cases.py builds inputs whose counters sit at exact
values next to those levels; here the literal rows are pinned to the CPU oracle and to the reference's own code (CPU),
and the GPU's whole table to the oracle, across record kinds and count paths."""
from __future__ import annotations

import numpy as np
import pytest

import mhm2_proxy_amd as m
import oracle_lib as O
import saturation_cases as S
from common import assert_tables_equal, oracle_ctg_table, oracle_table, ref_table, synth_set

K0 = 21
HOT0 = S.HOT["compact"]
READ_CASES = S.read_cases(HOT0, K0)
CTG_CASES = S.ctg_cases("S")


# ---- shared inputs ---------------------------------------------------------------------------------------------------

_READS, _BG, _EXP = {}, {}, {}


def case_reads(key, name, k, wide=False):
    """The reads of an input (cached: the cases of one input differ in the parameters alone)."""
    kind = S.record_kind(k, wide)
    tag = (key, name, k, kind if "hot" in name else None)
    if tag not in _READS:
        _READS[tag] = S.reads(S.inputs(key, S.HOT[kind])[name], key, k)
    return _READS[tag]


def background(k, dense=False):
    """300 random reads, so that the table is not one row. dense: 400 reads of a genome of 20000 instead, which puts more
    distinct keys into a coarse bucket than a 64-slot table holds (the forced re-sweeps)."""
    if (k, dense) not in _BG:
        b, o = synth_set(400, 20000, 77 + k) if dense else synth_set(300, 6000, 77 + k)
        _BG[k, dense] = [b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)]
    return _BG[k, dense]


def find_row(t: m.KmerTable, key_s: str):
    """(count, left, right) of the key's row in a table, or None."""
    kw = np.asarray(m.kmer_from_string(key_s, t.keys.shape[1] if t.keys.ndim == 2 else None), dtype=np.uint64)
    hit = np.flatnonzero((t.keys.reshape(len(t), -1) == kw).all(axis=1)) if len(t) else np.zeros(0, int)
    assert hit.size <= 1
    if not hit.size:
        return None
    i = int(hit[0])
    return int(t.counts[i]), chr(t.left[i]), chr(t.right[i])


# ---- CPU: the literal rows, the oracle and the reference's own code ---------------------------------------------------

def test_hot_constants_match_the_source():
    """HOT per record kind, from the launch header's table sizes (the static_assert HOT > 0x8000 of k_count)."""
    src = (O.ROOT / "mhm2_proxy_amd" / "csrc" / "kcount_launch.hpp").read_text()
    assert "constexpr int COUNT_CAP[5] = {0, 5120, 4000, 3264, 2752};" in src and "(cmp ? 6144 : COUNT_CAP[nl])" in src
    lds = 163840

    def miss_cap(nl, cmp):
        kb = 4 if cmp else 8
        table = (6144 if cmp else [0, 5120, 4000, 3264, 2752][nl]) * (kb * nl + 20) + 256
        return (lds - table) // (kb * nl + 4) & ~63

    assert S.MISS_CAP == {"compact": miss_cap(1, True), "wide1": miss_cap(1, False), 2: miss_cap(2, False),
                          3: miss_cap(3, False), 4: miss_cap(4, False)}
    assert all(0x8000 < h < 0xC000 for h in S.HOT.values()), S.HOT


@pytest.mark.parametrize("key", ["A", "S"])
def test_literal_rows_equal_oracle(key):
    """Every read case's arithmetic row is the oracle's row of the hot key (the case's reads alone, k = 21)."""
    key_s = S.key_string(key, K0)
    seen = 0
    for c in READ_CASES:
        if c.key != key:
            continue
        b, o = S.join(case_reads(key, c.name, K0))
        exp = S.row(S.case_records(c, HOT0), c.dyn, c.dmin)
        t = oracle_table(b, o, K0, dmin_thres=c.dmin, dyn_min_depth=c.dyn)
        assert find_row(t, key_s) == exp, c.id
        assert len(t) == (exp is not None), c.id  # no other k-mer: every read holds the key alone
        seen += 1
    assert seen >= 40


def test_hot_edge_rows_equal_oracle_for_every_record_kind():
    """The inputs at HOT - 1, HOT, HOT + 1 of the other record kinds (their HOT differs), on key A at each kind's k."""
    for k, wide in ((21, True), (33, False), (77, False), (99, False)):
        hot = S.HOT[S.record_kind(k, wide)]
        for name in ("pure_hot-1", "pure_hot", "pure_hot+1"):
            recs = S.inputs("A", hot)[name]
            b, o = S.join(S.reads(recs, "A", k))
            t = oracle_table(b, o, k, dmin_thres=2, dyn_min_depth=0.0)
            assert find_row(t, "A" * k) == S.row(recs, 0.0, 2) == (sum(recs.values()), "A", "A"), (k, name)


def test_cases_discriminate():
    """Which decision each case sits next to, and that together they hold every transition at a threshold above
    0x8000 with a counter at or past the clamp level."""
    ins = {key: S.inputs(key, HOT0) for key in ("A", "S")}
    near = {c: S.near(ins[c.key][c.name], c.dyn, c.dmin) for c in READ_CASES}
    assert all(S.discriminates(ins[c.key][c.name], c.dyn, c.dmin) for c in READ_CASES)
    declared = {  # (input, dyn, dmin): the neighbour, the row
        ("pure_65536", 0.0, 2): ("X>base", (65535, "A", "A")),       # top == thr == 65535
        ("top_65534", 0.0, 2): ("X>base", None),                      # top one below thr 65535: purged
        ("top_65535", 0.0, 2): ("kept>purged", (65535, "A", "A")),
        ("top_49150", 0.25, 2): ("kept>purged", None),                # thr 49151
        ("top_49151", 0.25, 2): ("X>base", (65535, "A", "A")),
        ("top_33421", 0.49, 2): ("X>base", None),                     # thr 33422
        ("top_32767", 0.9, 32768): ("kept>purged", None),
        ("top_32768", 0.9, 32768): ("X>base", (65535, "A", "A")),
        ("top_32766", 0.9, 32767): ("X>base", None),
        ("top_32766", 0.5, 2): ("X>base", None),                      # thr (int)(0.5 * 65535) = 32767
        ("top_1", 1.0, 2): ("kept>purged", None),                     # thr 2 under a count of 65535
        ("two_c001_49150", 0.25, 2): ("base>F", (65535, "A", "A")),
        ("two_c001_49151", 0.25, 2): ("base>F", (65535, "F", "F")),
        ("two_c001_33422", 0.49, 2): ("base>F", (65535, "F", "F")),
        ("two_c001_32767", 0.9, 32768): ("base>F", (65535, "A", "A")),
        ("pure_7fff", 0.9, 2): (None, None),                          # far from every threshold: not a case
        ("two_c001_2", 1.0, 2): ("base>F", (65535, "F", "F")),
        ("two_65535_65534", 0.0, 2): ("base>F", (65535, "A", "A")),
        ("two_65535_65535", 0.0, 2): ("base>F", (65535, "F", "F")),
        ("leftnone_6552", 0.9, 2): ("X>base", (65535, "X", "A")),
        ("rightnone_6553", 0.9, 2): ("X>base", (65535, "A", "A")),
    }
    for (name, dyn, dmin), (tag, row) in declared.items():
        got = S.near(ins["A"][name], dyn, dmin)
        if tag is None:
            assert not got and S.Case(name, "A", dyn, dmin) not in near, name
            continue
        assert tag in got and S.Case(name, "A", dyn, dmin) in near, (name, got)
        assert S.row(ins["A"][name], dyn, dmin) == row, name
    for name, dyn, dmin in (("pure_51200", 0.25, 2), ("two_65536_40000", 0.25, 2), ("pure_65536", 0.0, 2)):
        assert S.clamped_wrong(ins["A"][name], dyn, dmin), name          # a half read as 0x8000 is below the threshold
    for name in ("pure_c000", "two_c001_49152", "two_c001_32767"):
        assert not S.clamped_wrong(ins["A"][name], 0.9, 32768)            # 0x8000 == thr: exact at the clamp's target,
        assert S.clamped_wrong(ins["A"][name], 0.9, 32768, 0x7FFF), name  # and wrong one below it
    # the transitions where a clamped half decides under a threshold above its target
    wrong = [c for c in READ_CASES if S.clamped_wrong(ins[c.key][c.name], c.dyn, c.dmin)]
    tags = set().union(*(near[c] for c in wrong))
    assert {"X>base", "base>F", "kept>purged"} <= tags, tags
    for k, wide in ((21, False), (21, True), (33, False), (63, False), (77, False), (99, False)):
        sub = S.subset_cases(k, wide)
        hot = S.HOT[S.record_kind(k, wide)]
        sw = [c for c in sub if S.clamped_wrong(S.case_records(c, hot), c.dyn, c.dmin)]
        st = set().union(*(S.near(S.case_records(c, hot), c.dyn, c.dmin) for c in sw))
        assert {"X>base", "base>F", "kept>purged"} <= st, (k, st)
        assert max(S.packed_bytes(S.case_records(c, hot), c.key, k) for c in sub) <= S.MAX_BYTES
    # contig cases: a kept hot entry and a contig depth, each at or past the clamp level under such a threshold
    cw = [c for c in CTG_CASES if S.ctg_clamped_wrong(c)]
    assert {c.state for c in cw} >= {"absent", "singleton", "nonuu", "hot_ff", "hot_uu"}
    assert all(S.ctg_row(c) is not None for c in cw if len(c.ctgs) == 1)
    hot_uu = [c for c in CTG_CASES if c.state == "hot_uu"]
    assert all(S.ctg_row(c) == (51200, "G", "T") for c in hot_uu)  # kept at every dyn_min_depth


def _ctg_input(c: S.CtgCase, k: int, bg=()):
    b, o = S.join(list(bg) + S.reads(S.ctg_states(c.key)[c.state], c.key, k))
    seqs, depths = S.ctg_seqs(c, k)
    return b, o, seqs, depths


def test_contig_rows_equal_oracle():
    key_s = S.key_string("S", K0)
    for c in CTG_CASES:
        b, o, seqs, depths = _ctg_input(c, K0)
        t = oracle_ctg_table(b, o, seqs, depths, K0, dmin_thres=c.dmin, dyn_min_depth=c.dyn)
        assert find_row(t, key_s) == S.ctg_row(c), c.id


REF_VARIANTS = [(None, 20, 0.9), ("q25d75", 25, 0.75), ("d25", 20, 0.25)]


@pytest.mark.parametrize("variant,qcut,dyn", REF_VARIANTS, ids=["default", "q25d75", "d25"])
def test_reference_build_gives_the_same_rows(variant, qcut, dyn):
    """The reference's own kcount code on every input (both keys) and on the contig cases of its dyn_min_depth: the
    oracle's 65535 saturation is the reference's, also where the threshold passes 0x8000 (the d25 build)."""
    if O.kcountref() is None or O.kcountref(variant) is None:
        pytest.skip("oracle/_ref/libkcountref.so not built (reference tree absent)")
    for key in ("A", "S"):
        for name, recs in S.inputs(key, HOT0).items():
            if S.packed_bytes(recs, key, K0) > S.MAX_BYTES:
                continue
            b, o = S.join(case_reads(key, name, K0))
            for dmin in (2, 32768) if variant is None else (2,):
                ref = ref_table(b, o, K0, dmin_thres=dmin, variant=variant)
                assert find_row(ref, S.key_string(key, K0)) == S.row(recs, dyn, dmin), (key, name, dmin)
                assert_tables_equal(ref, oracle_table(b, o, K0, qual_cutoff=qcut, dmin_thres=dmin, dyn_min_depth=dyn),
                                    f"{key} {name} dmin={dmin}")
    for c in CTG_CASES:
        if c.dyn != (dyn if dyn in S.CTG_DYN else 0.25):  # (q25d75: the inputs of the 0.25 cases)
            continue
        b, o, seqs, depths = _ctg_input(c, K0)
        ref = ref_table(b, o, K0, seqs, depths, dmin_thres=c.dmin, variant=variant)
        exp = oracle_ctg_table(b, o, seqs, depths, K0, qual_cutoff=qcut, dmin_thres=c.dmin, dyn_min_depth=dyn)
        assert_tables_equal(ref, exp, f"{variant}: {c.id}")
        if c.dyn == dyn:
            assert find_row(ref, S.key_string("S", K0)) == S.ctg_row(c), c.id


# ---- GPU: the whole table against the oracle ---------------------------------------------------------------------------

def _hip(b, o, k, dyn, dmin, cuts=None, seqs=None, depths=None):
    cuts = cuts or [0, o.size - 1]
    with m.KmerCounter(k, dmin_thres=dmin, dyn_min_depth=dyn) as c:
        for a, z in zip(cuts[:-1], cuts[1:]):
            base = int(o[a])
            c.add_packed_reads(b[base:int(o[z])], (o[a:z + 1] - o[a]).astype(np.uint64))
        if seqs:
            c.add_ctgs(seqs, depths)
        c.finish()
        return c.fetch(), c.stats()


def _path(st) -> str:
    return (f"exact_reruns={st['exact_reruns']} overflow_sweeps={st['overflow_sweeps']} max_bucket={st['max_bucket']} "
            f"finish_passes={st.get('finish_passes')}")


def _check(got, st, exp, what):
    assert st["distinct"] == st["n_out"] + st["purged"], f"{what}: {_path(st)}"
    assert st["dropped"] == 0, what
    assert_tables_equal(got, exp, f"{what} [{_path(st)}]")


def _expected(c: S.Case, k: int, wide: bool, dense: bool = False):
    """(bytes, offsets, background reads, oracle table) of a case at k with the background in front."""
    kind = S.record_kind(k, wide)
    tag = (c, k, kind if "hot" in c.name else None, dense)
    if tag not in _EXP:
        bg = background(k, dense)
        b, o = S.join(bg + case_reads(c.key, c.name, k, wide))
        exp = oracle_table(b, o, k, dmin_thres=c.dmin, dyn_min_depth=c.dyn)
        row = S.row(S.inputs(c.key, S.HOT[kind])[c.name], c.dyn, c.dmin)
        assert find_row(exp, S.key_string(c.key, k)) == row, c.id
        _EXP[tag] = (b, o, len(bg), exp)
    return _EXP[tag]


def _run_read_case(c: S.Case, k: int, wide: bool = False, thirds: bool = False, dense: bool = False):
    b, o, n_bg, exp = _expected(c, k, wide, dense)
    n = o.size - 1
    cuts = [0, n_bg + (n - n_bg) // 3, n_bg + 2 * (n - n_bg) // 3, n] if thirds else None  # inside the hot key's reads
    got, st = _hip(b, o, k, c.dyn, c.dmin, cuts)
    _check(got, st, exp, f"k={k} {c.id}")
    return st


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("c", READ_CASES, ids=lambda c: c.id)
def test_read_case_compact(c):
    _run_read_case(c, K0)


SUBSET_KS = [(21, True), (33, False), (63, False), (77, False), (99, False)]


def _subset_params(ks):
    return [pytest.param(k, wide, c, id=f"k{k}{'w' if wide else ''}-{c.id}") for k, wide in ks
            for c in S.subset_cases(k, wide)]


@gpu
@pytest.mark.parametrize("k,wide,c", _subset_params(SUBSET_KS))
def test_subset_per_record_kind(k, wide, c, knob):
    """The adds, the clamp and HOT are instantiated per record kind: wide one-word, two-, three- and four-word keys."""
    if wide:
        knob("wide_records", 1)
    _run_read_case(c, k, wide)


@gpu
@pytest.mark.parametrize("mode", ["resweeps", "exact", "thirds", "passes"])
@pytest.mark.parametrize("k,wide,c", _subset_params([(21, False), (63, False)]))
def test_subset_count_paths(k, wide, c, mode, knob, monkeypatch):
    """The hot key counted in forced re-sweeps of a 64-slot table, through the exact partition, from three
    add_packed_reads calls cut inside its reads, and in a multi-pass finish."""
    if mode == "resweeps":
        knob("cap", 64)
        knob("fine_bits", 0)
        if k <= 21:  # compact records need 2k - 34 fine bits
            knob("wide_records", 1)
            wide = True
    elif mode == "exact":
        knob("exact", 1)
    elif mode == "passes":
        monkeypatch.setenv("MHMKC_PASSES", "3")
    st = _run_read_case(c, k, wide, thirds=mode == "thirds", dense=mode == "resweeps")
    if mode == "resweeps":
        assert st["overflow_sweeps"] > 0, _path(st)
    if mode == "passes":
        assert st["finish_passes"] == 3, _path(st)


_CTG_EXP = {}


def _run_ctg_case(c: S.CtgCase, k: int):
    if (c, k) not in _CTG_EXP:
        b, o, seqs, depths = _ctg_input(c, k, background(k))
        exp = oracle_ctg_table(b, o, seqs, depths, k, dmin_thres=c.dmin, dyn_min_depth=c.dyn)
        assert find_row(exp, S.key_string(c.key, k)) == S.ctg_row(c), c.id
        _CTG_EXP[c, k] = (b, o, seqs, depths, exp)
    b, o, seqs, depths, exp = _CTG_EXP[c, k]
    got, st = _hip(b, o, k, c.dyn, c.dmin, seqs=seqs, depths=depths)
    assert st["ctg_kmers"] > 0
    _check(got, st, exp, f"k={k} {c.id}")


@gpu
@pytest.mark.parametrize("c", CTG_CASES, ids=lambda c: c.id)
def test_contig_case_compact(c):
    """Each read-side state with and without ("absent") the read, against one or two contig occurrences."""
    _run_ctg_case(c, K0)


# at two- and three-word keys the hot states ride on A^k (S's single-record reads would pass the input bound)
CTG_SUBSET = ([c for c in S.ctg_cases("S", ["absent", "singleton", "nonuu"], [0.25, 0.0])] +
              [c for c in S.ctg_cases("A", ["hot_ff", "hot_uu"], [0.25, 0.0])])


@gpu
@pytest.mark.parametrize("k", [63, 77])
@pytest.mark.parametrize("c", CTG_SUBSET, ids=lambda c: c.id)
def test_contig_subset_wide_keys(c, k):
    _run_ctg_case(c, k)
