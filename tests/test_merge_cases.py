"""The read-pair merge (k_fq_merge, k_fq_merge_pack; merge_reads, src/merge_reads.cpp:237-588) on constructed pairs
(tests/merge_cases.py): the wave, chunk and loop edges of the kernels that pairs drawn from a random genome
(tests/test_fastq_pairs.py) reach by accident or not at all.

CPU: every case shows the structure it was built for in the trace of the literal restatement
(ref_merge_literal.merge_pair), and the C oracle (oracle/merge_reads.c) equals the literal restatement on every case.
GPU: add_fastq_pairs equals the oracle on the case list as one batch, in listed and in a fixed shuffled order, with
the launches' own grids and with the test knob merge_grid at 1 and 3 workgroups (4 and 12 waves), where every wave
takes several pairs in turn: the pair loops of both kernels, their prefetched descriptors and the reuse of a wave's
LDS after another pair."""
from __future__ import annotations

import functools
import random

import numpy as np
import pytest

import merge_cases as M
import oracle_lib as O
import ref_merge_literal as R
import test_fastq_pairs as P

OFFS = (33, 64)
GRIDS = (0, 1, 3)
CASES = {off: M.all_cases(off) for off in OFFS}
ERR_CASES = M.quality_error_cases()
assert len(CASES[64]) == len(CASES[33]) - 1  # (one case puts a quality >= 81 into the output: offset 33 only)


def _ordered(off, order):
    cs = list(CASES[off])
    if order == "shuffled":
        random.Random(20240607).shuffle(cs)
    return cs


@functools.lru_cache(maxsize=None)
def _batch(off, order):
    """-> (text, the oracle's (bytes, offsets, stats)); computed once and shared"""
    t = M.fastq_text(_ordered(off, order), off)
    return t, O.merge_fastq(t, off)


@functools.lru_cache(maxsize=None)
def _turns():
    t = M.fastq_text(M.turn_cases(), 33)
    return t, O.merge_fastq(t, 33)


@functools.lru_cache(maxsize=None)
def _aligned():
    t = M.fastq_text(M.alignment_cases()[0], 33)
    return t, O.merge_fastq(t, 33)


def _ok_pair(n):  # a clean pair in front of an error case, so that the record number is not 0
    return M.Case(f"ok{n}", M.partial(150, 150, 50, 1400 + n), {})


# --------------------------------------------------------------------------------------------------
# CPU


@pytest.mark.parametrize("off,n", [(off, n) for off in OFFS for n in range(len(CASES[off]))],
                         ids=[f"{off}-{n}-{c.name}" for off in OFFS for n, c in enumerate(CASES[off])])
def test_case_structure(off, n):
    """The literal restatement's trace shows what the case was built to hit."""
    M.check_case(CASES[off][n], off)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", range(len(ERR_CASES)), ids=[c.name for c in ERR_CASES])
def test_error_case_structure(n, off):
    tr, res = M.check_case(ERR_CASES[n], off)
    assert res is None and tr["scans"][-1]["i"] == 0


def test_trace_changes_nothing():
    for c in CASES[33][:80] + M.turn_cases()[::M.TURN_COPIES]:
        assert R.merge_pair(*c.mates(33), 33) == R.merge_pair(*c.mates(33), 33, trace={}), c.name


def test_case_list_covers_what_it_names():
    """The breaks, verdict sequences and exits over the whole list, so that a case cannot silently leave it."""
    seen_breaks, seen_exits, seen_verdicts = set(), set(), set()
    for c in CASES[33]:
        tr, _ = M.run_case(c, 33)
        for s in tr["scans"]:
            if s["break"]:
                seen_breaks.add((s["break"], s["break_j"]))
        seen_exits.add(tr["exit"])
        v = tuple(s["verdict"] for s in tr["scans"] if s["verdict"])
        groups = tuple(s["i"] // 64 for s in tr["scans"] if s["verdict"])
        seen_verdicts.add((v, groups[0] != groups[-1] if groups else False))
    for P_ in (63, 64, 127, 128):
        assert {("bothN2", P_), ("manyN", P_), ("mismatch", P_)} <= seen_breaks, P_
    assert ("manyN", 149) in seen_breaks
    assert seen_exits == {None, "abort", "good_again", "weak_after_good"}
    for v in (("good", "good"), ("weak", "good"), ("good", "weak")):
        assert (v, False) in seen_verdicts and (v, True) in seen_verdicts, v


def test_perror_sum_depends_on_order():
    """perror_order_*: the eight terms add up to 1.2 in one order and to the next double in the other, and 1.2 / 48 is
    at the limit: the verdict depends on the order of the additions (the reference's is position order)."""
    terms = [R.Q2PERROR[d] for d in M.ORDER_TERMS]
    assert len(set(terms)) == 8
    fwd = functools.reduce(lambda a, b: a + b, terms, 0.0)
    rev = functools.reduce(lambda a, b: a + b, terms[::-1], 0.0)
    assert fwd != rev and fwd / 48 <= 0.025 < rev / 48
    assert rev == np.nextafter(fwd, 2.0)  # one ulp apart
    by = {c.name: M.run_case(c, 33) for c in M.order_sum_cases()}
    assert by["perror_order_ascending"][0]["scans"][-1]["perror"] == fwd and by["perror_order_ascending"][1][1]
    assert by["perror_order_descending"][0]["scans"][-1]["perror"] == rev and not by["perror_order_descending"][1][1]


def test_coin_flip_limits_are_exact():
    assert 0.5 / 20 <= 0.025 < 0.5 / 19 and 0.5 / 15 <= 0.025 * 4 / 3 < 0.5 / 14


def test_alignment_cases_cover_every_alignment():
    """From the literal restatement's output offsets: each merged length and each unmerged mate-2 length of
    ALIGN_LENS starts at each of the four alignments of the output."""
    cases, want = M.alignment_cases()
    _, offs, _ = R.merge_fastq(M.fastq_text(cases, 33), 33)
    lens = np.diff(offs)
    got = set()
    for kind, L, a, n in want:
        r = 2 * n + (kind == "mate2")
        assert lens[r] == L and offs[r] % 4 == a, (kind, L, a, n, lens[r], offs[r] % 4)
        got.add((kind, L, offs[r] % 4))
    assert got == {(k, L, a) for k in ("merged", "mate2") for L in M.ALIGN_LENS for a in range(4)}


@pytest.mark.parametrize("order", ["listed", "shuffled"])
@pytest.mark.parametrize("off", OFFS)
def test_oracle_equals_literal_on_cases(off, order):
    t, (b, o, st) = _batch(off, order)
    b2, o2, st2 = R.merge_fastq(t, off)
    assert st == st2
    assert list(o) == o2 and b.tobytes() == b2
    assert st["pairs"] == len(CASES[off]) and 0 < st["merged"] < st["pairs"] and st["ambiguous"] >= 15


def test_oracle_equals_literal_on_turns():
    t, (b, o, st) = _turns()
    b2, o2, st2 = R.merge_fastq(t, 33)
    assert st == st2 and list(o) == o2 and b.tobytes() == b2


def test_oracle_equals_literal_case_by_case():
    """Each pair alone: bytes, offsets and all four statistics."""
    for off in OFFS:
        for c in CASES[off]:
            if c.name == "filler":
                continue
            t = M.fastq_text([c], off)
            b, o, st = O.merge_fastq(t, off)
            b2, o2, st2 = R.merge_fastq(t, off)
            assert st == st2 and list(o) == o2 and b.tobytes() == b2, (c.name, off)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", range(len(ERR_CASES)), ids=[c.name for c in ERR_CASES])
def test_oracle_quality_errors(n, off):
    t = M.fastq_text([_ok_pair(0), _ok_pair(1), ERR_CASES[n]], off)
    with pytest.raises(O.FastqError) as e:
        O.merge_fastq(t, off)
    assert e.value.record in (4, 5)
    with pytest.raises(ValueError):
        R.merge_fastq(t, off)


# --------------------------------------------------------------------------------------------------
# GPU


def _assert_gpu_equals(t, off, ref, what):
    import mhm2_proxy_amd as m
    pb, po, pst = ref
    with m.KmerCounter(21, device=0, qual_offset=off) as cnt:
        cnt.add_fastq_pairs(t)
        gb, go = cnt.fastq_packed()
        st = cnt.stats()
    assert len(go) == len(po) and (go == po).all(), what
    bad = np.flatnonzero(gb != pb)
    if bad.size:  # name the first read that differs
        r = int(np.searchsorted(po, bad[0], side="right")) - 1
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first in read {r} (pair {r // 2}) at base "
                             f"{int(bad[0] - po[r])}: {int(gb[bad[0]])} != {int(pb[bad[0]])}")
    for key in ("pairs", "merged", "ambiguous", "overlap_bases"):
        assert st["fq_" + key] == pst[key], (what, key, st["fq_" + key], pst[key])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["listed", "shuffled"])
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("grid", GRIDS)
def test_gpu_cases_equal_oracle(grid, off, order, knob):
    """The whole case list as one batch. merge_grid 0: one pair per wave; 1 and 3: a wave takes every 4th / 12th pair.
    (The grid varies slowest, so that consecutive calls differ in their output: bytes that a call fails to write
    cannot be right because the call before it left them in the same buffer.)"""
    knob("merge_grid", grid)
    t, ref = _batch(off, order)
    _assert_gpu_equals(t, off, ref, f"offset {off} {order} merge_grid={grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
def test_gpu_turns_equal_oracle(grid, knob):
    """merge_cases.turn_cases: runs of 12 pairs of a kind. A wave of a capped grid takes the pairs w, w + S, w + 2S,
    ... with S = 4 (merge_grid 1) or S = 12 (merge_grid 3); a run being 12 = 3 * 4 = 1 * 12 long, every wave of
    either grid meets every kind, in the list's order: long then short, N then none, a 504-base mate then a 30-base
    one, merged then unmerged. (The long instance of k_fq_merge takes its pairs in the order the long-pair list was
    filled in, which is not fixed; its three kinds of 12 pairs share its 4 or 12 waves.) The results must equal the
    oracle's, and so those of the default grid."""
    knob("merge_grid", grid)
    t, ref = _turns()
    _assert_gpu_equals(t, 33, ref, f"turns merge_grid={grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("grid", (0, 1))
def test_gpu_output_alignments(grid, knob):
    """put_run at every alignment of the merged reads and the unmerged mates 2 around its 256-byte steps (the batch of
    test_alignment_cases_cover_every_alignment, which starts at output byte 0)."""
    knob("merge_grid", grid)
    t, ref = _aligned()
    _assert_gpu_equals(t, 33, ref, f"alignments merge_grid={grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", range(len(ERR_CASES)), ids=[c.name for c in ERR_CASES])
def test_gpu_quality_errors(n, off):
    """Each bad-quality pair in a call of its own, after two clean pairs: the error code and the record numbers."""
    import mhm2_proxy_amd as m
    t = M.fastq_text([_ok_pair(0), _ok_pair(1), ERR_CASES[n]], off)
    with m.KmerCounter(21, device=0, qual_offset=off) as cnt:
        with pytest.raises(m.MhmkcError) as got:
            cnt.add_fastq_pairs(t)
    msg = str(got.value)
    assert msg.startswith("MHMKC_EINVAL") and "records 4 and 5: invalid quality" in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("grid", (1, 3))
@pytest.mark.parametrize("variant", ["default", "many_n"])
def test_gpu_random_pairs_capped_grid(variant, grid, knob):
    """Two of test_fastq_pairs' random variants with a wave taking 375 (125) pairs in turn."""
    knob("merge_grid", grid)
    t, off = P._text(variant, 1500)
    _assert_gpu_equals(t, off, O.merge_fastq(t, off), f"{variant} merge_grid={grid}")


def test_merge_grid_is_a_knob():
    from mhm2_proxy_amd import _native as N
    L = N.lib()
    assert L.mhmkc_debug_set(b"merge_grid", 3) == 0 and L.mhmkc_debug_set(b"merge_grid", 0) == 0
