"""Constructed read pairs for the merge (merge_reads, src/merge_reads.cpp:237-588): every pair is built from chosen
bases and qualities so that the reference's offset loop takes one named path, which the random pairs of
common.paired_fastq_text reach by accident or not at all. TEST INFRASTRUCTURE ONLY.

A pair is laid out in the frame the loop works in: mate 1 (s1, q1) and mate 2 reverse-complemented (rc, rq), so that
offset i compares s1[start_i + i + j] with rc[j]. Frame.mates() turns that back into the two FASTQ records. Every case
carries `expect`, the structure it is meant to hit, in terms of ref_merge_literal.merge_pair's trace; check_case()
asserts it. Qualities at N and mismatch positions are 1..30 above the offset, so that a quality the scan rewrites (or
must not rewrite) shows in the PackedRead byte (qualities above 31 clamp there).

Constants of the reference used below: overlap o has this_max_mismatch tmax(o) = 3 + 150 o / 1000, error_max_mismatch
emax(o) = tmax * 4 / 3 + 1, match_thres = max(o - tmax, 12); offsets are scanned down to overlap 11."""
from __future__ import annotations

from dataclasses import dataclass, field

import ref_merge_literal as R

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def tmax(o: int) -> int:
    return 3 + 150 * o // 1000


def emax(o: int) -> int:
    return tmax(o) * 4 // 3 + 1


def bases(n: int, seed: int) -> str:
    """n fixed background bases without structure (a 32-bit linear congruential sequence, its top bits)."""
    x = (seed * 2654435761 + 12345) % 2 ** 32
    out = []
    for _ in range(n):
        x = (x * 1664525 + 1013904223) % 2 ** 32
        out.append("ACGT"[x >> 30])
    return "".join(out)


class Frame:
    """A pair under construction: s1 / q1 and rc / rq (qualities as numbers above the offset); p0 is the s1 index that
    rc[0] is meant to align with, so position j of the intended overlap is (s1[p0 + j], rc[j])."""

    def __init__(self, s1: str, rc: str, p0: int = 0, q: int = 40):
        self.s1, self.rc, self.p0 = list(s1), list(rc), p0
        self.q1, self.rq = [q] * len(s1), [q] * len(rc)

    @property
    def len(self) -> int:
        return min(len(self.s1), len(self.rc))

    @property
    def start_i(self) -> int:
        return 0 if self.len == len(self.s1) else len(self.s1) - self.len

    @property
    def i0(self) -> int:  # the offset of the intended overlap
        return self.p0 - self.start_i

    @property
    def ov(self) -> int:
        return self.len - self.i0

    def mm(self, j: int, q1: int = 30, q2: int = 4) -> "Frame":
        """a plain mismatch at overlap position j; by default a large quality difference, i.e. a small perror term"""
        self.rc[j] = _OTHER[self.s1[self.p0 + j]]
        self.q1[self.p0 + j], self.rq[j] = q1, q2
        return self

    def flip(self, j: int, q: int = 20) -> "Frame":
        """a mismatch with equal qualities: perror += 0.5"""
        return self.mm(j, q, q)

    def n1(self, j: int, q: int, q2: int = 40) -> "Frame":
        """N in mate 1 against a base"""
        self.s1[self.p0 + j] = "N"
        self.q1[self.p0 + j], self.rq[j] = q, q2
        return self

    def n2(self, j: int, q: int, q1: int = 40) -> "Frame":
        """N in mate 2 against a base"""
        self.rc[j] = "N"
        self.rq[j], self.q1[self.p0 + j] = q, q1
        return self

    def both(self, j: int, q1: int = 7, q2: int = 9) -> "Frame":
        self.s1[self.p0 + j] = self.rc[j] = "N"
        self.q1[self.p0 + j], self.rq[j] = q1, q2
        return self

    def mates(self, off: int):
        """(seq1, quals1, seq2, quals2) as they stand in the FASTQ text; a negative quality is below the offset"""
        s2 = "".join(_COMP[c] for c in reversed(self.rc))
        return ("".join(self.s1), "".join(chr(off + q) for q in self.q1), s2,
                "".join(chr(off + q) for q in reversed(self.rq)))


def full(L: int, seed: int) -> Frame:
    b = bases(L, seed)
    return Frame(b, b)


def partial(L1: int, L2: int, ov: int, seed: int) -> Frame:
    """mate 1's last ov bases are rc's first ov, the rest is unrelated"""
    a = bases(L1, seed)
    return Frame(a, a[L1 - ov:] + bases(L2 - ov, seed + 7919), p0=L1 - ov)


def unrelated(L1: int, L2: int, seed: int) -> Frame:
    return Frame(bases(L1, seed), bases(L2, seed + 7919))


@dataclass
class Case:
    name: str
    frame: Frame
    expect: dict = field(default_factory=dict)
    only33: bool = False  # a quality >= 81 that ends up in the output: a character past 127 at offset 64
    # expect: "scan" {offset: fields the trace's scan at that offset must show}, "verdicts" [(offset, verdict)] every
    # scan with a verdict, in order, "absent" [offsets the fast filter must drop], "exit", "merged", "overlap", "amb",
    # "error" (the quality DIE), "no_scans", "q1" / "q2" {index: quality above the offset} of the output reads 0 / 1,
    # "lens" the output lengths

    def mates(self, off: int):
        return self.frame.mates(off)


def fastq_text(cases, off: int = 33) -> bytes:
    out = []
    for n, c in enumerate(cases):
        s1, q1, s2, q2 = c.mates(off)
        out.append(f"@{c.name}.{n}/1\n{s1}\n+\n{q1}\n@{c.name}.{n}/2\n{s2}\n+\n{q2}\n")
    return "".join(out).encode("latin-1")


def run_case(c: Case, off: int):
    """-> (trace, result or None where the reference DIEs)"""
    tr: dict = {}
    try:
        res = R.merge_pair(*c.mates(off), off, trace=tr)
    except ValueError:
        res = None
    return tr, res


def check_case(c: Case, off: int = 33):
    """Asserts that the literal restatement takes the path the case was built for."""
    tr, res = run_case(c, off)
    e, what = c.expect, f"{c.name} (offset {off})"
    scans = {s["i"]: s for s in tr["scans"]}
    assert tr["len"] == c.frame.len and tr["start_i"] == c.frame.start_i, what
    if e.get("no_scans"):
        assert not tr["scans"], what
    for i, want in e.get("scan", {}).items():
        assert i in scans, (what, i, sorted(scans))
        got = {k: scans[i][k] for k in want}
        assert got == want, (what, i, got, want)
    for i in e.get("absent", ()):
        assert i not in scans, (what, i)
    if "verdicts" in e:
        assert [(s["i"], s["verdict"]) for s in tr["scans"] if s["verdict"]] == e["verdicts"], what
    if e.get("error"):
        assert res is None, what
        assert tr["scans"][-1]["break"] == "quality", what
        return tr, res
    assert res is not None, what
    reads, merged, amb, ov = res
    assert tr["exit"] == e.get("exit"), (what, tr["exit"])
    assert merged == e["merged"] and amb == e.get("amb", 0) and ov == e.get("overlap", 0), (what, merged, amb, ov)
    if "lens" in e:
        assert [len(s) for s, _ in reads] == list(e["lens"]), what
    for r, key in ((0, "q1"), (1, "q2")):
        for x, q in e.get(key, {}).items():
            assert ord(reads[r][1][x]) - off == q, (what, key, x, ord(reads[r][1][x]) - off, q)
    return tr, res


# ---------------------------------------------------------------------------------------------------------------------
# chunk and lane edges of the scan: mates of 150, full overlap (three 64-position chunks), tmax 25, emax 34


def _both_n2(P):
    f = full(150, 100 + P).both(10).both(P, 5, 6)
    return Case(f"bothN2_at_{P}", f, {
        "scan": {0: {"break": "bothN2", "break_j": P, "matches": P + 1, "mismatches": 0}},
        "verdicts": [], "exit": "abort", "merged": False, "amb": 1, "q1": {10: 7, P: 5}, "q2": {149 - P: 6}})


def _many_n(P):
    f = full(150, 200 + P).n1(5, 11).n2(20, 12).n1(40, 13).n1(P, 14, q2=29)
    last = P == 149  # the reference breaks at the last position too; overlapChecked == overlap, so the verdict is good
    return Case(f"manyN_at_{P}", f, {
        "scan": {0: {"break": "manyN", "break_j": P, "matches": P + 1 - 4, "mismatches": 8}},
        "verdicts": [(0, "good")] if last else [], "exit": "abort", "merged": False, "amb": 1,
        "q1": {5: 0, 40: 0, P: 0, 20: 40}, "q2": {149 - 20: 12, 149 - P: 29}})


def _mm_positions(P):
    """32 positions up to P, every second one, P the last"""
    return [P - 2 * k for k in range(31, -1, -1)]


def _mm_break(P):
    """31 plain mismatches and three N mismatches: 34 == emax for the fast filter, 37 for the scan, which counts an N
    twice and passes 34 exactly at P (3 N + 28 plain before it, 35 with the one at P); two plain ones follow"""
    pos = _mm_positions(P)
    f = full(150, 300 + P).n1(pos[0], 11).n2(pos[1], 12).n1(pos[2], 13)
    for j in pos[3:] + [P + 3, P + 7]:
        f.mm(j)
    return Case(f"mmbreak_at_{P}", f, {
        "scan": {0: {"break": "mismatch", "break_j": P, "mismatches": 35, "matches": P + 1 - 32}},
        "exit": None, "merged": False, "amb": 0, "q1": {pos[0]: 0, pos[2]: 0, pos[3]: 30},
        "q2": {149 - pos[1]: 12}})


def _bad_q(name, j, side, q, seed, pre=None):
    """a mismatch at position j whose quality on one side is q (>= 81, or negative: below the offset)"""
    f = full(150, seed)
    if pre:
        pre(f)
    f.mm(j, q if side == 1 else 30, q if side == 2 else 30)
    return Case(name, f, {"error": True, "scan": {0: {"break": "quality", "break_j": j}}})


def edge_cases():
    out = [_both_n2(P) for P in (63, 64, 127, 128)]
    out += [_many_n(P) for P in (63, 64, 127, 128, 149)]
    out += [_mm_break(P) for P in (63, 64, 127, 128)]
    # two events in one chunk (64..127): the first lane wins
    f = full(150, 401).both(10).both(80, 5, 6).mm(90, 85, 30)
    out.append(Case("bothN2_then_badq", f, {"scan": {0: {"break": "bothN2", "break_j": 80}}, "verdicts": [],
                                            "exit": "abort", "merged": False, "amb": 1}, only33=True))
    # the fourth N and too many mismatches at one position: the N rule is checked first (:408 before :413), an abort.
    # 3 N + 27 plain = 33 before P, the fourth N at P makes 35 > 34; the filter sees 31
    P = 100
    pos = [P - 2 * k for k in range(30, -1, -1)]
    f = full(150, 402).n1(pos[0], 11).n2(pos[1], 12).n1(pos[2], 13)
    for j in pos[3:-1]:
        f.mm(j)
    f.n1(P, 14)
    out.append(Case("manyN_and_mismatches_same_position", f, {
        "scan": {0: {"break": "manyN", "break_j": P, "mismatches": 35}}, "verdicts": [], "exit": "abort",
        "merged": False, "amb": 1, "q1": {P: 0}}))
    # N mismatches after an abort in the same chunk: those up to the break become the offset, the later ones stay as
    # read; mate 2 comes out as read throughout (rev_quals2 is a copy)
    f = full(150, 403).n1(65, 11).n2(67, 12).n1(69, 13).n1(72, 14).n1(73, 15).n2(74, 16).n1(100, 17).n2(101, 18)
    out.append(Case("N_after_abort_same_chunk", f, {
        "scan": {0: {"break": "manyN", "break_j": 72}}, "verdicts": [], "exit": "abort", "merged": False, "amb": 1,
        "q1": {65: 0, 69: 0, 72: 0, 73: 15, 100: 17, 67: 40}, "q2": {149 - 67: 12, 149 - 74: 16, 149 - 101: 18}}))
    # the same after a plain mismatch break (at 72: 3 N + 28 plain before it): the scan of offset 0 leaves the later N
    # at 75 as read, but the loop goes on, and offset 139 (overlap 11: mate 1's tail repeats its head) scans the N at
    # 145 and rewrites it. The filter of offset 0 sees 32 + 2 N = 34 == emax.
    b = bases(139, 404)
    b = b + b[:11]
    f = Frame(b, b)
    pos = _mm_positions(72)
    f.n1(pos[0], 11).n2(pos[1], 12).n1(pos[2], 13)
    for j in pos[3:]:
        f.mm(j)
    f.n1(75, 15).n1(145, 16)
    out.append(Case("N_after_mismatch_break", f, {
        "scan": {0: {"break": "mismatch", "break_j": 72, "mismatches": 35},
                 139: {"break": None, "mismatches": 2, "matches": 10, "verdict": "weak"}},
        "verdicts": [(139, "weak")], "exit": None, "merged": False, "amb": 0,
        "q1": {pos[0]: 0, pos[2]: 0, 75: 15, 145: 0}, "q2": {149 - pos[1]: 12}}))
    return out


def quality_error_cases():
    """Each is its own call: the reference DIEs (:392-396). (A quality below the offset is a control character or a
    space at offset 33, which the end of a line would lose to the trimming of trailing white space: none is last.)"""
    def three_n(f):  # the position of the bad quality is also the fourth N's (:392 is reached before :408)
        f.n1(5, 11).n2(20, 12).n1(40, 13)

    out = [_bad_q("badq_high_chunk1_mate1", 70, 1, 81, 501), _bad_q("badq_low_chunk1_mate2", 127, 2, -2, 502),
           _bad_q("badq_high_chunk2_mate2", 128, 2, 90, 503), _bad_q("badq_low_chunk2_mate1", 148, 1, -2, 504),
           _bad_q("badq_then_bothN2", 80, 1, 85, 505, pre=lambda f: f.both(10).both(90))]
    f = full(150, 506)
    three_n(f)
    f.n1(100, 14, q2=81)
    out.append(Case("manyN_and_badq_same_position", f, {"error": True, "scan": {0: {"break": "quality", "break_j": 100}}}))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# verdict bookkeeping: a second hit after a first


def _periodic(period, L, seed):
    u = bases(period, seed)
    return (u * (L // period + 1))[:L]


def verdict_cases():
    out = []
    for tag, period, L in (("same_group", 20, 100), ("next_group", 80, 200)):  # second hit at offset 20 / 80
        o2 = L - period
        # good then good: a tandem repeat
        b = _periodic(period, L, 600 + period)
        out.append(Case(f"good_then_good_{tag}", Frame(b, b), {
            "verdicts": [(0, "good"), (period, "good")], "exit": "good_again", "merged": False, "amb": 1}))
        # weak then good: six coin-flip mismatches in rc's last `period` bases, which only offset 0 compares with
        # anything: perror 3.0 is above 0.025 L and at most L / 30
        f = Frame(b, b)
        for j in range(6 if L == 100 else 11):
            f.flip(L - 2 - 3 * j)
        out.append(Case(f"weak_then_good_{tag}", f, {
            "verdicts": [(0, "weak"), (period, "good")], "exit": "good_again", "merged": False, "amb": 1}))
        # good then weak: mate 2 == mate 1, so offset 0 is clean; the repeat is broken in mate 1 AND mate 2 alike at a
        # few positions: one in [period, L - period) costs offset `period` two mismatches, one outside it one
        b2 = list(b)
        breaks = (30, 55, 90) if L == 100 else (85, 100, 115, 150)  # 2 + 2 + 1 = 5 of 80; 2 + 2 + 2 + 1 = 7 of 120
        for p in breaks:
            b2[p] = _OTHER[b2[p]]
        f = Frame(b2, b2, q=25)  # (equal qualities: every mismatch is a coin flip)
        n = 5 if L == 100 else 7
        out.append(Case(f"good_then_weak_{tag}", f, {
            "scan": {period: {"mismatches": n, "perror": 0.5 * n, "overlap": o2}},
            "verdicts": [(0, "good"), (period, "weak")], "exit": "weak_after_good", "merged": False, "amb": 1}))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# thresholds, exactly at and one off


ORDER_TERMS = (4, 5, 6, 10, 11, 16, 17, 20)  # quality differences; see order_sum_cases


def order_sum_cases():
    """Eight different Q2Perror terms whose decimal sum is 1.2 = 0.025 * 48. Added in this order the double sum is 1.2
    and 1.2 / 48 <= 0.025: good, merged. Added in the reverse order it is 1.2000000000000002: weak. The reference adds
    in position order, so the two cases differ only in where the mismatches stand."""
    out = []
    for tag, terms in (("ascending", ORDER_TERMS), ("descending", ORDER_TERMS[::-1])):
        f = partial(150, 150, 48, 700)
        for n, d in enumerate(terms):
            f.mm(3 + 5 * n, 30, 30 - d)
        good = tag == "ascending"
        out.append(Case(f"perror_order_{tag}", f, {
            "scan": {102: {"mismatches": 8, "matches": 40}}, "verdicts": [(102, "good" if good else "weak")],
            "exit": None, "merged": good, "overlap": 48 if good else 0}))
    return out


def _ov_case(name, ov, n_mm, verdict, seed, flips=0, L=150):
    """overlap ov at the end of two mates of L, n_mm plain mismatches with small perror terms and `flips` coin flips"""
    f = partial(L, L, ov, seed)
    for n in range(n_mm):
        f.mm(1 + n * (ov - 2) // max(n_mm, 1))
    for n in range(flips):
        f.flip(ov - 1 - 2 * n)
    i = L - ov
    e = {"verdicts": [(i, verdict)] if verdict else [], "exit": None, "merged": verdict == "good",
         "overlap": ov if verdict == "good" else 0}
    if n_mm + flips <= emax(ov):
        e["scan"] = {i: {"mismatches": n_mm + flips, "matches": ov - n_mm - flips, "break": None}}
    else:
        e["absent"] = [i]
    return Case(name, f, e)


def threshold_cases():
    out = []
    # overlap 100: tmax 18, emax 25, match_thres 82
    f = full(100, 801)
    for n in range(18):
        f.mm(2 + 5 * n)
    out.append(Case("mm_eq_tmax_matches_eq_thres", f, {
        "scan": {0: {"mismatches": 18, "matches": 82}}, "verdicts": [(0, "good")], "merged": True, "overlap": 100,
        "q1": {2: 26}}))
    f = full(100, 802)
    for n in range(17):
        f.mm(2 + 5 * n)
    f.n1(90, 11)  # 18 positions: matches == match_thres, but the N counts twice: mismatches == tmax + 1
    out.append(Case("mm_eq_tmax_plus_1_by_N", f, {
        "scan": {0: {"mismatches": 19, "matches": 82}}, "verdicts": [(0, "weak")], "merged": False, "q1": {90: 0}}))
    f = full(100, 803)
    for n in range(16):
        f.mm(2 + 5 * n)
    f.n2(90, 11)
    out.append(Case("mm_eq_tmax_by_N", f, {
        "scan": {0: {"mismatches": 18, "matches": 83}}, "verdicts": [(0, "good")], "merged": True, "overlap": 100}))
    f = full(100, 804)
    for n in range(25):
        f.mm(1 + 3 * n)
    out.append(Case("mm_eq_emax", f, {"scan": {0: {"mismatches": 25, "break": None}}, "verdicts": [(0, "weak")],
                                     "merged": False}))
    f = full(100, 805)
    for n in range(23):
        f.mm(1 + 3 * n)
    f.n1(95, 11)
    out.append(Case("mm_eq_emax_by_N", f, {"scan": {0: {"mismatches": 25, "break": None}}, "verdicts": [(0, "weak")],
                                          "merged": False, "q1": {95: 0}}))
    f = full(100, 806)
    for n in range(24):
        f.mm(1 + 3 * n)
    f.n1(99, 11)  # 25 for the filter, 26 for the scan, at its last position
    out.append(Case("mm_eq_emax_plus_1_by_N", f, {
        "scan": {0: {"mismatches": 26, "break": "mismatch", "break_j": 99}}, "verdicts": [], "merged": False,
        "q1": {99: 0}}))
    # match_thres clamped to 12 (overlap 15: tmax 5, 15 - 5 < 12): matches alone decide
    out.append(_ov_case("matches_eq_thres_ov15", 15, 3, "good", 811))
    out.append(_ov_case("matches_eq_thres_minus_1_ov15", 15, 4, "weak", 812))
    # overlap 12 is the shortest that can be good, 11 the shortest scanned
    out.append(_ov_case("overlap_12", 12, 0, "good", 813))
    out.append(_ov_case("overlap_11", 11, 0, "weak", 814))
    # the steps of 150 * overlap / 1000 (overlaps 6 / 7 are never scanned: 11 is the shortest)
    out.append(_ov_case("step_ov13_mm_eq_emax", 13, 6, "weak", 821))
    out.append(_ov_case("step_ov13_mm_emax_plus_1", 13, 7, None, 822))  # (the fast filter drops it)
    out.append(_ov_case("step_ov14_mm_eq_emax", 14, 7, "weak", 823))
    out.append(_ov_case("step_ov19_mm_eq_tmax", 19, 5, "good", 824))
    out.append(_ov_case("step_ov19_mm_tmax_plus_1", 19, 6, "weak", 825))
    out.append(_ov_case("step_ov20_mm_eq_tmax", 20, 6, "good", 826))
    out.append(_ov_case("step_ov26_mm_eq_tmax", 26, 6, "good", 827))
    out.append(_ov_case("step_ov26_mm_tmax_plus_1", 26, 7, "weak", 828))
    out.append(_ov_case("step_ov27_mm_eq_tmax", 27, 7, "good", 829))
    # perror / overlap exactly at its limits, one coin flip: 0.5 / 20 == 0.025; 0.5 / 15 == 0.025 * 4 / 3 in double
    out.append(_ov_case("perror_eq_limit_ov20", 20, 0, "good", 831, flips=1))
    out.append(_ov_case("perror_above_limit_ov19", 19, 0, "weak", 832, flips=1))
    out.append(_ov_case("perror_eq_weak_limit_ov15", 15, 0, "weak", 833, flips=1))
    out.append(_ov_case("perror_above_weak_limit_ov14", 14, 0, None, 834, flips=1))
    return out + order_sum_cases()


# ---------------------------------------------------------------------------------------------------------------------
# lengths


def length_cases():
    out = []
    for n in (1, 2, 3, 4, 9, 10, 11, 12):
        # the short mate is the other one's end (mate 2 short: start_i = 150 - n) or start (mate 1 short)
        for side, f in (("mate2", partial(150, n, n, 900 + n)), ("mate1", partial(n, 150, n, 920 + n))):
            assert f.i0 == 0 and f.start_i == (150 - n if side == "mate2" else 0)
            unmerged = (150, n) if side == "mate2" else (n, 150)
            if n <= 10:  # len - MIN_OVERLAP + EXTRA_TEST_OVERLAP <= 0: no offset is tested
                e = {"no_scans": True, "merged": False, "lens": unmerged}
            elif n == 11:
                e = {"verdicts": [(0, "weak")], "merged": False, "lens": unmerged}
            else:
                e = {"verdicts": [(0, "good")], "merged": True, "overlap": 12, "lens": (150, 1)}
            out.append(Case(f"len_{n}_{side}_short", f, e))
    # around MG_LONG (504): the short-staging instance takes mates up to 504, the long one the rest
    for L in (503, 504, 505, 506):
        for tag, L1, L2 in (("mate1", L, 150), ("mate2", 150, L), ("both", L, L)):
            f = partial(L1, L2, 100, 940 + L)
            i = f.i0
            out.append(Case(f"long_{L}_{tag}", f, {"verdicts": [(i, "good")], "merged": True, "overlap": 100,
                                                   "lens": (L1 + L2 - 100, 1)}))
    # the longest line (2045)
    out.append(Case("len_2045_full", full(2045, 950).mm(1000).mm(2044), {
        "verdicts": [(0, "good")], "merged": True, "overlap": 2045, "lens": (2045, 1)}))
    out.append(Case("len_2045_partial", partial(2045, 2045, 1000, 951).n1(999, 11), {
        "verdicts": [(1045, "good")], "merged": True, "overlap": 1000, "lens": (3090, 1)}))
    return out


ALIGN_LENS = tuple(range(253, 261)) + tuple(range(509, 517))


def alignment_cases():
    """Merged reads of 253..260 and 509..516 bases (around put_run's 256-byte steps), and unmerged mates 2 of those
    lengths, each starting at every output alignment: the cases are in batch order, a small unmerged filler pair before
    a case where needed sets the alignment by the lengths of the reads before it. -> (cases, [(kind, length,
    alignment, index of the case in the list)])"""
    cases, want, pos = [], [], 0

    def pad(target):  # a filler of f + 1 output bytes, f in 1..4
        nonlocal pos
        d = (target - pos) % 4
        if d:
            f = (d - 1) if d > 1 else 4
            cases.append(Case("filler", unrelated(f, 1, 1000 + f), {"no_scans": True, "merged": False, "lens": (f, 1)}))
            pos += f + 1

    for M in ALIGN_LENS:
        for a in range(4):
            L = 150 if M < 400 else 300
            pad(a)
            want.append(("merged", M, a, len(cases)))
            f = partial(L, L, 2 * L - M, 1100 + M)
            cases.append(Case(f"merged_{M}_align{a}", f, {"verdicts": [(f.i0, "good")], "merged": True,
                                                          "overlap": 2 * L - M, "lens": (M, 1)}))
            pos += M + 1
    for M in ALIGN_LENS:
        for a in range(4):
            pad(a - 100)
            want.append(("mate2", M, a, len(cases)))
            cases.append(Case(f"mate2_{M}_align{a}", unrelated(100, M, 1200 + M),
                              {"verdicts": [], "merged": False, "lens": (100, M)}))
            pos += 100 + M
    return cases, want


def all_cases(off: int = 33):
    """Every case that merges or not without an error, in a fixed order (the quality errors are calls of their own)."""
    cs = edge_cases() + verdict_cases() + threshold_cases() + length_cases() + alignment_cases()[0]
    return [c for c in cs if off == 33 or not c.only33]


TURN_COPIES = 12


def _clean(name, f):
    return Case(name, f, {"verdicts": [(f.i0, "good")], "merged": True, "overlap": f.ov})


def turn_cases():
    """For the capped grids: runs of TURN_COPIES pairs of one kind each, so that with a stride of 4 waves (merge_grid 1)
    and of 12 (merge_grid 3) alike every wave meets the kinds in this order: with stride 12 one pair of each kind in
    turn, with stride 4 three of a kind and then the next kind. Each kind differs from the one before it in what a
    wave could carry over: a long pair then a short one, N then none, a long mate then a much shorter one (the code and
    flag words past the shorter pair's end are the longer one's), merged then unmerged."""
    by = {c.name: c for c in edge_cases() + length_cases()}
    kinds = [
        by["len_2045_full"],                                               # long instance; merged
        _clean("short_merged", partial(150, 150, 60, 1301)),
        by["manyN_at_128"],                                                # N, unmerged, rewritten qualities
        Case("no_N_unmerged", unrelated(150, 150, 1302), {"verdicts": [], "merged": False}),
        by["long_504_both"],                                               # the longest short-instance mates; merged
        _clean("short_30", partial(30, 30, 20, 1303)),
        by["N_after_mismatch_break"],                                      # N, unmerged, a weak hit
        by["long_506_both"],                                               # long instance again
        by["len_12_mate1_short"],                                          # merged, 12 against 150
        by["bothN2_at_64"],                                                # N, abort
        by["len_3_mate2_short"],                                           # no offsets at all
        _clean("short_merged_2", partial(150, 140, 75, 1304)),
    ]
    return [k for k in kinds for _ in range(TURN_COPIES)]
