"""Constructed inputs that put the eight extension counters of one hot k-mer at exact values next to the levels where
k_count's 16-bit LDS counters change their treatment: 0x8000 (the clamp's target), HOT (the count from
which a lane checks the clamp), 0xC000 (the clamp level), 65535 (the reference's saturation) and a second climb to the
clamp, crossed with every kind of (dyn_min_depth, dmin_thres) the library accepts. TEST INFRASTRUCTURE ONLY.

An input is a multiset of records {(left, right): n} of one key, left and right in "ACGTN" (N: no countable neighbour),
so its counters are arithmetic: count = min(sum n, 65535), left[x] = min(sum of n over (x, .), 65535), right alike
(ExtCounts::inc saturates every counter at 65535, kcount_cpu.cpp:148-164). row() is the reference's decision on such
counters, written out literally; tests/test_saturation.py asserts that it equals the CPU oracle's row for every input.

Two keys carry the records: A^k (its A/A records come from long poly-A reads, up to 400 records per read) and a fixed
random S, given alternately as S and as its reverse complement, so that the swap-and-complement of the extension codes
runs at saturation too. Every other record is a read `X key Y` of length k + 2.

A case is (input, key, dyn_min_depth, dmin_thres). near() names the decisions it sits next to: the transitions that one
step of one counter (or of the count) would cross. Only cases that discriminate are kept: those with such a neighbour,
and those whose row changes when a counter past the clamp level is read as the clamp's target or one below it."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from merge_cases import bases

Q31 = 31 << 3  # PackedRead quality bits
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
SAT = 65535
CLAMP_AT, CLAMP_TO = 0xC000, 0x8000  # ext_clamp, mhm2_proxy_amd/csrc/kcount_kernels.hip

# The build constants of k_count per record kind (kcount_kernels.hip, kcount_launch.hpp): a round's records RND =
# count_rpt * C_THREADS, the miss space miss_cap(NL, compact), and HOT = 0xC000 - 2 (RND + miss_cap), the count from
# which a lane that added to a slot checks the slot's halves for the clamp.
C_THREADS = 1024
RND = {"compact": 4 * C_THREADS, "wide1": 4 * C_THREADS, 2: C_THREADS, 3: C_THREADS, 4: C_THREADS}
MISS_CAP = {"compact": 1984, "wide1": 1664, 2: 960, 3: 704, 4: 512}
HOT = {kind: CLAMP_AT - 2 * (RND[kind] + MISS_CAP[kind]) for kind in RND}


def record_kind(k: int, wide: bool = False):
    """compact (k <= 21), wide1 (one 64-bit key word: the wide_records knob at k <= 21, or 21 < k < 32), else the key
    words."""
    if k < 32:
        return "wide1" if wide or k > 21 else "compact"
    return k // 32 + 1


PARAMS = [(0.9, 2), (0.9, 32768), (0.9, 32767), (0.5, 2), (0.49, 2), (0.25, 2), (0.0, 2), (0.0, 0), (1.0, 2)]


def threshold(count: int, dyn: float, dmin: int) -> int:
    return max(int((1.0 - dyn) * count), dmin)


def get_ext(cnt, count: int, dyn: float, dmin: int) -> str:
    """ExtCounts::get_ext (kcount_cpu.cpp:173-182) on counters cnt = [A, C, G, T] (a tie at the top is 'F' or 'X')."""
    thr = threshold(count, dyn, dmin)
    top, second = sorted(cnt, reverse=True)[:2]
    if top < thr:
        return "X"
    if second >= thr:
        return "F"
    return "ACGT"[list(cnt).index(top)]


def counters(recs: dict):
    """(count, left[4], right[4]) of an input, each saturated at 65535."""
    left, right = [0] * 4, [0] * 4
    for (lx, rx), n in recs.items():
        if lx != "N":
            left[CODE[lx]] += n
        if rx != "N":
            right[CODE[rx]] += n
    return min(sum(recs.values()), SAT), [min(v, SAT) for v in left], [min(v, SAT) for v in right]


def decide(count, left, right, dyn, dmin):
    """The table row (count, left, right) of such counters, or None when the k-mer is purged
    (insert_into_local_hashtable, kcount_cpu.cpp:503-517: count < 2, or 'X' on both sides)."""
    if count < 2:
        return None
    lc, rc = get_ext(left, count, dyn, dmin), get_ext(right, count, dyn, dmin)
    return None if lc == rc == "X" else (count, lc, rc)


def row(recs: dict, dyn: float, dmin: int):
    return decide(*counters(recs), dyn, dmin)


def _kind(a: str, b: str) -> str:
    order = {"X": 0, "F": 2}
    lo, hi = sorted((a, b), key=lambda c: order.get(c, 1))
    return f"{'X' if lo == 'X' else 'base'}>{'F' if hi == 'F' else 'base'}"


def near(recs: dict, dyn: float, dmin: int) -> set:
    """The transitions next to the case: "X>base", "base>F" and "X>F" (one side's choice changes when its largest or
    second-largest counter, or the count, moves by one) and "kept>purged" (the row appears or disappears)."""
    count, left, right = counters(recs)
    base = decide(count, left, right, dyn, dmin)
    out = set()
    variants = []
    for side in (0, 1):
        cnt = (left, right)[side]
        order = sorted(range(4), key=lambda i: -cnt[i])
        for i in order[:2]:
            for d in (-1, 1):
                if 0 <= cnt[i] + d <= SAT:
                    c2 = list(cnt)
                    c2[i] += d
                    variants.append((count, c2, right) if side == 0 else (count, left, c2))
    lo, ro = (sorted(range(4), key=lambda i: -c[i]) for c in (left, right))
    for j in (0, 1):  # one record more or less of a pair: the same step on both sides
        for d in (-1, 1):
            l2, r2 = list(left), list(right)
            l2[lo[j]] += d
            r2[ro[j]] += d
            if 0 <= l2[lo[j]] <= SAT and 0 <= r2[ro[j]] <= SAT:
                variants.append((count, l2, r2))
    for d in (-1, 1):
        if 2 <= count + d <= SAT:
            variants.append((count + d, left, right))
    for v in variants:
        other = decide(*v, dyn, dmin)
        if (other is None) != (base is None):
            out.add("kept>purged")
        for side in (1, 2):
            a = get_ext(*((left, right)[side - 1],), count, dyn, dmin)
            b = get_ext(v[side], v[0], dyn, dmin)
            if a != b and {a, b} & {"X", "F"}:
                out.add(_kind(a, b))
    return out


# ---- the two keys and their reads ------------------------------------------------------------------------------------

def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


@lru_cache(maxsize=None)
def key_string(key: str, k: int) -> str:
    """"A": A^k. "S": k fixed bases without structure, in their canonical orientation (S < revcomp(S), so that the
    table's row carries S itself and a read of revcomp(S) has its extensions swapped and complemented)."""
    if key == "A":
        return "A" * k
    s = bases(k, 9001 + k)
    assert s != revcomp(s)
    return min(s, revcomp(s))


# the pair of extensions that carries an input's main counter, the one of its runner-up, and a third
MAJOR = {"A": ("A", "A"), "S": ("G", "T")}
MINOR = {"A": ("C", "G"), "S": ("A", "C")}


def _rows(key_s: str, lx: str, rx: str, n: int, start: int, alternate: bool) -> np.ndarray:
    """n reads `lx key rx` as an (n, k + 2) byte array; with alternate, occurrence start + i is given as the reverse
    complement when odd."""
    fwd = np.array([CODE[c] for c in lx + key_s + rx], dtype=np.uint8) | np.uint8(Q31)
    out = np.tile(fwd, (n, 1))
    if alternate:
        rev = np.array([CODE[c] for c in COMP[rx] + revcomp(key_s) + COMP[lx]], dtype=np.uint8) | np.uint8(Q31)
        out[(np.arange(n) + start) % 2 == 1] = rev
    return out


def reads(recs: dict, key: str, k: int):
    """The reads of an input as a list of per-read byte arrays, its record kinds mixed in a fixed order."""
    key_s = key_string(key, k)
    recs = {p: n for p, n in recs.items() if n}
    bulk = []
    if key == "A" and ("A", "A") in recs:
        t = recs.pop(("A", "A"))
        while t > 0:
            step = min(t, 400)
            bulk.append(np.full(k + step + 1, Q31, dtype=np.uint8))
            t -= step
    blocks, start = [], 0
    for (lx, rx), n in sorted(recs.items()):
        blocks.append(_rows(key_s, lx, rx, n, start, key == "S"))
        start += n
    singles = np.concatenate(blocks) if blocks else np.zeros((0, k + 2), dtype=np.uint8)
    singles = singles[np.random.default_rng(12345).permutation(singles.shape[0])]
    out = []
    cuts = [singles.shape[0] * i // (len(bulk) + 1) for i in range(len(bulk) + 2)]
    for i in range(len(bulk) + 1):
        out.extend(singles[cuts[i]:cuts[i + 1]])
        if i < len(bulk):
            out.append(bulk[i])
    return out


def join(read_list):
    lens = np.array([r.size for r in read_list], dtype=np.uint64)
    offs = np.zeros(len(read_list) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    return (np.concatenate(read_list) if read_list else np.zeros(0, np.uint8)).astype(np.uint8), offs


def packed_bytes(recs: dict, key: str, k: int) -> int:
    """Bytes of reads(recs, key, k) without building them."""
    n = dict(recs)
    total = 0
    if key == "A":
        t = n.pop(("A", "A"), 0)
        total += t + (k + 1) * ((t + 399) // 400)
    return total + (k + 2) * sum(n.values())


MAX_BYTES = 3_500_000  # about 3 MB of packed reads: the largest input a test builds (32768 + reads of k + 2 = 101 bases)


# ---- inputs ----------------------------------------------------------------------------------------------------------

def inputs(key: str, hot: int) -> dict:
    """name -> records. top / second: the counters of the major and the minor extension pair, on both sides alike;
    none: records with N on both sides (they add to the count alone)."""
    M, m = MAJOR[key], MINOR[key]
    N2 = ("N", "N")
    d = {}
    levels = {"7fff": 0x7FFF, "8000": 0x8000, "8001": 0x8001, "hot-1": hot - 1, "hot": hot, "hot+1": hot + 1,
              "bfff": 0xBFFF, "c000": 0xC000, "c001": 0xC001, "51200": 51200, "65534": 65534, "65535": 65535,
              "65536": 65536, "18001": 0x18001}
    for name, n in levels.items():  # one counter on each side, equal to the count
        d[f"pure_{name}"] = {M: n}
    # the top counter at thr - 1 and thr under a count of 65536 (none-records fill it up: count >> top), for the
    # thresholds 2, 6553, 32767, 32768, 33422 (0.51 * 65535), 49151 (0.75 * 65535) and 65535
    for top in (1, 2, 6552, 6553, 32766, 32767, 32768, 33421, 33422, 49150, 49151):
        d[f"top_{top}"] = {M: top, N2: 65536 - top}
    d["top_59999"] = {M: 59999, N2: 1}  # dyn 0: thr = count = 60000
    d["top_65534"] = {M: 65534, N2: 2}  # dyn 0: thr = 65535, top one below; the count saturates
    d["top_65535"] = {M: 65535, N2: 1}
    # the runner-up at thr - 1 and thr under a top counter past the clamp level
    for second in (1, 2, 6552, 6553, 32766, 32767, 32768, 33421, 33422, 0xC000):
        d[f"two_c001_{second}"] = {M: 0xC001, m: second, N2: max(0, 65536 - 0xC001 - second)}
    for second in (49150, 49151):  # 0.75 * 65535 = 49151: both counters next to the clamp level
        d[f"two_c001_{second}"] = {M: 0xC001, m: second}
    d["two_65536_40000"] = {M: 65536, m: 40000}
    if key == "A":  # (131070 single-record reads of S would pass MAX_BYTES at every k)
        for second in (65534, 65535):  # dyn 0: thr = 65535, 'F' only when both counters saturate
            d[f"two_65535_{second}"] = {M: 65535, m: second}
    # one side without a countable neighbour in most records: count >> that side's top (thr 6553 at dyn 0.9)
    for top in (6552, 6553):
        d[f"leftnone_{top}"] = {("N", M[1]): 65536 - top, M: top}
        d[f"rightnone_{top}"] = {(M[0], "N"): 65536 - top, M: top}
    return d


@dataclass(frozen=True)
class Case:
    name: str   # the input's name
    key: str    # "A" or "S"
    dyn: float
    dmin: int

    @property
    def id(self) -> str:
        return f"{self.key}-{self.name}-dyn{self.dyn}-dmin{self.dmin}"


def read_cases(hot: int, k: int = 21, keys=("A", "S")) -> list:
    """Every (input, key, parameters) that sits next to a decision, the inputs within MAX_BYTES at this k."""
    out = []
    for key in keys:
        for name, recs in inputs(key, hot).items():
            if packed_bytes(recs, key, k) > MAX_BYTES:
                continue
            for dyn, dmin in PARAMS:
                if discriminates(recs, dyn, dmin):
                    out.append(Case(name, key, dyn, dmin))
    return out


# A subset that holds every transition (X>base, base>F, kept>purged) at a threshold above 0x8000 with a counter at or
# past the clamp level, the dmin_thres = 32768 edge on clamped counters, the 65535 / 65536 counts and both sides of HOT.
SUBSET = [
    ("pure_hot-1", 0.0, 2), ("pure_hot", 0.0, 2), ("pure_hot+1", 0.0, 0), ("pure_51200", 0.25, 2),
    ("pure_65535", 0.0, 0), ("pure_65536", 0.0, 2), ("pure_18001", 0.0, 2), ("top_65534", 0.0, 2), ("top_65535", 0.0, 2),
    ("two_c001_49150", 0.25, 2), ("two_c001_49151", 0.25, 2), ("two_c001_33422", 0.49, 2),
    ("two_c001_32767", 0.9, 32768), ("pure_c000", 0.9, 32768), ("two_65536_40000", 0.25, 2),
]


def subset_cases(k: int, wide: bool = False) -> list:
    """SUBSET on key A, and at k = 21 on key S too (its single-record reads pass MAX_BYTES at larger k)."""
    hot = HOT[record_kind(k, wide)]
    out = []
    for key in ("A", "S") if k <= 21 else ("A",):
        ins = inputs(key, hot)
        for name, dyn, dmin in SUBSET:
            if packed_bytes(ins[name], key, k) <= MAX_BYTES:
                out.append(Case(name, key, dyn, dmin))
    return out


def case_records(c: Case, hot: int) -> dict:
    return inputs(c.key, hot)[c.name]


def clamped_wrong(recs: dict, dyn: float, dmin: int, to: int = CLAMP_TO) -> bool:
    """Whether the row changes when every counter at or past the clamp level is read as `to`. With the clamp's target
    0x8000 that takes a threshold above 0x8000; with 0x7FFF it marks the cases that pin the target itself."""
    count, left, right = counters(recs)
    cl = [to if v >= CLAMP_AT else v for v in left]
    cr = [to if v >= CLAMP_AT else v for v in right]
    return decide(count, cl, cr, dyn, dmin) != decide(count, left, right, dyn, dmin)


def discriminates(recs: dict, dyn: float, dmin: int) -> bool:
    return bool(near(recs, dyn, dmin)) or clamped_wrong(recs, dyn, dmin) or clamped_wrong(recs, dyn, dmin, CLAMP_TO - 1)


# ---- contig cases ----------------------------------------------------------------------------------------------------

CTG_DEPTHS = [0x7FFF, 0x8000, 0xBFFF, 0xC000, 65535]
CTG_DYN = [0.9, 0.5, 0.25, 0.0]
CTG_EXT = ("A", "T")  # the contig `A key T`


def ctg_states(key: str) -> dict:
    """The read side of a contig case: name -> records of the key in the reads."""
    M, m = MAJOR[key], MINOR[key]
    return {
        "absent": {},
        "singleton": {m: 1},
        "nonuu": {m: 3, (M[0], m[1]): 3},          # two left extensions of equal weight
        "hot_ff": {M: 32768, m: 32768},            # count 65536, 'F' (or 'X') on both sides: replaced
        "hot_uu": {M: 51200},                      # count 51200 past the clamp level, unique on both sides: kept
    }


@dataclass(frozen=True)
class CtgCase:
    state: str
    key: str
    ctgs: tuple  # ((left, right, depth), ...) occurrences of the key in contigs, in the order they are applied
    dyn: float
    dmin: int = 2

    @property
    def id(self) -> str:
        c = "+".join(f"{lx}{rx}{d}" for lx, rx, d in self.ctgs)
        return f"{self.key}-{self.state}-{c}-dyn{self.dyn}"


def ctg_fold(ctgs, dyn, dmin):
    """insert_supermer_from_ctg over the key's contig occurrences alone (kcount_cpu.cpp:381-398): (count, left, right)
    of the contig entry."""
    count, lx, rx = None, None, None
    for l2, r2, d in ctgs:
        if count is None:
            count = d
        elif count != 0:
            one = lambda x: [count if "ACGT"[i] == x else 0 for i in range(4)]  # noqa: E731
            agree = get_ext(one(lx), count, dyn, dmin) == l2 and get_ext(one(rx), count, dyn, dmin) == r2
            count = min(count, d) if agree else 0
        lx, rx = l2, r2
    return count, lx, rx


def ctg_row(c: CtgCase):
    """The row of a contig case: the read entry when it has count >= 2 and a unique extension on both sides, else the
    folded contig entry."""
    count, left, right = counters(ctg_states(c.key)[c.state])
    if count >= 2:
        lc, rc = get_ext(left, count, c.dyn, c.dmin), get_ext(right, count, c.dyn, c.dmin)
        if lc not in "XF" and rc not in "XF":
            return decide(count, left, right, c.dyn, c.dmin)
    d, lx, rx = ctg_fold(c.ctgs, c.dyn, c.dmin)
    one = lambda x: [d if "ACGT"[i] == x else 0 for i in range(4)]  # noqa: E731
    return decide(d, one(lx), one(rx), c.dyn, c.dmin)


def ctg_cases(key: str = "S", states=None, dyns=CTG_DYN) -> list:
    out = []
    for state in states or ctg_states(key):
        for dyn in dyns:
            for d in CTG_DEPTHS:
                out.append(CtgCase(state, key, ((*CTG_EXT, d),), dyn))
            if state in ("absent", "singleton"):  # a second occurrence: the min rule, and count 0 on a disagreement
                out.append(CtgCase(state, key, ((*CTG_EXT, 65535), (*CTG_EXT, 0xC000)), dyn))
                out.append(CtgCase(state, key, ((*CTG_EXT, 0xC000), (*CTG_EXT, 65535)), dyn))
                out.append(CtgCase(state, key, ((*CTG_EXT, 65535), ("C", CTG_EXT[1], 65535)), dyn))
    return out


def ctg_seqs(c: CtgCase, k: int):
    """The contigs of a case: `left key right`, every second occurrence as its reverse complement."""
    key_s = key_string(c.key, k)
    seqs = []
    for i, (lx, rx, _) in enumerate(c.ctgs):
        s = lx + key_s + rx
        seqs.append(revcomp(s) if i % 2 else s)
    return seqs, np.array([d for _, _, d in c.ctgs], dtype=np.uint16)


def ctg_clamped_wrong(c: CtgCase) -> bool:
    """Whether the row changes when a counter at or past the clamp level is read as 0x8000 under a threshold above it:
    the kept read entry's counters, or the contig entry's depth."""
    count, left, right = counters(ctg_states(c.key)[c.state])
    d, _, _ = ctg_fold(c.ctgs, c.dyn, c.dmin)
    v = count if c.state == "hot_uu" else d  # (hot_uu's only counter is its count: kept under every threshold)
    return v >= CLAMP_AT and threshold(v, c.dyn, c.dmin) > CLAMP_TO
