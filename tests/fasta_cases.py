"""Reference and inputs for the assembly statistics and the FASTA text of device-resident contigs (include/mhmkc.h:
mhmkc_ctgs_stats_device, mhmkc_ctgs_fasta_device; Contigs::print_stats and Contigs::dump_contigs, src/contigs.cpp:92-180).

The reference is plain Python: fasta_ref formats with '%f' (the contract of to_string(double)), stats_ref sums the depths
with math.fsum and applies the N50 rule of the header, fmt_int restates the integer scheme the device formats depths with,
stats_text_ref the block print_stats logs. Every case builder asserts, from the reference, that the edge it is named after
is really in the case. numpy and Python only: no GPU, no library.
"""
from __future__ import annotations

import functools
import math
import struct
from fractions import Fraction
from typing import NamedTuple

import numpy as np

LEN_CLASSES = (1000, 5000, 10000, 25000, 50000)
TWO32 = float(2**32)
ID_MAX = 2**63 - 1


class Case(NamedTuple):
    name: str
    seqs: tuple        # bytes per contig
    depths: tuple      # float per contig
    first_id: int
    min_lens: tuple    # the min_ctg_len values the case is run with


# ------------------------------------------------------------------------------------------------
# the reference


def fasta_ref(seqs, depths, first_id: int, min_len: int) -> bytes:
    """dump_contigs' bytes (src/contigs.cpp:166-180): the id is the index in the unfiltered list, the sequence as it is."""
    return b"".join(b">Contig%d %s\n%s\n" % (first_id + c, ("%f" % d).encode(), s)
                    for c, (s, d) in enumerate(zip(seqs, depths)) if len(s) >= min_len)


def n50_ref(lens) -> tuple:
    """(n50, l50): the lengths in descending order, l50 the smallest number of leading contigs whose lengths sum to s with
    2 s >= the total, n50 the length of the last of them; (0, 0) when nothing is counted."""
    lens = sorted(lens, reverse=True)
    tot, s = sum(lens), 0
    for i, ln in enumerate(lens):
        s += ln
        if 2 * s >= tot:
            return ln, i + 1
    return 0, 0


def stats_ref(seqs, depths, min_len: int) -> dict:
    """print_stats' figures (src/contigs.cpp:92-113) with an exactly rounded depth sum, and N50 / L50."""
    kept = [(s, d) for s, d in zip(seqs, depths) if len(s) >= min_len]
    lens = [len(s) for s, _ in kept]
    n50, l50 = n50_ref(lens)
    return {"n_ctgs": len(kept), "tot_len": sum(lens), "max_len": max(lens, default=0),
            "n_ns": sum(s.count(b"N") for s, _ in kept), "tot_depth": math.fsum(d for _, d in kept),
            "len_sums": [sum(ln for ln in lens if ln >= c) for c in LEN_CLASSES], "n50": n50, "l50": l50}


def depth_bound(depths) -> float:
    """|a floating sum of n values in any order - the exact sum| <= (n - 1) u sum|d| (1 + O(u)), u = 2^-53; the tests
    allow n 2^-52 sum|d|, which also covers math.fsum's own half ulp."""
    return len(depths) * 2.0**-52 * math.fsum(abs(d) for d in depths)


def merge_stats(parts) -> dict:
    """The reduction over ranks of per-rank figures (everything but n50 / l50, which need the lengths)."""
    out = {"n_ctgs": 0, "tot_len": 0, "max_len": 0, "n_ns": 0, "tot_depth": 0.0, "len_sums": [0] * 5}
    for p in parts:
        for f in ("n_ctgs", "tot_len", "n_ns"):
            out[f] += p[f]
        out["max_len"] = max(out["max_len"], p["max_len"])
        out["tot_depth"] += p["tot_depth"]
        out["len_sums"] = [a + b for a, b in zip(out["len_sums"], p["len_sums"])]
    return out


def micro_int(d: float) -> int:
    """d * 10^6 rounded to nearest, ties to even, in integers: d = m 2^-s with the 53-bit significand; the product m 10^6
    is below 2^73; the quotient is the shift; round up when the remainder is above half, or is half and the quotient odd;
    a shift wider than the product gives 0. For finite d >= 0 below 2^32."""
    bits = struct.unpack("<Q", struct.pack("<d", d))[0]
    assert bits < 0x41F0000000000000, d
    e, frac = bits >> 52, bits & ((1 << 52) - 1)
    m, s = (frac | (1 << 52), 1075 - e) if e else (frac, 1074)
    assert s >= 21
    p = m * 10**6
    assert p < 2**73
    if s >= 74:
        return 0
    q, rem, half = p >> s, p & ((1 << s) - 1), 1 << (s - 1)
    return q + (1 if rem > half or (rem == half and q & 1) else 0)


def fmt_int(d: float) -> str:
    q = micro_int(d)
    return "%d.%06d" % (q // 10**6, q % 10**6)


def _g(x: float) -> str:
    return "%g" % x  # ostream << double at the default precision


def _div(a: float, b: float) -> str:
    if b == 0:  # the stream prints the IEEE result: 0.0 / 0 is x86's default NaN, which glibc prints with its sign
        return "-nan" if a == 0 else ("inf" if a > 0 else "-inf")
    return _g(a / b)


def stats_text_ref(st: dict, min_len: int) -> str:
    """The SLOG lines of print_stats (src/contigs.cpp:151-163) without colour codes; perc_str
    (upcxx-utils/src/log.cpp:428-434) is "num (p%)" with two fixed decimals, 0.00 for an empty total; the class label is
    left-justified in 19 columns."""
    tot = st["tot_len"]
    lines = [f"Assembly statistics (contig lengths >= {min_len})",
             f"    Number of contigs:       {st['n_ctgs']}",
             f"    Total assembled length:  {tot}",
             f"    Average contig depth:    {_div(st['tot_depth'], st['n_ctgs'])}",
             f"    Number of Ns/100kbp:     {_div(float(st['n_ns']) * 100000.0, tot)} ({st['n_ns']})",
             f"    Max. contig length:      {st['max_len']}",
             "    Contig lengths:"]
    for kbp, s in zip((1, 5, 10, 25, 50), st["len_sums"]):
        pc = "%.2f" % (0.0 if tot == 0 else 100.0 * s / tot)
        lines.append("        > " + f"{kbp}kbp:".ljust(19) + f"{s} ({pc}%)")
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------------------------
# inputs


def arrays(case: Case):
    """(bases uint8, offsets uint64 [n + 1], depths float64 [n]) of a case."""
    lens = np.fromiter((len(s) for s in case.seqs), dtype=np.uint64, count=len(case.seqs))
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    bases = np.frombuffer(b"".join(case.seqs), dtype=np.uint8).copy()
    return bases, offsets, np.asarray(case.depths, dtype=np.float64)


def rand_seq(rng, n: int) -> bytes:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def depth_values() -> list:
    """The values at which '%f' can go wrong."""
    rng = np.random.default_rng(7)
    v = [0.0, 5e-324, 65535.0, float(np.nextafter(TWO32, 0.0))]
    ties = [j / 128.0 for j in range(1, 4002, 2)]  # x.xxxxxx5 exactly: half-way cases of both parities
    v += ties
    carries = []
    for p in range(1, 10):  # 9.9999995 .. 999999999.9999995: the rounding carries into a new digit
        x = 10.0**p - 5e-7
        carries += [float(np.nextafter(x, 0.0)), x, float(np.nextafter(x, np.inf))]
    v += carries
    v += [s / den for den in (128.0, 256.0, 3.0) for s in range(1, 1025)]  # uutig depths: (sum + start count) / (m + 1)
    v += (rng.random(5000) * 10.0**rng.integers(-7, 10, 5000)).tolist()
    raw = rng.integers(0, 0x41F0000000000000, 5000, dtype=np.uint64)  # any exponent below 2^32
    v += raw.view(np.float64).tolist()
    # the edges are there, by the reference
    assert "%f" % 5e-324 == "0.000000" and "%f" % v[3] == "4294967296.000000"  # (rounds up to 2^32: 10 digits still)
    halves = [Fraction(t) * 10**6 for t in ties]
    assert all(h.denominator == 2 for h in halves)  # every j / 128 with odd j is an exact tie at the sixth decimal
    floors = [h.numerator // 2 for h in halves]
    assert any(q & 1 for q in floors) and any(not q & 1 for q in floors)  # ties that round up and ties that round down
    assert all(("%f" % t)[-1] in "02468" for t in ties)  # ... to even, by the reference
    for p in range(1, 10):
        a, b, c = ("%f" % x for x in carries[3 * (p - 1):3 * p])
        assert len(a) + 1 == len(c) and a.endswith(".999999") and c.endswith(".000000"), (a, b, c)
    assert all(0.0 <= x < TWO32 for x in v)
    return v


@functools.lru_cache(maxsize=None)
def depths_case() -> Case:
    rng = np.random.default_rng(11)
    v = depth_values()
    return Case("depths", tuple(rand_seq(rng, 17 + i % 9) for i in range(len(v))), tuple(v), 0, (0,))


def id_cases() -> list:
    """first_id such that the ids cross a digit count, 2^32, and end at the last id there is."""
    rng = np.random.default_rng(13)
    out = []
    for name, first in (("9", 8), ("99", 98), ("1e9", 999999998), ("2^32", 2**32 - 2), ("1e18", 10**18 - 2),
                        ("2^63", ID_MAX - 4)):
        seqs = tuple(rand_seq(rng, 30 + i) for i in range(4))
        c = Case(f"ids-{name}", seqs, (1.5, 2.25, 3.0, 4.125), first, (0,))
        ids = [first + i for i in range(4)]
        if name == "2^63":
            assert ids[-1] + 1 == ID_MAX  # first_id + n_ctgs == 2^63 - 1, the bound itself
        elif name == "2^32":
            assert ids[1] == 2**32 - 1 and ids[2] == 2**32
        else:
            assert len(str(ids[1])) + 1 == len(str(ids[2]))
        out.append(c)
    return out


FIXED_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 499, 500, 501, 999, 1000, 1001,
                 4999, 5000, 9999, 10000, 24999, 25000, 49999, 50000, 70001)


def seq_starts(seqs, depths, first_id: int, min_len: int) -> list:
    """Per written contig (source offset of its bases, offset of its bases in the text, length), from the reference."""
    out, src, dst = [], 0, 0
    for c, (s, d) in enumerate(zip(seqs, depths)):
        if len(s) >= min_len:
            hdr = len(b">Contig%d %s\n" % (first_id + c, ("%f" % d).encode()))
            out.append((src, dst + hdr, len(s)))
            dst += hdr + len(s) + 1
        src += len(s)
    return out


@functools.lru_cache(maxsize=None)
def lengths_case() -> Case:
    """Every fixed length, one long contig and 2000 random ones: every pair (source offset mod 16, text offset mod 16)
    occurs at a contig of at least 48 bases."""
    for seed in range(40):
        rng = np.random.default_rng(100 + seed)
        lens = list(FIXED_LENGTHS) + rng.integers(1, 401, 2000).tolist()
        seqs = tuple(rand_seq(rng, n) for n in lens)
        depths = tuple((rng.random(len(lens)) * 10.0**rng.integers(0, 6, len(lens))).tolist())
        pairs = {(s % 16, d % 16) for s, d, n in seq_starts(seqs, depths, 0, 0) if n >= 48}
        if len(pairs) == 256:
            mx = max(lens)
            assert mx == 70001 and all(x in lens for x in FIXED_LENGTHS)
            return Case("lengths", seqs, depths, 0, (0, 1, 499, 500, 501, 1000, mx, mx + 1))
    raise AssertionError("no seed of 40 gives every (source, text) residue pair")


@functools.lru_cache(maxsize=None)
def filter_case() -> Case:
    """The first, the last and runs of 70 consecutive contigs filtered out (min_ctg_len 30)."""
    rng = np.random.default_rng(17)
    lens = [5] + [40, 41] + [7] * 70 + [35] * 3 + [29] * 70 + [30, 31] + [3] * 70 + [64, 29]
    seqs = tuple(rand_seq(rng, n) for n in lens)
    keep = [n >= 30 for n in lens]
    assert not keep[0] and not keep[-1]
    runs = "".join("k" if x else "f" for x in keep).split("k")
    assert sum(1 for r in runs if len(r) == 70) == 3
    return Case("filters", seqs, tuple((rng.random(len(lens)) * 100).tolist()), 1000, (30, 0))


def empty_case() -> Case:
    return Case("empty", (), (), 5, (0, 500))


@functools.lru_cache(maxsize=None)
def ns_case() -> Case:
    """N at a contig's first and last byte, at the edges of the 16-byte units of the bases array, a contig of only N,
    lowercase n (not counted); min_ctg_len 40 filters out some of the contigs that hold N."""
    rng = np.random.default_rng(19)
    seqs = [bytearray(rand_seq(rng, n)) for n in (50, 23, 64, 41, 16, 39, 100, 7, 48)]
    seqs[0][0] = seqs[0][-1] = ord("N")
    seqs[1][:] = b"N" * 23
    seqs[3][5] = ord("n")
    seqs[5][0] = seqs[5][38] = ord("N")
    seqs[7][:] = b"n" * 7
    flat_off = np.cumsum([0] + [len(s) for s in seqs])
    for c in (2, 6):  # N at global positions 16 j - 1 and 16 j inside these contigs
        j = (int(flat_off[c]) + 16 + 15) // 16
        for pos in (16 * j - 1, 16 * j):
            seqs[c][pos - int(flat_off[c])] = ord("N")
    seqs = tuple(bytes(s) for s in seqs)
    flat = b"".join(seqs)
    npos = [i for i, ch in enumerate(flat) if ch == ord("N")]
    assert any(p % 16 == 15 for p in npos) and any(p % 16 == 0 for p in npos)
    assert seqs[0][0] == seqs[0][-1] == ord("N") and set(seqs[1]) == {ord("N")} and b"n" in seqs[3]
    all_n, kept_n = stats_ref(seqs, [1.0] * 9, 0)["n_ns"], stats_ref(seqs, [1.0] * 9, 40)["n_ns"]
    assert 0 < kept_n < all_n and flat.count(b"n") == 8
    return Case("ns", seqs, tuple(float(i + 1) for i in range(9)), 0, (0, 1, 2, 40, 24))


def n50_cases() -> list:
    rng = np.random.default_rng(23)

    def mk(name, lens):
        return Case(f"n50-{name}", tuple(rand_seq(rng, n) for n in lens), tuple(2.0 + i for i in range(len(lens))), 0, (0,))

    out = [mk("equal", [20] * 6), mk("half-even", [30, 10, 10, 10]), mk("half-odd", [31, 10, 10, 10]),
           mk("just-below-half", [29, 10, 10, 10]), mk("last", [1] * 5), mk("one", [77])]
    want = {"equal": (20, 3), "half-even": (30, 1), "half-odd": (31, 1), "just-below-half": (10, 2), "last": (1, 3),
            "one": (77, 1)}
    for c in out:  # the 2 s >= tot_len edge, by the rule
        assert n50_ref([len(s) for s in c.seqs]) == want[c.name[4:]], c.name
    tot = sum(len(s) for s in out[1].seqs)
    assert 2 * 30 == tot and 2 * 31 > sum(len(s) for s in out[2].seqs) and 2 * 29 < sum(len(s) for s in out[3].seqs)
    return out


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    return tuple([depths_case(), lengths_case(), filter_case(), empty_case(), ns_case()] + id_cases() + n50_cases())
