"""Helpers of the uutig tests (test_uutigs.py): the rule of mhmkc_uutigs (include/mhmkc.h) restated in Python over a
fetched table and its links, and the small genomes whose tables hold the rule's rare structures (a long cycle, a
hairpin, rows that are their own reverse complement)."""
from __future__ import annotations

import numpy as np

import mhm2_proxy_amd as m
from query_lib import COMP, NO_ROW, OK, RC

STRUCTURES = ("path", "cycle_many", "cycle_one", "hairpin", "nonmutual_inner", "nonmutual_start")


def revcomp(s: str) -> str:
    return s[::-1].translate(COMP)


def pack_reads(seqs, qual: int = 31):
    """PackedRead bytes (code | quality << 3) and offsets of ACGT strings, every base at one quality."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    b = np.array([code[c] | (qual << 3) for s in seqs for c in s], dtype=np.uint8)
    return b, offs


def random_genome(n: int, seed: int) -> str:
    rng = np.random.default_rng(seed)
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def circular_set(n: int = 500, seed: int = 77, read_len: int = 100, step: int = 7):
    """A circular genome of n bases read with wrap-around, each read three times: at k <= read_len one cycle of n rows
    (the genome is repeated until a read fits, so n may be smaller than a read)."""
    g = random_genome(n, seed)
    gg = g * (2 + read_len // n)
    reads = [gg[a:a + read_len] for a in range(0, n, step)]
    return pack_reads([r for r in reads for _ in range(3)])


def palindrome_set(k: int, with_start: bool, seed: int = 91, u_len: int = 300, read_len: int = 100, step: int = 7):
    """The genome U + revcomp(U), tiled by reads, each three times. Its centre k-mer is its own reverse complement for
    even k (a row with a non-mutual port) and a hairpin for odd k; with_start appends A^(k/2) to U, which makes the
    centre row A^(k/2) T^(k/2), the smallest key of its component: its start."""
    u = random_genome(u_len, seed)
    if with_start:  # (a C before the run: no k-mer holds more A's in front than the centre's)
        u = u[:-1] + "C" + "A" * (k // 2)
    g = u + revcomp(u)
    starts = list(range(0, len(g) - read_len, step)) + [len(g) - read_len]
    return pack_reads([g[a:a + read_len] for a in starts for _ in range(3)])


TIE_X = "A" * 16 + "C" + "A" * 15  # the first key word of every tied key


def tie_shared(word: int, seed: int = 133) -> str:
    """The 32 (word - 1) bases that follow TIE_X in every tied key: with them the keys share their first `word` words."""
    return random_genome(32 * (word - 1), seed)


def tiled(g: str, read_len: int, step: int) -> list:
    """Reads of read_len bases every step bases of the linear genome g and one at its end, each three times."""
    starts = list(range(0, len(g) - read_len, step)) + [len(g) - read_len]
    return [g[a:a + read_len] for a in starts for _ in range(3)]


def tie_set(seed: int = 33, r_len: int = 120, read_len: int = 100, step: int = 7, word: int = 1):
    """A genome in which X = A^16 C A^15 occurs twice, followed by C and by T: for 35 <= k <= 100 the two k-mers that
    begin with X are the smallest keys of their (single) component and share their first key word, so the start is
    decided by the later words. word > 1 puts the same 32 (word - 1) bases between X and the C / T: the two keys share
    exactly their first `word` words (k >= 32 word + 3)."""
    x = TIE_X + tie_shared(word)
    r = [random_genome(r_len, seed + i) for i in range(3)]
    g = r[0] + "G" + x + "C" + r[1] + "G" + x + "T" + r[2]
    return pack_reads(tiled(g, read_len, step))


def order_tie_set(word: int, n_gen: int = 6, seed: int = 214, r_len: int = 150, read_len: int = 160, step: int = 7):
    """n_gen separate linear genomes R_j + PRE_j + X + S + R'_j (X, S as in tie_set; PRE_j two bases over C, G, T, distinct
    per genome, so that no two genomes share a k-mer and none holds a smaller key): n_gen paths whose start keys all
    begin with X + S, so their order, the contigs' ids, is decided in key word `word` (counted from 0) at the earliest."""
    x = TIE_X + tie_shared(word)
    pres = [a + b for a in "CGT" for b in "CGT"][:n_gen]
    assert len(pres) == n_gen
    reads = []
    for j, pre in enumerate(pres):
        g = random_genome(r_len, seed + 2 * j) + pre + x + random_genome(r_len, seed + 2 * j + 1)
        reads += tiled(g, read_len, step)
    return pack_reads(reads)


def cycle_set(length: int, seed: int = 401):
    """A circular genome of `length` bases: at k = 21 one cycle of exactly `length` rows."""
    return circular_set(length, seed + length)


MULTI_CYCLES = (33, 64, 257, 512)
MULTI_LINEAR = 700


def multi_cycle_set(seed: int = 501, read_len: int = 100, step: int = 7):
    """Circular genomes of MULTI_CYCLES bases, a linear one of MULTI_LINEAR bases and three poly-A reads: at k = 21
    cycles of 1, 33, 64, 257 and 512 rows beside a path of MULTI_LINEAR - k - 1 rows."""
    reads = []
    for j, n in enumerate(MULTI_CYCLES):
        g = random_genome(n, seed + j)
        gg = g * (2 + read_len // n)
        reads += [gg[a:a + read_len] for a in range(0, n, step) for _ in range(3)]
    reads += tiled(random_genome(MULTI_LINEAR, seed + len(MULTI_CYCLES)), read_len, step)
    reads += ["A" * read_len] * 3
    return pack_reads(reads)


def tiny_set(k: int, rows: int, seed: int = 601):
    """One random read of k + 1 + rows bases, three times: `rows` rows with both extensions, one contig."""
    return pack_reads([random_genome(k + 1 + rows, seed + k)] * 3)


def common_prefix(strs) -> int:
    """The number of leading bases that all the strings share."""
    n = 0
    while all(len(s) > n and s[n] == strs[0][n] for s in strs):
        n += 1
    return n


def uutigs_ref(t: m.KmerTable, nxt: np.ndarray, status: np.ndarray) -> dict:
    """mhmkc_uutigs restated (include/mhmkc.h): ports, mutual links, components, start, layout, depth, order, strand and
    the row map, from the table and its links alone. Returns offsets, seqs (list of str), depths, n_kmers, row_ctg,
    row_pos, row_rc, cyclic (per contig: a cycle), start_keys (per contig), the set of STRUCTURES met and the numbers of walkable rows and of non-mutual ports."""
    n, k = len(t), t.k
    strs = m.keys_to_strings(t.keys, k) if n else []
    counts = [int(x) for x in t.counts]
    walkable = [chr(int(t.left[i])) in "ACGT" and chr(int(t.right[i])) in "ACGT" for i in range(n)]

    def entry(i, d):  # the port an OK port enters
        st = int(status[d, i])
        if (st & ~RC) != OK:
            return None
        return int(nxt[d, i]), d ^ (1 if st & RC else 0) ^ 1

    met = set()
    link = {}  # linked port -> the port it enters
    nonmutual = set()  # rows with a non-mutual port
    n_nonmutual = 0
    for i in range(n):
        for d in (0, 1):
            en = entry(i, d)
            if en is None:
                continue
            assert walkable[i] and walkable[en[0]], "a link leaves or enters a row without two base extensions"
            if en == (i, d):
                met.add("hairpin")
            elif entry(*en) == (i, d):
                link[(i, d)] = en
            else:
                assert strs[i] == revcomp(strs[i]), "a non-mutual port on a row that is not its own reverse complement"
                nonmutual.add(i)
                n_nonmutual += 1

    def travel(i, d):  # the rows met leaving (i, d), each with the port travel leaves it through; stops at an end or at i
        out = [(i, d)]
        while (i, d) in link:
            j, e = link[(i, d)]
            i, d = j, e ^ 1
            if (i, d) == out[0]:
                return out, True
            out.append((i, d))
        return out, False

    comp_of = [-1] * n
    comps = []  # (rows in travel order with their leaving ports, is a cycle)
    for i in range(n):  # paths: from the end port with the smaller (row, d) of the two
        for d in (0, 1):
            if walkable[i] and (i, d) not in link:
                chain, cyc = travel(i, d ^ 1)
                assert not cyc
                last = chain[-1]
                if (i, d) < last:
                    for r, _ in chain:
                        assert comp_of[r] < 0, "a row in two components"
                        comp_of[r] = len(comps)
                    comps.append((chain, False))
    for i in range(n):  # what is left lies on cycles
        if walkable[i] and comp_of[i] < 0:
            chain, cyc = travel(i, 0)
            assert cyc
            for r, _ in chain:
                assert comp_of[r] < 0
                comp_of[r] = len(comps)
            comps.append((chain, True))

    recs = []  # (start key, bases, depth, placed rows, is a cycle)
    for chain, cyc in comps:
        mrows = len(chain)
        s = min((r for r, _ in chain), key=lambda r: strs[r])
        if cyc:  # leftwards from the start, all the way round
            chain, _ = travel(s, 0)
            assert len(chain) == mrows
            met.add("cycle_one" if mrows == 1 else "cycle_many")
        else:
            met.add("path")
        ds = next(d for r, d in chain if r == s)
        # travel order is left to right in the start's frame when the start is left through its port 1
        placed = [(x if ds == 1 else mrows - 1 - x, r, 0 if d == ds else 1) for x, (r, d) in enumerate(chain)]
        placed.sort()
        oriented = [revcomp(strs[r]) if rc else strs[r] for _, r, rc in placed]
        for a, b in zip(oriented, oriented[1:]):
            assert a[1:] == b[:-1], "neighbouring rows of a contig do not overlap"
        seq = "".join(o[0] for o in oriented[:-1]) + oriented[-1]
        depth = (sum(counts[r] for r, _ in chain) + counts[s]) / (mrows + 1)
        for r, _ in chain:
            if r in nonmutual:
                met.add("nonmutual_start" if r == s else "nonmutual_inner")
        recs.append((strs[s], seq, depth, placed, cyc))
    recs.sort(key=lambda x: x[0])

    row_ctg = np.full(n, NO_ROW, dtype=np.uint32)
    row_pos = np.zeros(n, dtype=np.uint32)
    row_rc = np.zeros(n, dtype=np.uint8)
    offsets = np.zeros(len(recs) + 1, dtype=np.uint64)
    for c, (_, seq, _, placed, _) in enumerate(recs):
        offsets[c + 1] = int(offsets[c]) + len(seq)
        for pos, r, rc in placed:
            row_ctg[r], row_pos[r], row_rc[r] = c, pos, rc
    return {"offsets": offsets, "seqs": [x[1] for x in recs], "depths": np.array([x[2] for x in recs], dtype=np.float64),
            "n_kmers": np.array([len(x[3]) for x in recs], dtype=np.uint32), "row_ctg": row_ctg, "row_pos": row_pos,
            "row_rc": row_rc, "cyclic": np.array([x[4] for x in recs], dtype=bool), "start_keys": [x[0] for x in recs],
            "met": met, "n_walkable": sum(walkable), "n_nonmutual": n_nonmutual}


def ref_lines(ref: dict) -> list:
    """Sorted "<canonical uutig> <depth %.6f>" lines, as query_lib.walk_links and tests/cpp/dbjg_test.cpp give them."""
    return sorted(f"{min(s, revcomp(s))} {d:.6f}" for s, d in zip(ref["seqs"], ref["depths"]))
