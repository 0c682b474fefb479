"""Single-rank read extraction at its span, group, tile, view and round edges (TEST INFRASTRUCTURE): a plain numpy
reference of what the extraction computes per window, and the inputs ("cases") that put k_read_start_bits, load_tile,
the walks (walk_windows, walk_c32_lh, walk_m2, WalkSpan::valid_mask[_wide]) and scatter_staged[_c40] of
mhm2_proxy_amd/csrc/kcount_kernels.hip on those edges. No GPU import: tests/test_extract_cases.py holds the reference
to the oracle and every case to its figures on the CPU, tests/test_extract_edges.py runs the cases on the GPU.

  windows(b, o, k, qcut)    every counted window of a batch (the interior windows 1 .. L-k-1 of every read with
                            L >= k + 2): stream position, canonical key (N read as G), left / right ext code in the key's
                            orientation (EXT_NONE for an N neighbour or one of quality < qcut)
  table(w)                  the table of those windows by the plain rule: count, per-side counters, get_ext with the
                            dynamic threshold, the purge of singletons and of X/X rows

Every case is decisive: each read that holds a window is in the batch a second time as its reverse complement with
every quality good (its twin), and no canonical k-mer repeats otherwise. So every key occurs exactly twice at
dmin_thres = 2, an extension is its letter if the first copy's neighbour is countable and X if not, and one wrong or
dropped window adds or removes a row: a whole-table comparison sees every bit the extraction computes.

A case is a builder (k) -> Built (one or more batches) with a predicate over the reference's output that proves the
case has its edge (CASES[name].figures, every value must be true). A builder searches seeds until its figures and the
decisiveness conditions hold; one that cannot is a failure, not a skip.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path

import numpy as np

import oracle_lib as O
from supermer_cases import EXT_NONE, GOODQ, LOWQ, _top_mask, _words32, join, n_longs, reads_of  # noqa: F401

# The geometry the cases aim at, by key words (mhm2_proxy_amd/csrc: TILE_BASES and E_THREADS_NL in kcount_launch.hpp,
# E_CAP in kcount_kernels.hip; test_extract_cases.test_constants_match_the_source fails if they moved).
TILE = {1: 4096, 2: 4096, 3: 1536, 4: 2048}      # bases per extraction tile
THREADS = {1: 256, 2: 256, 3: 256, 4: 256}       # threads per tile
SPAN = {nl: TILE[nl] // THREADS[nl] for nl in TILE}  # W: consecutive windows per thread
E_CAP = {1: 4096, 2: 2560, 3: 1024, 4: 768}
CAP = {nl: min(E_CAP[nl], TILE[nl]) for nl in TILE}  # records staged at once (kECap)
GROUP = 32          # bases per staged group
HALO_GROUPS = 1     # groups staged to the left of a tile
QCUT = 20           # KmerCounter's default qual_cutoff
QUALS = (0, 1, 19, 20, 30, 31)  # the qualities every flagged read set holds

# one k per walk and its compiled-in twin (ISSUE: compact 10..21, generic one-word 22, 31, two-word 33..63, three- and
# four-word keys)
KS = (10, 15, 16, 20, 21, 22, 31, 33, 34, 47, 55, 62, 63, 65, 77, 95, 97, 99, 127)

CSRC = Path(__file__).resolve().parents[1] / "mhm2_proxy_amd" / "csrc"


def source_constants() -> dict:
    """TILE_BASES, E_THREADS_NL and E_CAP as the sources state them."""
    out = {}
    for name, fname in (("TILE_BASES", "kcount_launch.hpp"), ("E_THREADS_NL", "kcount_launch.hpp"),
                        ("E_CAP", "kcount_kernels.hip")):
        m = re.search(r"constexpr\s+int\s+" + name + r"\[5\]\s*=\s*\{([^}]*)\}", (CSRC / fname).read_text())
        assert m, f"{name} not found in {fname}"
        v = [int(x) for x in m.group(1).split(",")]
        out[name] = {nl: v[nl] for nl in (1, 2, 3, 4)}
    return out


# ------------------------------------------------------------------------------------------------
# the reference

def good_bits(b: np.ndarray, qcut: int = QCUT) -> np.ndarray:
    """The base can be counted as an extension: it is not N and its quality is at least qcut."""
    return ((b & 7) < 4) & ((b >> 3) >= qcut)


@dataclass
class Win:
    """The counted windows of one batch, in read order."""
    k: int
    n_bases: int
    n_reads: int
    pos: np.ndarray     # (n,) stream position of the window's first base
    read: np.ndarray    # (n,) its read
    keys: np.ndarray    # (n, n_longs) canonical key
    rc: np.ndarray      # (n,) the key is the reverse complement
    cl: np.ndarray      # (n,) the left / right neighbour's code (N as G), forward
    cr: np.ndarray
    left: np.ndarray    # (n,) ext codes in the key's orientation at the qcut given (EXT_NONE: none)
    right: np.ndarray
    ukeys: np.ndarray = field(default=None)   # the distinct keys, sorted word-wise
    inv: np.ndarray = field(default=None)     # (n,) each window's row of ukeys

    @property
    def ext(self) -> np.ndarray:
        return ((self.left << 3) | self.right).astype(np.uint8)


def ext_codes(w: Win, good: np.ndarray):
    """(left, right) ext codes of every window in its key's orientation, from the countable bits: complemented and
    swapped where the key is the reverse complement."""
    gl, gr = good[w.pos - 1], good[w.pos + w.k]
    lf, rf = np.where(gl, w.cl, EXT_NONE), np.where(gr, w.cr, EXT_NONE)
    lr, rr = np.where(gr, 3 - w.cr, EXT_NONE), np.where(gl, 3 - w.cl, EXT_NONE)
    return np.where(w.rc, lr, lf).astype(np.int64), np.where(w.rc, rr, rf).astype(np.int64)


def windows(b, o, k: int, qcut: int = QCUT) -> Win:
    b = np.ascontiguousarray(b, dtype=np.uint8)
    o = np.asarray(o).astype(np.int64)
    nl, N = n_longs(k), int(b.size)
    lens = np.diff(o)
    nw = np.clip(lens - k - 1, 0, None)
    read = np.repeat(np.arange(lens.size, dtype=np.int64), nw)
    first = np.cumsum(nw) - nw
    j = np.arange(int(nw.sum()), dtype=np.int64) - np.repeat(first, nw) + 1  # interior windows 1 .. L-k-1
    pos = o[:-1][read] + j
    c = b & 7
    code = np.where(c == 4, 2, c & 3).astype(np.uint64)  # N -> G
    pad = np.zeros(32 * nl + 32, np.uint64)
    F = _words32(np.concatenate([code, pad]))
    R = _words32(np.concatenate([(np.uint64(3) - code)[::-1], pad]))
    tm = _top_mask(k - 32 * (nl - 1))
    fw = np.stack([F[pos + 32 * w] for w in range(nl)], axis=1) if pos.size else np.zeros((0, nl), np.uint64)
    q = N - k - pos  # the window's reverse complement starts here in the reversed, complemented stream
    rc = np.stack([R[q + 32 * w] for w in range(nl)], axis=1) if pos.size else np.zeros((0, nl), np.uint64)
    fw[:, nl - 1] &= tm
    rc[:, nl - 1] &= tm
    lt = np.zeros(pos.size, bool)  # rc < fw, word-wise lexicographic (Kmer::operator<)
    decided = np.zeros(pos.size, bool)
    for w in range(nl):
        lt = np.where(decided, lt, rc[:, w] < fw[:, w])
        decided |= rc[:, w] != fw[:, w]
    keys = np.ascontiguousarray(np.where(lt[:, None], rc, fw))
    x = Win(k, N, int(lens.size), pos, read, keys, lt, code[pos - 1].astype(np.int64),
            code[pos + k].astype(np.int64), None, None)
    x.left, x.right = ext_codes(x, good_bits(b, qcut))
    if pos.size:
        x.ukeys, inv = np.unique(keys, axis=0, return_inverse=True)
        x.inv = inv.reshape(-1).astype(np.int64)
    else:
        x.ukeys, x.inv = np.zeros((0, nl), np.uint64), np.zeros(0, np.int64)
    return x


_LETTERS = np.frombuffer(b"ACGT", np.uint8)


def _get_ext(cnt4: np.ndarray, count: np.ndarray, dmin_thres: int, dyn_min_depth: float) -> np.ndarray:
    """get_ext over rows of A, C, G, T counters: X below the threshold, F if the runner-up reaches it, else the letter
    with the most votes (ties to the higher letter). The threshold is max(dmin_thres, int((1 - dyn) * count))."""
    s = np.sort(cnt4, axis=1)
    top = 3 - np.argmax(cnt4[:, ::-1], axis=1)
    dmin = np.maximum(np.floor((1.0 - dyn_min_depth) * count.astype(np.float64)).astype(np.int64), dmin_thres)
    out = _LETTERS[top]
    out = np.where(s[:, 2] >= dmin, ord("F"), out)
    return np.where(s[:, 3] < dmin, ord("X"), out).astype(np.uint8)


@dataclass
class Table:
    keys: np.ndarray
    counts: np.ndarray
    left: np.ndarray
    right: np.ndarray
    stats: dict

    def same(self, other: "Table") -> bool:
        return (self.keys.shape == other.keys.shape and np.array_equal(self.keys, other.keys)
                and np.array_equal(self.counts, other.counts) and np.array_equal(self.left, other.left)
                and np.array_equal(self.right, other.right))


def table(w: Win, left=None, right=None, dmin_thres: int = 2, dyn_min_depth: float = 0.9, rows=None) -> Table:
    """The table of the windows, rows sorted by key. rows: only these rows of w.ukeys (every key's row depends on its own
    windows alone, so the rows of a subset are the whole table's)."""
    left = w.left if left is None else left
    right = w.right if right is None else right
    inv, G, ukeys = w.inv, w.ukeys.shape[0], w.ukeys
    if rows is not None:
        rows = np.unique(np.asarray(rows, np.int64))
        sel = np.flatnonzero(np.isin(inv, rows))
        inv, left, right = np.searchsorted(rows, inv[sel]), left[sel], right[sel]
        G, ukeys = rows.size, ukeys[rows]
    cnt = np.minimum(np.bincount(inv, minlength=G), 65535)
    L = np.minimum(np.bincount(inv * 5 + left, minlength=5 * G).reshape(G, 5)[:, :4], 65535)
    R = np.minimum(np.bincount(inv * 5 + right, minlength=5 * G).reshape(G, 5)[:, :4], 65535)
    lch, rch = _get_ext(L, cnt, dmin_thres, dyn_min_depth), _get_ext(R, cnt, dmin_thres, dyn_min_depth)
    keep = (cnt >= 2) & ~((lch == ord("X")) & (rch == ord("X")))
    st = dict(occurrences=int(inv.size), distinct=int(G), purged=int(G - keep.sum()), n_out=int(keep.sum()))
    return Table(ukeys[keep], cnt[keep].astype(np.uint16), lch[keep], rch[keep], st)


# ------------------------------------------------------------------------------------------------
# building blocks

def flagged(rng, L: int, low: float = 0.3, n_rate: float = 0.0) -> np.ndarray:
    """A random read: `low` of its bases below QCUT, n_rate of them N (of any quality), qualities over 0 .. 31 with the
    values of QUALS frequent."""
    codes = rng.integers(0, 4, size=L).astype(np.uint8)
    lo_q = np.where(rng.random(L) < 0.6, rng.choice([0, 1, 19], size=L), rng.integers(0, QCUT, size=L))
    hi_q = np.where(rng.random(L) < 0.6, rng.choice([20, 30, 31], size=L), rng.integers(QCUT, 32, size=L))
    q = np.where(rng.random(L) < low, lo_q, hi_q).astype(np.uint8)
    codes[rng.random(L) < n_rate] = 4
    return (codes | (q << 3)).astype(np.uint8)


def rev_twin(r: np.ndarray) -> np.ndarray:
    """The reverse complement of a read with every quality good. An N is read as G in a key, so its place takes C: the
    twin's k-mers are the read's."""
    c = r & 7
    return (np.where(c < 4, 3 - c, 1).astype(np.uint8) | np.uint8(GOODQ << 3))[::-1].copy()


def with_base(r: np.ndarray, i: int, kind: str, rng) -> None:
    """Make base i of a read low quality, N (good quality) or good."""
    c = int(r[i]) & 7
    if kind == "N":
        r[i] = 4 | (GOODQ << 3)
    else:
        if c == 4:
            c = int(rng.integers(0, 4))
        r[i] = c | ((LOWQ if kind == "low" else GOODQ) << 3)


def base_kind(b: np.ndarray, i: int) -> str:
    return "N" if (int(b[i]) & 7) == 4 else "good" if (int(b[i]) >> 3) >= QCUT else "low"


@dataclass
class Batch:
    b: np.ndarray
    o: np.ndarray
    first: np.ndarray   # (n_bases,) the base belongs to a first copy (a read that was not placed as a twin)


class Layout:
    """Reads placed one after another. A read that holds a window leaves its twin pending; the pending twins fill the
    way to the next target position (with fresh reads where none fits) and the rest follow at the end."""

    def __init__(self, rng, k: int):
        self.rng, self.k = rng, k
        self.reads, self.is_first, self.pending, self.pos = [], [], [], 0

    def put(self, r: np.ndarray, twin: bool = True, first: bool = True) -> int:
        start = self.pos
        self.reads.append(np.asarray(r, np.uint8))
        self.is_first.append(first)
        self.pos += int(r.size)
        if twin and r.size >= self.k + 2:
            self.pending.append(rev_twin(r))
        return start

    def fresh(self, L: int, low: float = 0.3, n_rate: float = 0.0) -> np.ndarray:
        return flagged(self.rng, int(L), low, n_rate)

    def empty(self, n: int = 1) -> None:
        for _ in range(n):
            self.put(np.zeros(0, np.uint8), twin=False)

    def owe(self, r: np.ndarray) -> None:
        """The twin of a read that lies elsewhere (in another batch)."""
        self.pending.append(rev_twin(r))

    def at(self, target: int) -> None:
        assert target >= self.pos, (target, self.pos)
        k = self.k
        while self.pos < target:
            gap = target - self.pos
            i = next((i for i, t in enumerate(self.pending) if t.size <= gap), None)
            if i is not None:
                self.put(self.pending.pop(i), twin=False, first=False)
            else:
                self.put(self.fresh(gap if gap <= k + 160 else int(self.rng.integers(k + 2, k + 150)), low=0.15))

    def flush(self) -> None:
        while self.pending:
            self.put(self.pending.pop(0), twin=False, first=False)

    def batch(self) -> Batch:
        assert not self.pending, "twins left over"
        b, o = join(self.reads)
        first = np.repeat(np.array(self.is_first, bool), [r.size for r in self.reads]) if self.reads else np.zeros(0, bool)
        return Batch(b, o, first)


@dataclass
class Built:
    batches: list          # [Batch]
    wins: list             # [Win] of every batch at QCUT
    extra: dict = field(default_factory=dict)

    def all_reads(self) -> Batch:
        """Every read of the case as one batch (reads never span batches: the table is that of the batches)."""
        rs = [x for bt in self.batches for x in reads_of(bt.b, bt.o.astype(np.int64))]
        b, o = join(rs)
        return Batch(b, o, np.concatenate([bt.first for bt in self.batches]) if self.batches else np.zeros(0, bool))


def twice_fraction(w: Win) -> float:
    """The share of the distinct keys that occur exactly twice."""
    if not w.ukeys.shape[0]:
        return 1.0
    return float((np.bincount(w.inv, minlength=w.ukeys.shape[0]) == 2).mean())


def decisive(k: int, built: Built) -> dict:
    """The decisiveness conditions of a case: from the oracle's stats, occurrences == 2 * distinct for k >= 16 (every
    key exactly twice, as no key occurs once: each counted read has its twin); for k < 16, where 4^k / 2 keys cannot hold
    a case without repeats, at least 95 % of the distinct keys exactly twice."""
    a = built.all_reads()
    st = O.kcount(a.b, a.o, k).stats()
    if k >= 16:
        return {"occurrences == 2 * distinct (oracle)": st["occurrences"] == 2 * st["distinct"] and st["distinct"] > 0}
    return {">= 95 % of the keys occur exactly twice": twice_fraction(windows(a.b, a.o, k)) >= 0.95,
            "some window is counted (oracle)": st["distinct"] > 0}


def _seeded(build, figures, k: int, tries: int = 40) -> Built:
    """The first of build(seed) that is decisive and whose figures are all true."""
    for seed in range(tries):
        batches, extra = build(seed)
        built = Built(batches, [windows(bt.b, bt.o, k) for bt in batches], extra)
        if all(decisive(k, built).values()) and all(figures(k, built).values()):
            return built
    return built  # (the test names what is missing)


def _starts(bt: Batch) -> np.ndarray:
    return bt.o.astype(np.int64)[:-1]


def _lens(bt: Batch) -> np.ndarray:
    return np.diff(bt.o.astype(np.int64))


# ------------------------------------------------------------------------------------------------
# the cases

def span_phases(k):
    """Read starts at every residue modulo lcm(32, W), at each one read of k + 2 bases (one window), one of k + 1 (none)
    and one of k + 3: every funnel shift of codes64 / bits32, and the `last` scan and st_bits at every offset within a
    span's reach of k + W."""
    M = math.lcm(GROUP, SPAN[n_longs(k)])

    def build(seed):
        rng = np.random.default_rng(11000 + 10 * k + seed)
        lay = Layout(rng, k)
        need = {(r, L) for r in range(M) for L in (k + 1, k + 2, k + 3)}
        lay.put(lay.fresh(k + 7))
        while need:
            r = lay.pos % M
            here = sorted(L for rr, L in need if rr == r)
            if here:
                need.discard((r, here[0]))
                lay.put(lay.fresh(here[0]))
            else:  # a short read moves the phase on to the nearest residue that still needs a read
                lay.put(lay.fresh(min((rr - r) % M for rr, _ in need)))
        lay.flush()
        return [lay.batch()], {}
    return _seeded(build, span_phases_figures, k)


def span_phases_figures(k, built):
    M = math.lcm(GROUP, SPAN[n_longs(k)])
    bt, w = built.batches[0], built.wins[0]
    s, L = _starts(bt), _lens(bt)
    out = {f"reads of k + {d} start at every residue mod {M} (lcm(32, W = {SPAN[n_longs(k)]}))":
           set((s[L == k + d] % M).tolist()) == set(range(M)) for d in (1, 2, 3)}
    one = np.flatnonzero(np.bincount(w.read, minlength=L.size) == 1)
    out[f"reads with exactly one window start at every residue mod {M}"] = set((s[one] % M).tolist()) == set(range(M))
    return out


N_EMPTY_ENDS, N_EMPTY_ROW, LONG_GROUPS = 3000, 70, 40


def short_runs(k):
    """Runs of reads of length 0, 1, k - 1, k and k + 1 between countable reads (several read starts inside one window's
    [p, p + k]); 70 empty reads in a row; 3000 empty reads at the start of the batch and 3000 at its end; a read longer
    than 40 groups; and a second batch whose only counted window is its last."""
    def build(seed):
        rng = np.random.default_rng(12000 + 10 * k + seed)
        lay = Layout(rng, k)
        lay.empty(N_EMPTY_ENDS)
        shorts = [0, 1, k - 1, k, k + 1]
        for _ in range(16):
            lay.put(lay.fresh(k + 2 + int(rng.integers(0, 40))))
            run = [shorts[i] for i in rng.permutation(5)] + \
                [int(x) for x in rng.choice([0, 0, 1, 1, k - 1, k, k + 1], size=int(rng.integers(0, 6)))]
            for L in run:
                lay.put(lay.fresh(L), twin=False)
        lay.put(lay.fresh(k + 9))
        lay.empty(N_EMPTY_ROW)
        lay.put(lay.fresh(k + 9))
        lay.put(lay.fresh(LONG_GROUPS * GROUP + 77 + k))
        single = lay.fresh(k + 2)
        lay.owe(single)
        lay.flush()
        lay.empty(N_EMPTY_ENDS)
        lay2 = Layout(rng, k)
        for L in (0, 1, k + 1, 0, k, k - 1, 0, 0, 1):
            lay2.put(lay2.fresh(L), twin=False)
        lay2.put(single, twin=False)
        return [lay.batch(), lay2.batch()], {}
    return _seeded(build, short_runs_figures, k)


def short_runs_figures(k, built):
    bt, w = built.batches[0], built.wins[0]
    o, L = bt.o.astype(np.int64), _lens(bt)
    countable = L >= k + 2
    # read starts (the end's among them) inside [s, s + k] for a start s: three or more
    crowd = int((np.searchsorted(o, o + k, side="right") - np.searchsorted(o, o, side="left")).max())
    idx = np.flatnonzero(countable)
    between = [int((L[a + 1:z] == 0).sum()) for a, z in zip(idx[:-1], idx[1:]) if (L[a + 1:z] == 0).all()]
    w2, b2 = built.wins[1], built.batches[1]
    return {"three or more read starts inside one window's [p, p + k]": crowd >= 3,
            "runs hold reads of 0, 1, k - 1, k, k + 1": {0, 1, k - 1, k, k + 1} <= set(L.tolist()),
            f"{N_EMPTY_ROW} empty reads in a row between two countable reads": N_EMPTY_ROW in between,
            f"{N_EMPTY_ENDS} empty reads at the start": bool((L[:N_EMPTY_ENDS] == 0).all()) and int(idx[0]) == N_EMPTY_ENDS,
            f"{N_EMPTY_ENDS} empty reads at the end": bool((L[-N_EMPTY_ENDS:] == 0).all()) and L[-N_EMPTY_ENDS - 1] > 0,
            f"a first-copy read longer than {LONG_GROUPS} groups": int(L.max()) > LONG_GROUPS * GROUP,
            "the first batch counts windows": w.pos.size > 0,
            "the second batch's only counted window is its last": w2.pos.size == 1 and int(w2.pos[0]) + k + 1 == b2.b.size
            and _lens(b2).size > 1}


EDGE_STARTS = (-33, -32, -1, 0, 1)
EDGE_FLANKS = (("low", "N"), ("N", "good"), ("good", "low"))


def tile_edges(k):
    """At the tile boundaries B = T and 2T: a countable read that ends and a countable read that starts at B - 33,
    B - 32, B - 1, B and B + 1; and reads that straddle B from before B - k to past B + k, so that a window lies at
    every split of its key over B, the window at tile position 0 is counted with its left neighbour B - 1 (in the halo
    group) low, N or good, and the window at B - 1 with its right neighbour B + k - 1 low, N or good. Four batches,
    two boundaries each."""
    T = TILE[n_longs(k)]

    def build(seed):
        rng = np.random.default_rng(13000 + 10 * k + seed)
        jobs = [("start", d) for d in EDGE_STARTS] + [("flank", f) for f in EDGE_FLANKS]
        batches = []
        for i in range(0, len(jobs), 2):
            lay = Layout(rng, k)
            for (what, arg), B in zip(jobs[i:i + 2], (T, 2 * T)):
                if what == "start":
                    X = lay.fresh(k + 2 + int(rng.integers(0, 30)))
                    lay.at(B + arg - X.size)
                    lay.put(X)
                    lay.put(lay.fresh(k + 2 + 34 + int(rng.integers(0, 30))))
                else:
                    s = B - k - 2 - int(rng.integers(0, 20))
                    R = lay.fresh(B + 2 * k + 2 + int(rng.integers(0, 20)) - s, low=0.15)
                    with_base(R, B - 1 - s, arg[0], rng)
                    with_base(R, B + k - 1 - s, arg[1], rng)
                    lay.at(s)
                    lay.put(R)
            lay.flush()
            batches.append(lay.batch())
        return batches, {}
    return _seeded(build, tile_edges_figures, k)


def tile_edges_figures(k, built):
    nl = n_longs(k)
    T = TILE[nl]
    starts, used, left0, right1, splits = set(), set(), set(), set(), set()
    for bt, w in zip(built.batches, built.wins):
        s, L = _starts(bt), _lens(bt)
        for B in (T, 2 * T):
            ok = np.flatnonzero((L[1:] >= k + 2) & (L[:-1] >= k + 2)) + 1  # a countable read behind a countable read
            d = set((s[ok] - B).tolist()) & set(EDGE_STARTS)
            starts |= d
            if d:
                used.add(B)
            if (w.pos == B).any():
                left0.add(base_kind(bt.b, B - 1))
            if (w.pos == B - 1).any():
                right1.add(base_kind(bt.b, B + k - 1))
            inside = B - w.pos  # bases of the window before B
            splits |= set(inside[(inside > 0) & (inside < k)].tolist())
    return {f"countable reads end and start at B + {EDGE_STARTS}, B = T = {T} or 2T (TILE_BASES)": starts == set(EDGE_STARTS),
            "both boundaries T and 2T are used": used == {T, 2 * T},
            "the window at tile position 0 is counted with its left neighbour low, N and good": left0 == {"low", "N", "good"},
            "the window at B - 1 is counted with its right neighbour low, N and good": right1 == {"low", "N", "good"},
            "a counted window at every split of its k bases over B": splits == set(range(1, k))}


def _end_batch(rng, k: int, n: int, last: np.ndarray, owed=()) -> Batch:
    """A batch of exactly n bases whose last read is `last` (a first copy; its twin leads the batch)."""
    lay = Layout(rng, k)
    lay.put(rev_twin(last), twin=False, first=False)
    for r in owed:
        lay.put(rev_twin(r), twin=False, first=False)
    gap = n - lay.pos - last.size
    half = gap // 2
    assert half >= k + 2, (n, k)
    rem, fill = half, []
    while rem:
        L = rem if rem < 2 * (k + 2) + 60 else int(rng.integers(k + 2, k + 60))
        fill.append(lay.fresh(L))
        rem -= L
    for r in fill:
        lay.put(r, twin=False)
    for i in rng.permutation(len(fill)):
        lay.put(rev_twin(fill[i]), twin=False, first=False)
    if gap - 2 * half:
        lay.put(lay.fresh(gap - 2 * half), twin=False)
    lay.put(last, twin=False)
    assert lay.pos == n
    return lay.batch()


def data_end(k):
    """Batches of n_bases = 0, 1 and 31 (mod 32), of T and of T + 1 bases (a tile that holds one base), each ending in a
    countable first-copy read, so that its last window's right neighbour is the batch's last base (low and good), and a
    batch that is one read of k + 2 bases."""
    T = TILE[n_longs(k)]
    base = GROUP * ((8 * k + 400) // GROUP)

    def build(seed):
        rng = np.random.default_rng(14000 + 10 * k + seed)
        single = flagged(rng, k + 2)
        batches = []
        for i, n in enumerate((base, base + 1, base + 31, T, T + 1)):
            last = flagged(rng, k + 2 + int(rng.integers(0, 40)))
            with_base(last, last.size - 1, "low" if i % 2 == 0 else "good", rng)
            batches.append(_end_batch(rng, k, n, last, owed=[single] if i == 0 else ()))
        batches.append(Batch(single, np.array([0, single.size], np.uint64), np.ones(single.size, bool)))
        return batches, {}
    return _seeded(build, data_end_figures, k)


def data_end_figures(k, built):
    T = TILE[n_longs(k)]
    sizes = [int(bt.b.size) for bt in built.batches]
    lastw = all(w.pos.size and int(w.pos[-1]) + k == bt.b.size - 1 for bt, w in zip(built.batches, built.wins))
    kinds = {base_kind(bt.b, bt.b.size - 1) for bt in built.batches}
    t1 = [w for bt, w in zip(built.batches, built.wins) if bt.b.size == T + 1]
    return {"n_bases = 0, 1, 31 (mod 32)": {0, 1, 31} <= {n % GROUP for n in sizes if n not in (T, T + 1)},
            f"n_bases = T and T + 1 (T = {T}, TILE_BASES)": T in sizes and T + 1 in sizes,
            "every batch's last window has the batch's last base as its right neighbour": lastw,
            "that base is low in one batch and good in another": {"low", "good"} <= kinds,
            "a last group with fewer than 32 bases": any(n % GROUP for n in sizes),
            "the window before the tile that holds one base is counted": bool(t1) and int(t1[0].pos[-1]) == T - k,
            "a batch that is one read of k + 2 bases": any(bt.o.size == 2 and bt.b.size == k + 2 for bt in built.batches)}


FLAG_QCUTS = (0, 1, 20, 31, 32)


def _flag_reads(rng, k: int, total: int):
    """First-copy reads of about `total` bases: 30 % of the bases below QCUT, 2 % N of any quality."""
    reads = []
    n = 0
    while n < total:
        L = int(rng.integers(k + 2, k + 300)) if rng.random() < 0.85 else int(rng.choice([0, 1, k, k + 1, k + 2, k + 3]))
        reads.append(flagged(rng, L, low=0.3, n_rate=0.02))
        n += L
    return reads


def flags(k):
    """Random reads whose first copy has 30 % of its bases below the cutoff and 2 % N, some of them of good quality: N
    inside keys and as neighbours, every quality of QUALS as a neighbour's. Run at qual_cutoff 0, 1, 20, 31 and 32."""
    def build(seed):
        rng = np.random.default_rng(15000 + 10 * k + seed)
        lay = Layout(rng, k)
        for r in _flag_reads(rng, k, 9000):
            lay.put(r)
        lay.pending = [lay.pending[i] for i in rng.permutation(len(lay.pending))]
        lay.flush()
        return [lay.batch()], {}
    return _seeded(build, flags_figures, k)


def flags_figures(k, built):
    out = {}
    for bt, w in zip(built.batches, built.wins):
        fb = bt.b[bt.first]
        isn = (bt.b & 7) == 4
        low = float(((fb >> 3) < QCUT).mean())
        cs = np.concatenate([[0], np.cumsum(isn)])
        nb = np.concatenate([w.pos - 1, w.pos + k])  # the neighbours of counted windows
        nbf = nb[bt.first[nb]]
        out.update({"25-35 % of the first copy is below the cutoff": 0.25 <= low <= 0.35,
                    "1-3 % of the first copy is N": 0.01 <= float(((fb & 7) == 4).mean()) <= 0.03,
                    "an N lies inside a counted window": bool((cs[w.pos + k] - cs[w.pos] > 0).any()),
                    "an N of good quality is a neighbour": bool((isn[nbf] & ((bt.b[nbf] >> 3) >= QCUT)).any()),
                    "an N of low quality is a neighbour": bool((isn[nbf] & ((bt.b[nbf] >> 3) < QCUT)).any()),
                    f"neighbours of quality {QUALS}": set(QUALS) <= set((bt.b[nbf] >> 3).tolist())})
    return out


def round_counts(nl: int):
    """The per-tile window counts of the rounds case: around one and two stage capacities, where they fit in a tile."""
    T, C = TILE[nl], CAP[nl]
    return [n for n in (C - 1, C, C + 1, 2 * C, 2 * C + 1) if n + 1 <= T and (n <= C + 1 or 2 * C + 1 <= T)]


def rounds(k):
    """Keys of two or more words, whose tiles are emptied in rounds of CAP records: one read over three whole tiles
    (each counts T windows and leaves in ceil(T / CAP) rounds), and tiles that hold exactly CAP - 1, CAP, CAP + 1 and,
    where 2 CAP + 1 <= T, 2 CAP and 2 CAP + 1 counted windows (one read from the tile's first base, then reads too
    short to count)."""
    nl = n_longs(k)
    T = TILE[nl]
    assert nl >= 2

    def build(seed):
        rng = np.random.default_rng(16000 + 10 * k + seed)
        lay = Layout(rng, k)
        lay.at(T - 7)
        lay.put(lay.fresh(4 * T + k + 9 - (T - 7), low=0.2))
        tile = 5
        for n in round_counts(nl):
            lay.at(tile * T)
            lay.put(lay.fresh(n + k + 1, low=0.2))
            while lay.pos < (tile + 1) * T:
                lay.put(lay.fresh(min(k + 1, (tile + 1) * T - lay.pos)), twin=False)
            tile += 1
        lay.flush()
        return [lay.batch()], {"tiles": list(range(5, tile))}
    return _seeded(build, rounds_figures, k)


def rounds_figures(k, built):
    nl = n_longs(k)
    T, C = TILE[nl], CAP[nl]
    w = built.wins[0]
    per_tile = np.bincount(w.pos // T)
    want = round_counts(nl)
    got = [int(per_tile[t]) for t in built.extra["tiles"]]
    return {f"three tiles in a row count T = {T} windows each (TILE_BASES)": per_tile[1:4].tolist() == [T, T, T],
            f"a full tile leaves in two or more rounds of {C} (E_CAP)": -(-T // C) >= 2,
            f"tiles count exactly {want} windows": got == want and {C - 1, C, C + 1} <= set(got),
            "2 CAP and 2 CAP + 1 where they fit": (2 * C + 1 > T) or {2 * C, 2 * C + 1} <= set(got)}


# ---- host chunks (slice views)

VIEW_HEADS = (0, 1, 8, 15)


def host_chunks(o, chunk: int, nib: int):
    """The first read of every H2D chunk of a host batch under the knob chunk_bytes, as mhmkc::add_host (nib 0: a chunk
    ends at the first read boundary `chunk` or more bytes from its first byte) and add_host_nib (nib 1, 2: the first
    chunk a quarter of that, and at most max(64, chunk / 32) reads a chunk) cut them. The GPU test ties this to the
    library through its h2d_chunks figure."""
    o = np.asarray(o).astype(np.int64)
    n, chunk = o.size - 1, max(64, chunk)
    rmax = max(64, chunk // 32)
    out, r0, ci = [], 0, 0
    while r0 < n:
        out.append(r0)
        want = chunk if nib == 0 or ci else max(64, chunk // 4)
        hi = n if nib == 0 else min(n, r0 + rmax)
        r1 = r0 + 1
        while r1 < hi and o[r1] - o[r0] < want:
            r1 += 1
        r0, ci = r1, ci + 1
    return out


def chunk_heads(o, chunk: int, nib: int):
    o = np.asarray(o).astype(np.int64)
    return [int(o[r]) % 16 for r in host_chunks(o, chunk, nib)]


def _pick_chunks(o, nib: int):
    """A few chunk sizes, each giving four or more chunks, whose chunks begin at every b0 mod 16 of VIEW_HEADS."""
    need, picked = set(VIEW_HEADS), []
    for c in range(700, 1900, 7):
        h = chunk_heads(o, c, nib)
        if len(h) >= 4 and need & set(h[1:]):
            picked.append(c)
            need -= set(h[1:])
        if not need:
            break
    return picked if not need else []


def _views(k, dry: bool):
    def build(seed):
        rng = np.random.default_rng(17000 + 10 * k + seed + (500 if dry else 0))
        lay = Layout(rng, k)
        if dry:  # more bytes than the largest chunk size, in reads too short to count
            while lay.pos < 1900:
                lay.put(lay.fresh(int(rng.choice([k - 1, k, k + 1])), n_rate=0.02), twin=False)
        for r in _flag_reads(rng, k, 7000):
            lay.put(r)
        lay.pending = [lay.pending[i] for i in rng.permutation(len(lay.pending))]
        lay.flush()
        bt = lay.batch()
        return [bt], {"chunks": {nib: _pick_chunks(bt.o, nib) for nib in (0, 1)}}
    return _seeded(build, views_dry_figures if dry else views_figures, k)


def views(k):
    """The flags content as a host batch cut into small H2D chunks (the knob chunk_bytes), each extracted as a slice view
    that begins at the 16-byte aligned position at or below its first read: chunk sizes (Built.extra["chunks"], by the
    byte and the nibble path's cutting rule) under which chunks begin at b0 mod 16 = 0, 1, 8 and 15 (the view's head,
    `beg` in the walks)."""
    return _views(k, False)


def views_dry(k):
    """views behind reads too short to count, so that the first chunk holds no counted window."""
    return _views(k, True)


def views_figures(k, built):
    bt = built.batches[0]
    out = flags_figures(k, built)
    for nib in (0, 1):
        cs = built.extra["chunks"][nib]
        heads = set()
        for c in cs:
            heads |= set(chunk_heads(bt.o, c, nib)[1:])
        out[f"nib {nib}: chunks begin at b0 mod 16 = {VIEW_HEADS}"] = set(VIEW_HEADS) <= heads
        out[f"nib {nib}: four or more chunks at every size"] = bool(cs) and all(
            len(host_chunks(bt.o, c, nib)) >= 4 for c in cs)
    return out


def views_dry_figures(k, built):
    bt, w = built.batches[0], built.wins[0]
    out = views_figures(k, built)
    o = bt.o.astype(np.int64)
    for nib in (0, 1):
        for c in built.extra["chunks"][nib]:
            r1 = host_chunks(o, c, nib)[1]
            out[f"nib {nib}, {c} bytes: the first chunk holds no counted window"] = bool((w.read >= r1).all())
    return out


@dataclass
class Case:
    build: callable
    figures: callable
    qcuts: tuple = (QCUT,)
    min_longs: int = 1     # the fewest key words the case exists for
    views: bool = False    # a host-chunk case (run under chunk_bytes and as split and device adds)


CASES = {
    "span_phases": Case(span_phases, span_phases_figures),
    "short_runs": Case(short_runs, short_runs_figures),
    "tile_edges": Case(tile_edges, tile_edges_figures),
    "data_end": Case(data_end, data_end_figures),
    "flags": Case(flags, flags_figures, qcuts=FLAG_QCUTS),
    "rounds": Case(rounds, rounds_figures, min_longs=2),
    "views": Case(views, views_figures, views=True),
    "views_dry": Case(views_dry, views_dry_figures, views=True),
}


def cases_for(k: int):
    return [name for name, c in CASES.items() if n_longs(k) >= c.min_longs]


@lru_cache(maxsize=None)
def built(name: str, k: int) -> Built:
    """A case at one k, built once per process."""
    return CASES[name].build(k)


@lru_cache(maxsize=None)
def oracle(name: str, k: int, qcut: int = QCUT):
    """(keys, counts, left, right, stats) of the oracle over all the case's reads, computed once per process."""
    a = built(name, k).all_reads()
    t = O.kcount(a.b, a.o, k, qual_cutoff=qcut)
    return (*t.fetch(), t.stats())
