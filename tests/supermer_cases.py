"""The supermer exchange at its tile, word, flank and rank edges (TEST INFRASTRUCTURE): a plain numpy reference of
supermer formation, and the inputs ("cases") that put the kernels of DESIGN.md §3.5b on those edges.

With MHMKC_OWNER_MINIMIZER on several ranks and keys of two or more words a rank ships, per read slab, runs of
consecutive windows with one owner (k_smer_owner, k_smer_pack), each as n + k + 1 bases in whole 32-base words, and the
owner rebuilds the records from them (k_smer_extract). The reference here restates what must come out of that:

  windows(b, o, k)             every counted window of a batch (the interior windows 1 .. L-k-1 of every read with
                               L >= k + 2, N read as G): canonical key, ext code, stream position, flank bits
  reference(b, o, k, world)    the same with every window's owner (oracle_lib.target_ranks), the maximal runs (same
                               read, same owner, consecutive windows) and the runs cut at multiples of the tile size
  Ref.owned / n_runs / n_cut / words    what a slab sends: windows per destination, supermers, 32-base words

A case is a function (k, world) -> {rank: [(bytes, offs, "host" | "device"), ...]}, deterministic, with a predicate over
the reference's output that proves the case has its edge (CASES[name].figures, every value must be true). A builder
searches seeds until its predicate holds. Unless a case says otherwise a batch is one slab (a host batch below the H2D
chunk size, a device batch), whose stream position 0 is the batch's first base.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import oracle_lib as O

# Bases per extraction tile for keys of 2, 3 and 4 words: mirrors TILE_BASES in mhm2_proxy_amd/csrc/kcount_launch.hpp
# (k_smer_owner / k_smer_pack cut every run at a multiple of it). An assertion that depends on it says so.
TILE = {2: 4096, 3: 1536, 4: 2048}
QCUT = 20           # KmerCounter's default qual_cutoff
GOODQ, LOWQ = 31, 5
EXT_NONE = 4        # the ext code of a flank that is not countable (kmer_ops.hpp)
KS = (33, 63, 65, 95, 97, 127)  # one and 31 bases in the last key word, for 2, 3 and 4 words


def n_longs(k: int) -> int:
    return k // 32 + 1


def tile_of(k: int) -> int:
    return TILE[n_longs(k)]


def smer_words(n, k: int):
    """32-base words of a supermer of n windows: its n + k - 1 bases and the two flanks."""
    return (n + k + 1 + 31) // 32


# ------------------------------------------------------------------------------------------------
# the reference

def _words32(c: np.ndarray) -> np.ndarray:
    """w[p] = the 32 two-bit codes from position p, the first in the top bits (codes past the end read 0)."""
    w = c.astype(np.uint64) << np.uint64(62)
    sh = 1
    while sh < 32:
        nxt = np.zeros_like(w)
        nxt[:-sh] = w[sh:]
        w |= nxt >> np.uint64(2 * sh)
        sh *= 2
    return w


def _top_mask(n: int) -> np.uint64:
    return np.uint64(0xFFFFFFFFFFFFFFFF if n >= 32 else (0xFFFFFFFFFFFFFFFF >> (2 * n)) ^ 0xFFFFFFFFFFFFFFFF)


@dataclass
class Ref:
    """The counted windows of one batch, in read order, and their supermers."""
    k: int
    T: int
    n_bases: int
    n_reads: int
    keys: np.ndarray    # (n, n_longs) canonical key
    ext: np.ndarray     # (n,) (left << 3) | right in the key's orientation
    pos: np.ndarray     # (n,) stream position of the window's first base
    read: np.ndarray    # (n,) its read
    gl: np.ndarray      # (n,) the left / right flank base is countable (quality >= QCUT and not N)
    gr: np.ndarray
    owner: np.ndarray = field(default=None)   # (n,) get_kmer_target_rank
    start: np.ndarray = field(default=None)   # (n,) the window starts a maximal run
    cut: np.ndarray = field(default=None)     # (n,) the window starts a run cut at the tile edges
    world: int = 0

    def runs(self, cut: bool):
        """(first window, window count, owner) of every run."""
        first = np.flatnonzero(self.cut if cut else self.start)
        n = np.diff(np.append(first, self.pos.size))
        return first, n, self.owner[first].astype(np.int64)

    def owned(self) -> np.ndarray:
        return np.bincount(self.owner, minlength=self.world).astype(np.int64)

    def n_runs(self) -> int:
        return int(self.start.sum())

    def n_cut(self) -> int:
        return int(self.cut.sum())

    def words(self) -> int:
        return int(smer_words(self.runs(True)[1], self.k).sum())

    def per_dest(self):
        """Cut runs and words per destination."""
        _, n, d = self.runs(True)
        return (np.bincount(d, minlength=self.world).astype(np.int64),
                np.bincount(d, weights=smer_words(n, self.k), minlength=self.world).astype(np.int64))


def windows(b: np.ndarray, o: np.ndarray, k: int) -> Ref:
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
    good = (c < 4) & ((b >> 3) >= QCUT)
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
    keys = np.where(lt[:, None], rc, fw)
    gl, gr = good[pos - 1], good[pos + k]
    cl, cr = code[pos - 1].astype(np.int64), code[pos + k].astype(np.int64)
    lf, rf = np.where(gl, cl, EXT_NONE), np.where(gr, cr, EXT_NONE)
    lr, rr = np.where(gr, 3 - cr, EXT_NONE), np.where(gl, 3 - cl, EXT_NONE)
    ext = np.where(lt, (lr << 3) | rr, (lf << 3) | rf).astype(np.uint8)
    return Ref(k, tile_of(k), N, int(lens.size), np.ascontiguousarray(keys), ext, pos, read, gl, gr)


def reference(b, o, k: int, world: int, T: int | None = None) -> Ref:
    r = windows(b, o, k)
    r.world, r.T = world, T or r.T
    r.owner = O.target_ranks(r.keys, k, world).astype(np.int64) if r.pos.size else np.zeros(0, np.int64)
    new = np.ones(r.pos.size, bool)
    if r.pos.size:
        new[1:] = (r.read[1:] != r.read[:-1]) | (r.owner[1:] != r.owner[:-1])
    r.start = new
    r.cut = new | (r.pos % r.T == 0)
    return r


def rank_totals(refs: dict, world: int) -> dict:
    """Per rank over {rank: [Ref per batch]}: the windows it owns (from every rank), and of what it adds the maximal
    runs, the cut runs, their words and its windows."""
    owned = np.zeros(world, np.int64)
    out = {}
    for r in range(world):
        rs = refs.get(r, [])
        for x in rs:
            owned += x.owned()
        out[r] = {"runs": sum(x.n_runs() for x in rs), "cut": sum(x.n_cut() for x in rs),
                  "words": sum(x.words() for x in rs), "windows": sum(int(x.pos.size) for x in rs)}
    for r in range(world):
        out[r]["owned"] = int(owned[r])
    return out


# ------------------------------------------------------------------------------------------------
# building blocks of the cases

def pack(codes, quals=GOODQ) -> np.ndarray:
    return (np.asarray(codes, np.uint8) | (np.asarray(quals, np.uint8) << 3)).astype(np.uint8)


def rand_read(rng, L: int) -> np.ndarray:
    return pack(rng.integers(0, 4, size=L), GOODQ)


def revcomp_read(r: np.ndarray) -> np.ndarray:
    """The reverse complement of a packed read, qualities reversed with it. An N is read as G in a key, so its place in
    the reverse complement takes C: the twin's k-mers over it are the original's."""
    c = r & 7
    return (np.where(c < 4, 3 - c, 1).astype(np.uint8) | (r & 0xF8))[::-1].astype(np.uint8)


def twins(rng, reads):
    """A copy of every read, about half of them as the reverse complement, in another order. A k-mer that occurs once is
    purged from the table, and with it every trace of its flank bits: the cases add every random read at least twice, so
    that each window's record reaches the table (count 2, each extension with 0, 1 or 2 votes)."""
    out = [revcomp_read(r) if rng.integers(0, 2) else r.copy() for r in reads]
    return [out[i] for i in rng.permutation(len(out))]


def join(reads):
    offs = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum([r.size for r in reads], out=offs[1:])
    return (np.concatenate(reads) if reads else np.zeros(0, np.uint8)).astype(np.uint8), offs


def reads_of(b, o):
    return [b[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)]


def refs_of(batches: dict, k: int, world: int) -> dict:
    return {r: [reference(b, o, k, world) for b, o, _ in bl] for r, bl in batches.items()}


def all_reads(batches: dict):
    """Every read of a case as one batch (for the oracle's table)."""
    rs = [x for r in sorted(batches) for b, o, _ in batches[r] for x in reads_of(b, o)]
    return join(rs)


def _seeded(build, figures, k, world, tries=40):
    """The first of build(seed) whose figures are all true."""
    for seed in range(tries):
        batches = build(seed)
        refs = refs_of(batches, k, world)
        if all(figures(k, world, batches, refs).values()):
            return batches
    return batches  # (the test names the figure that is missing)


def _flat(refs):
    return [x for r in sorted(refs) for x in refs[r]]


# ------------------------------------------------------------------------------------------------
# the cases

def one_window(k, world):
    """Reads of length 0, 1, k, k + 1 (no window), k + 2 (one window: n = 1, both flanks are the read's ends) and k + 3,
    interleaved; rank 0's first batch and rank 1's last hold reads but no window."""
    rng = np.random.default_rng(1000 + k)
    out = {}
    for r in range(world):
        lens = [0, 1, k, k + 1, k + 2, k + 3] * 8
        reads = [rand_read(rng, L) for L in lens]
        none = join([rand_read(rng, L) for L in [0, 1, k, k + 1] * 4])
        out[r] = [(*join(reads), "host"), (*join(twins(rng, reads)), "device")]
        if r == 0:
            out[r].insert(0, (*none, "host"))
        if r == 1:
            out[r].append((*none, "device"))
    return out


def one_window_figures(k, world, batches, refs):
    fl = _flat(refs)
    return {"supermers with n == 1": sum(int((x.runs(True)[1] == 1).sum()) for x in fl) > 0,
            "a batch with reads and no window": any(x.n_reads > 0 and x.pos.size == 0 for x in fl),
            "reads of k + 2": any(int((np.bincount(x.read) == 1).sum()) > 0 for x in fl if x.pos.size)}


def tile_straddle(k, world):
    """Reads of several tiles' length, and short reads behind filler reads so that a read starts at stream offset T - 1,
    T and T + 1 and a read's last counted window is at T - 1."""
    T = tile_of(k)

    def build(seed):
        rng = np.random.default_rng(2000 + 10 * k + seed)
        pool = [rand_read(rng, int(T * f)) for f in (2.3, 3.1)]  # every batch holds them, on either strand
        fill = rand_read(rng, T + 1)                             # the fillers are its prefixes
        short, tail = rand_read(rng, k + 9), rand_read(rng, 40 + k)

        def longs():
            return twins(rng, pool)

        def behind(n):  # a short read starting at stream offset n
            return [fill[:n].copy(), short.copy()]
        out = {r: [] for r in range(world)}
        out[0].append((*join(behind(T - 1) + longs() + [revcomp_read(tail)]), "host"))
        out[0].append((*join(behind(T) + longs()), "device"))
        out[1].append((*join(behind(T + 1) + longs()), "host"))
        # a read of length L at offset x whose last window x + L - k - 1 is T - 1
        out[1].append((*join([fill[:T - 40].copy(), tail.copy()] + longs()), "device"))
        for r in range(2, world):
            out[r].append((*join(longs()), "host"))
        return out
    return _seeded(build, tile_straddle_figures, k, world)


def tile_straddle_figures(k, world, batches, refs):
    T = tile_of(k)
    fl = _flat(refs)
    straddle = sum(int(((x.pos[1:] % T == 0) & ~x.start[1:]).sum()) for x in fl if x.pos.size)
    starts = set()
    last_at = False
    spans3 = False
    two_edges = False
    for r in sorted(batches):
        for (b, o, _), x in zip(batches[r], refs[r]):
            o = np.asarray(o).astype(np.int64)
            starts |= set(o[:-1][np.diff(o) >= k + 2].tolist())
            spans3 |= bool(((o[1:] - 1) // T - o[:-1] // T >= 2).any())
            if x.pos.size:
                lastw = np.append(x.read[1:] != x.read[:-1], True)
                last_at |= bool((x.pos[lastw] == T - 1).any())
                first, n, _ = x.runs(False)
                two_edges |= bool(((x.pos[first] + n - 1) // T - x.pos[first] // T >= 2).any())
    return {f"a maximal run holds windows T-1 and T (T = {T}, TILE_BASES)": straddle > 0,
            "reads start at T-1, T, T+1": {T - 1, T, T + 1} <= starts,
            "a read's last window is T-1": last_at,
            "a run crosses two tile edges or a read spans 3 tiles": two_edges or spans3}


def one_owner_long(k, world):
    """One poly-A read and one period-3 repeat, each longer than 3 T (one owner each: every cut run but the last has
    exactly T windows, the largest descriptor), and a few short random reads on another rank."""
    T = tile_of(k)
    L = 3 * T + 211  # (the poly-A k-mer's total stays far below 65535)

    def build(seed):
        rng = np.random.default_rng(3000 + 10 * k + seed)
        out = {r: [] for r in range(world)}
        out[0].append((*join([pack(np.zeros(L, np.uint8))]), "host"))
        out[0].append((*join([pack(np.resize(np.array([0, 1, 2], np.uint8), L + 5))]), "device"))
        few = [rand_read(rng, k + 2 + int(rng.integers(0, 4))) for _ in range(2)]
        out[1].append((*join(few + twins(rng, few)), "host"))
        return out
    return _seeded(build, one_owner_long_figures, k, world)


def one_owner_long_figures(k, world, batches, refs):
    T = tile_of(k)
    fl = _flat(refs)
    owned = sum(x.owned() for x in fl)
    return {f"a cut run of exactly T = {T} windows (TILE_BASES)": any(bool((x.runs(True)[1] == T).any()) for x in fl),
            "a batch sends nothing to a destination": any(x.pos.size and bool((x.owned() == 0).any()) for x in fl),
            "a rank owns no window (world >= 3)": world < 3 or bool((owned == 0).any()),
            "the hot k-mer stays below 65535": max(int(x.pos.size) for x in fl) < 65535}


def _flank_sites(x: Ref):
    """Window indices by flank kind: (runs' first windows, runs' last windows, reads' first windows, reads' last
    windows, first windows of a run that follows another run of the same read, first windows of a cut run that
    continues a maximal run over a tile edge)."""
    first = np.flatnonzero(x.start)
    last = np.append(first[1:] - 1, x.pos.size - 1) if first.size else first
    rnew = np.ones(x.pos.size, bool)
    rnew[1:] = x.read[1:] != x.read[:-1]
    rfirst = np.flatnonzero(rnew)
    rlast = np.append(rfirst[1:] - 1, x.pos.size - 1) if rfirst.size else rfirst
    junction = np.flatnonzero(x.start & ~rnew)
    edge = np.flatnonzero(x.cut & ~x.start)
    return first, last, rfirst, rlast, junction, edge


def _flank_bits(k, world, n_rate):
    T = tile_of(k)

    def build(seed):
        rng = np.random.default_rng(4000 + 10 * k + seed + (500 if n_rate else 0))
        out = {}
        for r in range(world):
            reads = [rand_read(rng, int(rng.integers(k + 2, 420))) for _ in range(30)]
            reads += [rand_read(rng, int(T * 2.2)) for _ in range(2)]  # tile edges inside runs
            if n_rate:  # N -> G changes keys and owners: the reference below is of the bases with their N
                for x in reads:
                    x[rng.random(x.size) < n_rate] = 4 | (GOODQ << 3)
            bl = []
            for kind, rs in (("host", reads), ("device", twins(rng, reads))):
                b, o = join(rs)
                x = reference(b, o, k, world)
                first, last, rfirst, rlast, junction, edge = _flank_sites(x)
                low = []
                for idx, right in ((first, False), (last, True), (rfirst, False), (rlast, True)):
                    sel = idx[rng.random(idx.size) < 0.4]
                    low.append(x.pos[sel] + k if right else x.pos[sel] - 1)
                # where two runs of a read meet at windows p, p + 1 (two owners, or one owner and a tile edge): base p
                # is the second run's left flank and lies inside the first, base p + k is the first run's right flank
                # and lies inside the second
                for idx, rate in ((junction, 0.4), (edge, 0.5)):
                    sel = idx[rng.random(idx.size) < rate]
                    low.append(x.pos[sel] - 1)
                    sel = idx[rng.random(idx.size) < rate]
                    low.append(x.pos[sel] - 1 + k)
                low = np.concatenate(low)
                b[low] = (b[low] & 7) | (LOWQ << 3)  # quality only: no key, no owner changes
                bl.append((b, o, kind))
            out[r] = bl
        return out
    return _seeded(build, flank_bits_n_figures if n_rate else flank_bits_figures, k, world)


def flank_bits(k, world):
    """Random reads, each on both batches of its rank (twins), with the quality lowered, without changing any key, at
    the left flank of runs' first windows, the right flank of their last windows, reads' first and last bases, and the
    bases where two adjacent runs meet: two owners, or one owner cut at a tile edge (the flank is then in the staged
    tile's halo group)."""
    return _flank_bits(k, world, 0.0)


def flank_bits_n(k, world):
    """flank_bits with N bases sprinkled in (read as G in the keys, never countable as a flank)."""
    return _flank_bits(k, world, 1 / 70)


def flank_bits_figures(k, world, batches, refs):
    both = {name: set() for name in ("run first/left", "run last/right", "read first base", "read last base",
                                     "junction left", "junction right", "tile edge left", "tile edge right")}
    for x in _flat(refs):
        if not x.pos.size:
            continue
        first, last, rfirst, rlast, junction, edge = _flank_sites(x)
        both["run first/left"] |= set(x.gl[first].tolist())
        both["run last/right"] |= set(x.gr[last].tolist())
        both["read first base"] |= set(x.gl[rfirst].tolist())
        both["read last base"] |= set(x.gr[rlast].tolist())
        both["junction left"] |= set(x.gl[junction].tolist())
        both["junction right"] |= set(x.gr[junction - 1].tolist())
        both["tile edge left"] |= set(x.gl[edge].tolist())
        both["tile edge right"] |= set(x.gr[edge - 1].tolist())
    return {f"{name}: bit on and off": v == {True, False} for name, v in both.items()}


def flank_bits_n_figures(k, world, batches, refs):
    out = flank_bits_figures(k, world, batches, refs)
    n_flank = n_inside = 0
    for r in sorted(batches):
        for (b, o, _), x in zip(batches[r], refs[r]):
            if not x.pos.size:
                continue
            isn = (b & 7) == 4
            first, last, *_ = _flank_sites(x)
            n_flank += int(isn[x.pos[first] - 1].sum()) + int(isn[x.pos[last] + k].sum())
            cs = np.concatenate([[0], np.cumsum(isn)])
            n_inside += int((cs[x.pos[last] + k] - cs[x.pos[first]] > 0).sum())
    out["an N is a run's flank"] = n_flank > 0
    out["an N lies inside a run"] = n_inside > 0
    return out


def word_edges(k, world):
    """Reads of mixed lengths: runs whose n + k + 1 bases end on, one past and one before a word edge, that start at
    source shifts 0, 1 and 31, and the smallest (n = 1) and largest (n = T) word counts."""
    T = tile_of(k)

    def build(seed):
        rng = np.random.default_rng(5000 + 10 * k + seed)
        out = {}
        for r in range(world):
            reads = [rand_read(rng, int(rng.integers(0, 700))) for _ in range(40)]
            reads += [rand_read(rng, k + 2), rand_read(rng, 32 * int(rng.integers(4, 9)))]
            host = list(reads)
            if r == 0:
                host.insert(7, pack(np.zeros(2 * T + k + 40, np.uint8)))  # covers a whole tile wherever it lies
            out[r] = [(*join(host), "host"), (*join(twins(rng, reads)), "device")]
        return out
    return _seeded(build, word_edges_figures, k, world)


def word_edges_figures(k, world, batches, refs):
    T = tile_of(k)
    rem, shift, nmin, nmax = set(), set(), False, False
    for x in _flat(refs):
        first, n, _ = x.runs(True)
        rem |= set(((n + k + 1) % 32).tolist())
        shift |= set(((31 + x.pos[first] % T) % 32).tolist())  # k_smer_pack's sh of the run's first word
        nmin |= bool((n == 1).any())
        nmax |= bool((n == T).any())
    return {"(n + k + 1) % 32 takes 0, 1, 31": {0, 1, 31} <= rem,
            "the source shift takes 0, 1, 31": {0, 1, 31} <= shift,
            f"a run of the fewest words ({smer_words(1, k)})": nmin,
            f"a run of the most words ({smer_words(T, k)}, n = T = {T}, TILE_BASES)": nmax}


def idle_and_empty(k, world):
    """Rank 0 adds nothing at all; rank 1's first batch holds only reads shorter than k + 2 (with two ranks it adds a
    batch of random reads after it, so that there is something to count); the other ranks hold random reads."""
    rng = np.random.default_rng(6000 + k)
    out = {0: []}
    short = join([rand_read(rng, int(rng.integers(0, k + 2))) for _ in range(25)])
    out[1] = [(*short, "host")]
    def some():
        reads = [rand_read(rng, int(rng.integers(100, 300))) for _ in range(25)]
        return join(reads + twins(rng, reads))
    if world == 2:
        out[1].append((*some(), "device"))
    for r in range(2, world):
        out[r] = [(*some(), "host" if r % 2 else "device")]
    return out


def idle_and_empty_figures(k, world, batches, refs):
    return {"rank 0 adds no batch": len(batches[0]) == 0,
            "rank 1's first batch has reads and no window": refs[1][0].n_reads > 0 and refs[1][0].pos.size == 0,
            "some window is counted": sum(int(x.pos.size) for x in _flat(refs)) > 0}


UNEVEN_RANK, UNEVEN_CHUNK = 1, 3000


def uneven_slabs(k, world):
    """Random reads on every rank as a host batch; rank 1 takes them in H2D chunks of 3000 bytes (the knob chunk_bytes),
    so it has many slabs (slice views with a head offset) and the others one."""
    rng = np.random.default_rng(7000 + k)
    out = {}
    for r in range(world):
        reads = [rand_read(rng, int(rng.integers(k + 2, 400))) for _ in range(60)]
        out[r] = [(*join(reads + twins(rng, reads)), "host")]
    return out


def uneven_slabs_figures(k, world, batches, refs):
    return {"rank 1's batch spans many chunks": batches[UNEVEN_RANK][0][0].size > 5 * UNEVEN_CHUNK,
            "every rank has windows": all(x.pos.size > 0 for x in _flat(refs))}


def _dealt(b, o, world):
    """Contiguous shards of the reads, each as a host batch (first half) and a device batch."""
    n = o.size - 1
    out = {}
    for r in range(world):
        lo, hi = n * r // world, n * (r + 1) // world
        mid = (lo + hi) // 2
        out[r] = [(b[int(o[a]):int(o[z])].copy(), (o[a:z + 1] - o[a]).astype(np.uint64), kind)
                  for a, z, kind in ((lo, mid, "host"), (mid, hi, "device"))]
    return out


def edge_set(k, world):
    """common.edge_case_set() as it is, dealt to the ranks."""
    from common import edge_case_set

    return _dealt(*edge_case_set(), world)


def long_ragged(k, world):
    """common.long_ragged_set(k) as it is, dealt to the ranks."""
    from common import long_ragged_set

    return _dealt(*long_ragged_set(k), world)


def hot_owner(k, world):
    """common.hot_set() (one canonical k-mer past 65535 occurrences) dealt to the ranks. Its 800 poly-A reads of 150
    bases give 800 * (150 - k - 1) windows, which passes 65535 up to k = 67; above that n_poly is the smallest multiple
    of 100 that passes 66000 (k = 99: 1400 reads, 70000 windows)."""
    from common import hot_set

    per_read = 150 - k - 1
    n_poly = max(800, 100 * -(-66000 // (100 * per_read)))
    return _dealt(*hot_set(n_poly=n_poly), world)


def _has_windows(k, world, batches, refs):
    return {"some window is counted": sum(int(x.pos.size) for x in _flat(refs)) > 0,
            "every rank adds reads": all(len(batches[r]) > 0 for r in range(world))}


@dataclass
class Case:
    build: callable
    figures: callable
    env_by_rank: dict = field(default_factory=dict)
    multi_slab_ranks: tuple = ()   # ranks whose batches are several slabs: no tile-dependent equality there


CASES = {
    "one_window": Case(one_window, one_window_figures),
    "tile_straddle": Case(tile_straddle, tile_straddle_figures),
    "one_owner_long": Case(one_owner_long, one_owner_long_figures),
    "flank_bits": Case(flank_bits, flank_bits_figures),
    "flank_bits_n": Case(flank_bits_n, flank_bits_n_figures),
    "word_edges": Case(word_edges, word_edges_figures),
    "idle_and_empty": Case(idle_and_empty, idle_and_empty_figures),
    "uneven_slabs": Case(uneven_slabs, uneven_slabs_figures,
                         env_by_rank={UNEVEN_RANK: {"knob:chunk_bytes": str(UNEVEN_CHUNK)}},
                         multi_slab_ranks=(UNEVEN_RANK,)),
    "edge_set": Case(edge_set, _has_windows),
    "long_ragged": Case(long_ragged, _has_windows),
}
EXTRA_CASES = {"hot_owner": Case(hot_owner, _has_windows)}


@lru_cache(maxsize=None)
def built(name: str, k: int, world: int):
    """(batches, refs) of a case, built once per process."""
    case = CASES.get(name) or EXTRA_CASES[name]
    batches = case.build(k, world)
    return batches, refs_of(batches, k, world)
