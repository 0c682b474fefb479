"""Constructed FASTQ texts for the single-end front end (k_fq_count, k_fq_lines, k_fq_records, k_fq_pack in
mhm2_proxy_amd/csrc/fastq.hip): every text is built so that a chosen byte lies at a chosen absolute offset, or a chosen
record at a chosen place of its wave, which the generated texts of tests/test_fastq.py reach by accident or not at all.
TEST INFRASTRUCTURE ONLY.

The parser gives 16 bytes to a lane, 1024 to a wave and 4096 to a workgroup (chunk). A newline's offset p is on a
`lane` boundary when p % 16 == 15 (and not more), on a `wave` boundary when p % 1024 == 1023 (and not more), on a
`chunk` boundary when p % 4096 == 4095; `end` is the text's last byte (or, for a text without a final newline, the
place where that newline would be). The trailing-whitespace walk of the line that ends at p reads backwards from p - 1:
the lane's own bytes, then one byte of the lane below (`dpp`; from memory for lane 0 of a wave: `mem0`), then memory
(`mem`). A Case carries what it was built for as data (claims, pack claims, wave groups, the expected error);
check_case() asserts all of it from the text's bytes, not from the builders' arithmetic.

Groups (the letters of tests/test_fastq_cases.py): a first character of the next line, b trailing whitespace, c newline
density and text sizes, d the line length limit, e k_fq_pack's alignment cross, f mixed lengths within a wave, g pack4's
paths, h read names, i error selection."""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, replace

import oracle_lib as O

WS = b" \t\v\f\r"
KINDS = ("id", "seq", "plus", "qual")
BOUNDS = ("lane", "wave", "chunk")
FQ_MAX_LINE = 2045
RUNS = (1, 2, 15, 16, 17, 33)
# (run length, run start - boundary): the run starts 0, 1 or 2 bytes before the 16-byte boundary B, its newline is in
# the lane that starts at B (so a run that starts 2 bytes before B has 2 characters at the least)
EDGE_RUNS = ((1, 0), (1, -1), (2, 0), (2, -1), (2, -2), (3, -2), (15, 0), (16, -1), (17, -2))
IUPAC = b"NURYKMSWBDHV"
ACCEPTED = b"ACGT" + IUPAC
E_LENS = tuple(range(0, 10)) + tuple(range(60, 69)) + tuple(range(124, 133))
E_FULL = (5, 64, 65)  # lengths that meet every (s, sequence mod 4, quality mod 4)
F_GROUPS = ((2045, 0, 1, 64), (0, 0, 0, 2045), (65, 2045, 3, 128))


def seq_of(L: int, i: int = 0) -> bytes:
    return bytes(b"ACGTN"[(i + j) % 5] for j in range(L))


def qual_of(L: int, qoff: int = 33, i: int = 0) -> bytes:
    """qualities offset + (j mod 31): with seq_of's bases every output byte differs from its neighbours"""
    return bytes(qoff + (i + j) % 31 for j in range(L))


def ws_run(n: int, k: int = 0) -> bytes:
    """n whitespace characters, cycling through all five kinds from the k-th on"""
    return bytes(WS[(k + j) % 5] for j in range(n))


def classify(p: int):
    """the boundary kind of a newline at offset p"""
    return "chunk" if p % 4096 == 4095 else "wave" if p % 1024 == 1023 else "lane" if p % 16 == 15 else None


def classify_edge(B: int):
    """the kind of the 16-byte boundary B (the first byte of a lane)"""
    return classify(B - 1) if B > 0 else None


def next_off(minpos: int, kind: str) -> int:
    p = minpos
    while classify(p) != kind:
        p += 1
    return p


def source(pos: int, q: int) -> str:
    """where k_fq_lines takes byte q from while it walks back from the newline at pos"""
    base = pos & ~15
    if q < 0:
        return "start"
    if q >= base:
        return "own"
    if q == base - 1:
        return "dpp" if (pos >> 4) & 63 else "mem0"
    return "mem"


@dataclass(frozen=True)
class Rec:
    name: bytes = b"@r"
    seq: bytes = b""
    qual: bytes = b""
    plus: bytes = b"+"
    ws: tuple = (b"", b"", b"", b"")  # trailing whitespace of the id, sequence, '+' and quality lines

    def lines(self):
        return [self.name + self.ws[0], self.seq + self.ws[1], self.plus + self.ws[2], self.qual + self.ws[3]]

    def text(self) -> bytes:
        return b"".join(ln + b"\n" for ln in self.lines())

    def nl_off(self, line: int) -> int:
        """the offset of the line's newline from the record's first byte"""
        return sum(len(ln) + 1 for ln in self.lines()[:line + 1]) - 1

    def with_ws(self, line: int, run: bytes) -> "Rec":
        w = list(self.ws)
        w[line] = run
        return replace(self, ws=tuple(w))


def rec(L: int, i: int = 0, qoff: int = 33, name: bytes = b"@r") -> Rec:
    return Rec(name, seq_of(L, i), qual_of(L, qoff, i))


@dataclass(frozen=True)
class Claim:
    pos: int             # the newline's offset (the text's size for a last line without one)
    line: str            # the line kind that ends there
    boundary: str | None  # lane / wave / chunk
    end: bool = False    # the text's last byte (or the missing final newline)
    ws: int = 0          # trailing whitespace of that line
    edge: str | None = None  # the run was placed against a 16-byte boundary B of this kind ...
    rel: int | None = None   # ... and starts at B + rel


@dataclass(frozen=True)
class PackClaim:
    rec: int
    L: int
    s: int    # output misalignment: the bases before the record mod 4
    sa: int   # the sequence line's address mod 4
    qa: int   # the quality line's address mod 4


@dataclass
class Case:
    group: str
    name: str
    text: bytes
    claims: tuple = ()
    packs: tuple = ()
    groups: tuple = ()        # (first record, (four lengths)): four records that share a wave of k_fq_pack
    error: tuple | None = None  # (kind, record) where the reference dies
    n_rec: int | None = None  # records of a valid text
    qoff: int = 33
    literal: bool = True      # the literal restatement applies (it has no line buffer: not in group d)

    @property
    def valid(self) -> bool:
        return self.error is None


class Text:
    """A text under construction. fill_to() emits valid filler records up to an offset, place() puts a record so that
    one of its newlines lands on an offset."""

    def __init__(self, qoff: int = 33):
        self.b = bytearray()
        self.qoff = qoff
        self.nrec = 0
        self.claims: list = []

    @property
    def pos(self) -> int:
        return len(self.b)

    def add(self, r: Rec) -> int:
        self.b += r.text()
        self.nrec += 1
        return self.nrec - 1

    def raw(self, data: bytes) -> None:
        self.b += data

    def fill_to(self, target: int) -> None:
        """Valid filler records ('@xxxx' names without space or tab, 1..8 bases) so that the next record starts at
        target: short ones, then one whose id is stretched to take the exact rest. A record of k id characters and L
        bases takes k + 2 L + 6 bytes, 9 at the least."""
        gap = target - self.pos
        if gap == 0:
            return
        assert gap >= 9, f"a gap of {gap} bytes holds no record"
        while gap >= 40:
            L = 1 + self.nrec % 8
            k = max(3, min(1000, gap - 2 * L - 6 - 15))
            self.add(Rec(b"@" + b"x" * k, seq_of(L, self.nrec), qual_of(L, self.qoff, self.nrec)))
            gap = target - self.pos
        L = 1 if gap < 19 else 1 + self.nrec % 4
        k = gap - 2 * L - 6
        assert 1 <= k <= FQ_MAX_LINE - 1
        self.add(Rec(b"@" + b"x" * k, seq_of(L, self.nrec), qual_of(L, self.qoff, self.nrec)))
        assert self.pos == target

    def place(self, r: Rec, line: int, target: int, stretch: bool = False) -> int:
        """Put r so that the newline of its line `line` is at offset target: with filler records in front, or
        (stretch) by lengthening its id with 'x' (after fillers, when the gap is more than an id can take)."""
        start = target - r.nl_off(line)
        gap = start - self.pos
        assert gap >= 0
        if stretch:
            if gap > 29:
                self.fill_to(start - 20)
                gap = 20
            assert b" " not in r.name and b"\t" not in r.name and len(r.name) + gap <= FQ_MAX_LINE
            r = replace(r, name=r.name + b"x" * gap)
        else:
            self.fill_to(start)
        n = self.add(r)
        assert self.b[target] == 10
        return n

    def room(self, r: Rec, line: int, stretch: bool = False) -> int:
        """the lowest offset place() can put that newline at"""
        return self.pos + r.nl_off(line) + (0 if stretch else 9)

    def claim(self, pos: int, line: str, **kw) -> None:
        self.claims.append(Claim(pos, line, classify(pos), **kw))

    def case(self, group: str, name: str, final_nl: bool = True, **kw) -> Case:
        b = bytes(self.b)
        if not final_nl:
            assert b.endswith(b"\n")
            b = b[:-1]
        if "error" not in kw or kw["error"] is None:
            kw.setdefault("n_rec", self.nrec)
        return Case(group, name, b, claims=tuple(self.claims), qoff=self.qoff, **kw)


# --------------------------------------------------------------------------------------------------
# what a text holds, read from its bytes


def measure(text: bytes, pos: int):
    """-> (line kind, boundary kind, is the end, trailing whitespace) of the line that ends at pos"""
    n = len(text)
    if pos == n:
        assert n and text[-1] != 10, "the claim is a missing final newline, the text has one"
    else:
        assert text[pos] == 10, f"no newline at {pos}"
    t = 0
    while pos - 1 - t >= 0 and text[pos - 1 - t] in WS:
        t += 1
    return KINDS[text.count(b"\n", 0, pos) % 4], classify(pos), pos >= n - 1, t


def parse(text: bytes):
    """-> [(L, sequence start, quality start, quality L)] of the complete records (plain split and rstrip)"""
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    starts, p = [], 0
    for ln in lines:
        starts.append(p)
        p += len(ln) + 1
    return [(len(lines[r + 1].rstrip(WS)), starts[r + 1], starts[r + 3], len(lines[r + 3].rstrip(WS)))
            for r in range(0, len(lines) // 4 * 4, 4)]


def pack_layout(text: bytes):
    """-> [(L, s, sa, qa)] per record: what k_fq_pack meets (a text buffer and an output aligned to 4 bytes)"""
    out, nb = [], 0
    for L, sb, qb, _ in parse(text):
        out.append((L, nb % 4, sb % 4, qb % 4))
        nb += L
    return out


def walk_sources(c: Case):
    """-> {(line, boundary or None, 'ws' | 'stop', source)}: for every claimed newline inside the text the source of
    the deepest whitespace byte and of the byte that stops the walk"""
    seen = set()
    for cl in c.claims:
        if cl.pos >= len(c.text):
            continue
        if cl.ws:
            seen.add((cl.line, cl.boundary, "ws", source(cl.pos, cl.pos - cl.ws)))
        seen.add((cl.line, cl.boundary, "stop", source(cl.pos, cl.pos - cl.ws - 1)))
    return seen


def check_case(c: Case):
    """The case holds what it says it was built for. Returns the oracle's (bytes, offsets) of a valid case."""
    for cl in c.claims:
        line, boundary, end, t = measure(c.text, cl.pos)
        assert (line, boundary, end, t) == (cl.line, cl.boundary, cl.end, cl.ws), (c.name, cl, line, boundary, end, t)
        if cl.edge is not None:
            B = cl.pos - cl.ws - cl.rel
            assert cl.rel in (0, -1, -2) and classify_edge(B) == cl.edge and B <= cl.pos < B + 16, (c.name, cl, B)
    layout = pack_layout(c.text)
    for p in c.packs:
        assert layout[p.rec] == (p.L, p.s, p.sa, p.qa), (c.name, p, layout[p.rec])
    for first, lens in c.groups:
        assert first % 4 == 0 and tuple(x[0] for x in layout[first:first + 4]) == tuple(lens), (c.name, first, lens)
    if c.valid:
        b, o = O.fastq_pack(c.text, c.qoff)
        assert len(o) - 1 == c.n_rec, (c.name, len(o) - 1, c.n_rec)
        assert all(x[0] == x[3] for x in parse(c.text))
        return b, o
    try:
        O.fastq_pack(c.text, c.qoff)
    except O.FastqError as e:
        assert (e.kind, e.record) == c.error, (c.name, e.kind, e.record, c.error)
        return None
    raise AssertionError(f"{c.name}: the oracle accepts a text built to fail with {c.error}")


# --------------------------------------------------------------------------------------------------
# a. the first character of the next line


def _lead(T: Text) -> None:
    T.add(rec(5, 0, T.qoff, b"@lead"))


def cases_a():
    out = []
    for ch, line in ((b"@", "qual"), (b"+", "seq")):
        for kind in BOUNDS:
            for twin in (False, True):
                T = Text()
                _lead(T)
                if ch == b"@":  # the '@' of record x follows the quality newline of the record before it
                    P = rec(7, 1, name=b"@p")
                    tgt = next_off(T.room(P, 3), kind)
                    T.place(P, 3, tgt)
                    x = T.add(rec(6, 2, name=(b"#" if twin else b"@") + b"x1"))
                else:  # the '+' of record x follows its own sequence newline; the id is stretched
                    X = replace(rec(6, 2, name=b"@x2"), plus=(b"-" if twin else b"+") + b"x2")
                    tgt = next_off(T.room(X, 1, True), kind)
                    x = T.place(X, 1, tgt, stretch=True)
                T.add(rec(9, 3, name=b"@tail"))
                T.claim(tgt, line)
                err = ("id" if ch == b"@" else "plus", x) if twin else None
                what = "at" if ch == b"@" else "plus"
                out.append(T.case("a", f"a-first-{what}-{kind}{'-twin' if twin else ''}", error=err))
    # the id and '+' newlines on each boundary (their next characters are a base and a quality)
    for line in (0, 2):
        for kind in BOUNDS:
            T = Text()
            _lead(T)
            X = replace(rec(8, 4, name=b"@y"), plus=b"+y")
            tgt = next_off(T.room(X, line), kind)
            T.place(X, line, tgt)
            T.add(rec(3, 1, name=b"@tail"))
            T.claim(tgt, KINDS[line])
            out.append(T.case("a", f"a-{KINDS[line]}-newline-{kind}"))
    # the text's last byte is the newline on each boundary; the same text without it (end = n, rtrim_end)
    for kind in BOUNDS:
        for final_nl in (True, False):
            T = Text()
            _lead(T)
            X = rec(7, 2, name=b"@last")
            tgt = next_off(T.room(X, 3), kind)
            T.place(X, 3, tgt)
            T.claims.append(Claim(tgt, "qual", kind, end=True))
            out.append(T.case("a", f"a-end-{kind}{'' if final_nl else '-no-newline'}", final_nl=final_nl))
    return out


# --------------------------------------------------------------------------------------------------
# b. trailing whitespace runs


def _ws_rec(line: int, n: int, k: int, L: int = 6) -> Rec:
    r = replace(rec(L, k, name=b"@w%d" % k), plus=b"+w")
    return r.with_ws(line, ws_run(n, k))


def cases_b():
    out = []
    # runs that end at a newline on each boundary kind, on every line kind (sequence and quality lines are
    # asymmetric: whitespace after the one and not after the other)
    for line in range(4):
        for kind in BOUNDS:
            T = Text()
            _lead(T)
            for k, n in enumerate(RUNS):
                X = _ws_rec(line, n, k + line, L=5 + k)
                tgt = next_off(T.room(X, line), kind)
                T.place(X, line, tgt)
                T.claim(tgt, KINDS[line], ws=n)
            T.add(rec(4, 1, name=b"@tail"))
            out.append(T.case("b", f"b-run-{KINDS[line]}-{kind}"))
    # runs that start 0, 1 or 2 bytes before a lane, wave or chunk boundary
    for line in (0, 1, 3):
        for kind in BOUNDS:
            T = Text()
            _lead(T)
            for k, (n, rel) in enumerate(EDGE_RUNS):
                X = _ws_rec(line, n, k + 2 * line, L=4 + k % 5)
                B = next_off(T.room(X, line) + 2, kind) + 1  # a boundary of that kind with room for the record
                tgt = B + rel + n
                T.place(X, line, tgt)
                T.claim(tgt, KINDS[line], ws=n, edge=kind, rel=rel)
            T.add(rec(4, 2, name=b"@tail"))
            out.append(T.case("b", f"b-edge-{KINDS[line]}-{kind}"))
    # whitespace-only sequence and quality lines (L = 0), a '+' line followed by whitespace, CRLF on every line
    T = Text()
    _lead(T)
    for a, b in ((1, 40), (40, 1), (1, 1), (40, 40)):
        T.add(Rec(b"@empty", b"", b"", b"+", (b"", ws_run(a, a), b"", ws_run(b, b + 1))))
        T.add(rec(3, a, name=b"@between"))
    T.add(replace(rec(5, 1, name=b"@plusws"), ws=(b"", b"", b" \t\r", b"")))
    T.add(replace(rec(5, 2, name=b"@crlf"), ws=(b"\r", b"\r", b"\r", b"\r")))
    T.add(Rec(b"@emptyplain"))
    T.add(rec(2, 0, name=b"@tail"))
    out.append(T.case("b", "b-empty-lines"))
    # a last line without a newline that ends in whitespace: k_fq_records' rtrim_end
    for n in (1, 17):
        T = Text()
        _lead(T)
        T.add(rec(6, 1, name=b"@last").with_ws(3, ws_run(n, n)))
        T.claims.append(Claim(T.pos - 1, "qual", classify(T.pos - 1), end=True, ws=n))
        out.append(T.case("b", f"b-end-ws{n}-no-newline", final_nl=False))
    # " \n" in place of the id line and of the '+' line
    for line, kind in ((0, "id"), (2, "plus")):
        T = Text()
        _lead(T)
        T.add(rec(4, 1))
        r = rec(5, 2, name=b"@bad")
        x = T.nrec
        ls = r.lines()
        ls[line] = b" "
        T.raw(b"".join(ln + b"\n" for ln in ls))
        T.add(rec(4, 3))
        out.append(T.case("b", f"b-blank-{kind}-line", error=(kind, x)))
    return out


# --------------------------------------------------------------------------------------------------
# c. newline density and text sizes


def _sized(n: int, final_nl: bool) -> Case:
    T = Text()
    last = rec(6, 3, name=b"@last")
    size = len(last.text()) - (0 if final_nl else 1)
    if n - size >= 9:
        T.fill_to(n - size)
    else:
        assert n == size
    T.add(last)
    c = T.case("c", f"c-size-{n}{'' if final_nl else '-no-newline'}", final_nl=final_nl)
    assert len(c.text) == n
    c.claims = (Claim(n - 1 if final_nl else n, "qual", classify(n - 1 if final_nl else n), end=True),)
    return c


def cases_c():
    out = []
    for nl in (5000, 5001):  # every lane's popcount is 16, a wave's scan 1024
        T = Text()
        _lead(T)
        T.raw(b"\n" * nl)
        out.append(T.case("c", f"c-{nl}-newlines", error=("id", 1)))
    # lines of FQ_MAX_LINE characters back to back: waves without a newline, the fewest newlines a chunk can hold
    T = Text()
    for i in range(3):
        T.add(Rec(b"@" + b"x" * (FQ_MAX_LINE - 1), seq_of(FQ_MAX_LINE, i), qual_of(FQ_MAX_LINE, 33, i),
                  b"+" + b"y" * (FQ_MAX_LINE - 1)))
    out.append(T.case("c", "c-sparse-newlines"))
    # a chunk without any newline needs a line past the limit: the error is `long`, at that record
    T = Text()
    _lead(T)
    T.add(Rec(b"@long", seq_of(9000), qual_of(9000)))
    T.add(rec(3, 1))
    out.append(T.case("c", "c-chunk-without-newline", error=("long", 1), literal=False))
    for n in (160, 161, 175, 4095, 4096, 4097, 8192):
        for final_nl in (True, False):
            out.append(_sized(n, final_nl))
    return out


# --------------------------------------------------------------------------------------------------
# d. the line length limit


def cases_d():
    out = []
    for line in range(4):
        for N in (FQ_MAX_LINE - 1, FQ_MAX_LINE, FQ_MAX_LINE + 1):
            for cr in (False, True):  # the N characters of the line with and without a '\r' among them
                body = N - (1 if cr else 0)
                tail = b"\r" if cr else b""
                if line == 0:
                    X = rec(5, 1, name=b"@" + b"x" * (body - 1)).with_ws(0, tail)
                elif line == 2:
                    X = replace(rec(5, 1, name=b"@d"), plus=b"+" + b"p" * (body - 1)).with_ws(2, tail)
                else:  # the other of the sequence and quality lines holds as many characters, never more than the limit
                    L = body
                    X = Rec(b"@d", seq_of(L, 2), qual_of(L, 33, 2)).with_ws(line, tail)
                    if L > FQ_MAX_LINE:
                        cut = {"qual": X.qual[:FQ_MAX_LINE]} if line == 1 else {"seq": X.seq[:FQ_MAX_LINE]}
                        X = replace(X, **cut)
                assert len(X.lines()[line]) == N
                T = Text()
                _lead(T)
                x = T.add(X)
                T.add(rec(4, 3, name=b"@tail"))
                err = ("long", x) if N > FQ_MAX_LINE else None
                out.append(T.case("d", f"d-{KINDS[line]}-{N}{'-cr' if cr else ''}", error=err, literal=False))
    return out


# --------------------------------------------------------------------------------------------------
# e. k_fq_pack's alignment cross


def e_wanted():
    """(L, s, sa, qa): every triple at E_FULL, every s (with varying line addresses) at the other lengths"""
    w = []
    for L in E_LENS:
        if L in E_FULL:
            w += [(L, s, sa, qa) for s in range(4) for sa in range(4) for qa in range(4)]
        else:
            w += [(L, s, (s + L) % 4, (2 * s + L + 1) % 4) for s in range(4)]
    return w


def records_e(qoff: int = 33):
    """-> (records, [(record index, L, s, sa, qa)]) in an order that yields the wanted alignments when the text
    starts at offset 0 with no bases before it: a pad record sets s, the id length sa, and trailing whitespace on
    the sequence line or the '+' line's length (in turn) qa"""
    recs, claims, pos, nb = [], [], 0, 0

    def push(r):
        nonlocal pos, nb
        recs.append(r)
        pos += len(r.text())
        nb += len(r.seq)

    for n, (L, s, sa, qa) in enumerate(e_wanted()):
        if nb % 4 != s:
            Lp = (s - nb) % 4
            push(rec(Lp + (4 if n % 3 == 0 else 0), n, qoff, b"@pad"))
        k = (sa - (pos + 3)) % 4  # the id is '@e' + k 'x', then its newline
        name = b"@e" + b"x" * k
        d = (qa - (pos + len(name) + 1 + L + 1 + 1 + 1)) % 4  # bytes still missing in front of the quality line
        r = Rec(name, seq_of(L, n), qual_of(L, qoff, n + 1))
        r = r.with_ws(1, ws_run(d, n)) if n % 2 else replace(r, plus=b"+" + b"p" * d)
        claims.append((len(recs), L, s, sa, qa))
        push(r)
    return recs, claims


def batch_text(recs) -> bytes:
    return b"".join(r.text() for r in recs)


def shuffled(recs, seed: int = 20240611):
    rs = list(recs)
    random.Random(seed).shuffle(rs)
    return rs


def cases_e():
    out = []
    for qoff in (33, 64):
        recs, claims = records_e(qoff)
        out.append(Case("e", f"e-alignment-cross-{qoff}", batch_text(recs), packs=tuple(PackClaim(*c) for c in claims),
                        n_rec=len(recs), qoff=qoff))
    return out


# --------------------------------------------------------------------------------------------------
# f. mixed lengths within a wave and a block (16 records per workgroup, 4 per wave)


def f_groups():
    """every rotation of every group"""
    return [g[i:] + g[:i] for g in F_GROUPS for i in range(4)]


def records_f(groups, extra: int):
    recs = []
    for g in groups:
        recs += [rec(L, len(recs), name=b"@f%d" % len(recs)) for L in g]
    recs += [rec(1 + i % 7, i, name=b"@s%d" % i) for i in range(extra)]
    return recs


def cases_f():
    G = f_groups()
    out = []
    for name, groups, extra in (("f-all-groups", G, 0), ("f-partial-block-1", G[:4], 1),
                                ("f-partial-block-15", G[4:], 15)):
        recs = records_f(groups, extra)
        assert len(recs) % 16 == extra
        out.append(Case("f", name, batch_text(recs), groups=tuple((4 * i, g) for i, g in enumerate(groups)),
                        n_rec=len(recs)))
    return out


# --------------------------------------------------------------------------------------------------
# g. pack4's paths


def special_quals(qoff: int):
    vals = [qoff - 1, qoff, qoff + 30, qoff + 31, qoff + 32, qoff + 63, qoff + 64, qoff + 94, 0x7f, 0x80, 0x81, 0xff]
    return sorted({v for v in vals if v <= 0xff})


def _special_positions(n: int):
    """(record length, position of the special byte): each position of a dword of an 8-base record (both dwords in
    turn), and the last valid byte of a partial last dword"""
    return [(8, p + (4 if (n + p) % 2 else 0)) for p in range(4)] + [(5, 4), (6, 5), (7, 6)]


def records_g(qoff: int):
    """valid records: every IUPAC code among A/C/G/T, every special quality among ordinary ones (the dword then takes
    the per-byte path and its ordinary bytes must still come out right), whitespace just past the sequence"""
    recs = []
    for n, ch in enumerate(IUPAC):
        for L, p in _special_positions(n):
            s = bytearray(seq_of(L, n).replace(b"N", b"G"))
            s[p] = ch
            recs.append(Rec(b"@base%c%d" % (ch, p), bytes(s), qual_of(L, qoff, n)))
    for n, q in enumerate(special_quals(qoff)):
        for L, p in _special_positions(n):
            if q in WS and p == L - 1:
                continue  # a trailing whitespace character is no quality
            ql = bytearray(qual_of(L, qoff, n))
            ql[p] = q
            recs.append(Rec(b"@qual%02x-%d" % (q, p), seq_of(L, n), bytes(ql)))
    for n, w in enumerate((b"\r", b"\t", b" \r", b"\t\v\f")):
        for L in (4, 5, 7, 8):
            recs.append(rec(L, n, qoff, b"@past").with_ws(1, w))
    recs.append(Rec(b"@accepted", ACCEPTED, qual_of(len(ACCEPTED), qoff)))
    return recs


def _error_text(bad: Rec, before: int = 2, after: int = 2):
    T = Text()
    for i in range(before):
        T.add(rec(5 + i, i, name=b"@ok%d" % i))
    x = T.add(bad)
    for i in range(after):
        T.add(rec(3 + i, i, name=b"@after%d" % i))
    return T, x


def cases_g():
    out = []
    for qoff in (33, 64):
        recs = records_g(qoff)
        out.append(Case("g", f"g-valid-{qoff}", batch_text(recs), n_rec=len(recs), qoff=qoff))
    # every byte value as a base: the accepted ones are g-valid's last record, each other one a text of its own
    for v in range(256):
        if v == 10 or v in ACCEPTED:
            continue
        s = bytearray(b"ACGTACGT")
        s[2 + v % 4] = v
        T, x = _error_text(Rec(b"@sweep", bytes(s), qual_of(8)))
        out.append(T.case("g", f"g-base-{v:02x}", error=("char", x)))
    # a refused byte at each dword position and as the last valid byte, in a middle record
    for n, v in enumerate(b"aIQFX\xc1"):
        for L, p in _special_positions(n):
            s = bytearray(seq_of(L, n))
            s[p] = v
            T, x = _error_text(Rec(b"@refused", bytes(s), qual_of(L)), before=2 + n % 3)
            out.append(T.case("g", f"g-refused-{v:02x}-len{L}-at{p}", error=("char", x)))
    return out


# --------------------------------------------------------------------------------------------------
# h. read names


NAME_TABLE = (
    (b"@ab 1:N:0:", True), (b"@ab 1:N:0", False), (b"@abcd/1 x", True), (b"@abc/1 x", True), (b"@a\tb c", False),
    (b"@a b\t1:N:0:x", True), (b"@a b\tc", False), (b"@aR1", True), (b"@a/1", True), (b"@", True),
    (b"@ab c/1\t1:N:0:1", True), (b"@0123456789abcd 3:N:0:1", False), (b"@0123456789abcdefg\t2:Y:18:A", False),
)


def names_h():
    """[(id line, accepted)]"""
    names = list(NAME_TABLE)
    for i in (14, 15, 16, 17, 31, 32):  # the first space or tab at index i of the name after the '@'
        for sep in (b" ", b"\t"):
            stem = b"@" + bytes(b"abcdefghijklmnopqrstuvw"[j % 23] for j in range(i))
            names += [(stem + sep + b"1:N:0:ACGT", True), (stem + sep + b"2:Y:18:A", False), (stem + sep + b"c", False),
                      (stem + sep + b"1:N:0", False), (stem + sep + b"2:N:0:", True),   # len == ep + 6, ep + 7
                      (stem[:-2] + b"/2" + sep + b"c", True)]
    for t in (20, 40):  # a space in the first 16 characters, the first tab in the second or third 16: the tab wins
        stem = b"@ab cd" + b"e" * (t - 5)
        assert stem[1:].index(b" ") == 2 and len(stem) - 1 == t
        names += [(stem + b"\t1:N:0:x", True), (stem + b"\tzz", False),
                  (b"@ab 1:N:0:x" + b"e" * (t - 10) + b"\tq", False)]
    # two separators of a kind: the first one counts (with the last one the verdicts would be the other way round)
    for sep in (b" ", b"\t"):
        for stem in (b"@abcd", b"@" + b"x" * 18, b"@" + b"x" * 30):
            names += [(stem + sep + b"1:N:0:x" + sep + b"y", True), (stem + sep + b"cd/1" + sep + b"x", False)]
    return names


def cases_h():
    names = names_h()
    good = [Rec(nm, seq_of(3 + i % 5, i), qual_of(3 + i % 5, 33, i)) for i, (nm, ok) in enumerate(names) if ok]
    out = [Case("h", "h-accepted-names", batch_text(good), n_rec=len(good))]
    for i, (nm, ok) in enumerate(names):
        if not ok:
            T, x = _error_text(rec(6, i, name=nm), before=1 + i % 3)
            out.append(T.case("h", f"h-rejected-{i}", error=("name", x)))
    return out


# --------------------------------------------------------------------------------------------------
# i. error selection: texts with two or three errors


def _with_errors(n: int, errs: dict) -> bytes:
    """n records; errs: record -> 'char' | 'len' | 'name'"""
    out = []
    for i in range(n):
        r = rec(4 + i % 9, i, name=b"@i%d" % i)
        kind = errs.get(i)
        if kind == "char":
            r = replace(r, seq=b"x" + r.seq[1:])
        elif kind == "len":
            r = replace(r, qual=r.qual[:-1])
        elif kind == "name":
            r = replace(r, name=b"@i%d 3:N:0:1" % i)
        out.append(r)
    return batch_text(out)


def cases_i():
    out = [
        Case("i", "i-char3-len5", _with_errors(8, {3: "char", 5: "len"}), error=("char", 3)),
        Case("i", "i-len3-char5", _with_errors(8, {3: "len", 5: "char"}), error=("len", 3)),
        Case("i", "i-char-17-40-300", _with_errors(310, {17: "char", 40: "char", 300: "char"}), error=("char", 17)),
        Case("i", "i-char-300-40-len-17", _with_errors(310, {17: "len", 40: "char", 300: "char"}), error=("len", 17)),
        Case("i", "i-two-in-a-wave", _with_errors(40, {22: "char", 23: "char"}), error=("char", 22)),
        Case("i", "i-two-in-a-wave-upper-first", _with_errors(40, {23: "char", 26: "char"}), error=("char", 23)),
        Case("i", "i-name2-truncated", _with_errors(6, {2: "name"}) + b"@cut\nACGT\n", error=("name", 2)),
    ]
    dangling = (b"@cut", b"ACGT", b"+")
    for k in (1, 2, 3):  # truncation alone after 3 whole records
        for final_nl in (True, False):
            t = _with_errors(3, {}) + b"\n".join(dangling[:k]) + (b"\n" if final_nl else b"")
            pos = len(t) - 1 if final_nl else len(t)
            out.append(Case("i", f"i-truncated-{k}-lines{'' if final_nl else '-no-newline'}", t,
                            claims=(Claim(pos, KINDS[k - 1], classify(pos), end=True),), error=("trunc", 3)))
    return out


# --------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f() + cases_g() + cases_h() + cases_i()
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def group(g: str, valid=None):
    return [c for c in all_cases() if c.group == g and (valid is None or c.valid == valid)]
