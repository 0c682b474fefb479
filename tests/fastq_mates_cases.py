"""Read pairs from two mate texts (mhmkc_add_fastq_mates*, include/mhmkc.h): the rule restated in plain Python and
the inputs of test_fastq_mates_cases.py, test_fastq_mates.py and test_fastq_mates_files.py.

The rule (the reference's FastqReader over "r1.fq:r2.fq" alternates between the two files, src/fastq.cpp:509-518, and
merge_reads' loop stops at the first failed read, src/merge_reads.cpp:318-321): the texts A and B are read A[0], B[0],
A[1], B[1], ... until the text whose turn it is has nothing left; a text that ends inside a record fails only if that
record's turn comes. interleave_as_read(A, B) returns the one text holding exactly what was read, in that order, so
that the expected result of a two-text call is the one-text call (or the oracle's merge) on it. TEST INFRASTRUCTURE
ONLY."""
from __future__ import annotations

import common as c


def _lines(text: bytes):
    """The lines fgets would return: split at newlines, a last line without one kept, no empty line after the last."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def _records(text: bytes):
    """(complete records as 4-line lists, the lines of a cut last record or [])."""
    lines = _lines(text)
    full = len(lines) // 4 * 4
    return [lines[i:i + 4] for i in range(0, full, 4)], lines[full:]


def split_mates(interleaved: bytes):
    """An interleaved text's records 0, 2, 4, ... as text A and 1, 3, 5, ... as text B (complete records only)."""
    recs, _ = _records(interleaved)
    a = b"".join(b"\n".join(r) + b"\n" for r in recs[0::2])
    b = b"".join(b"\n".join(r) + b"\n" for r in recs[1::2])
    return a, b


def interleave_as_read(a: bytes, b: bytes) -> bytes:
    """What the alternating reader reads of A and B, as one text: turn by turn, a complete record is taken, a cut
    record is taken and ends the reading (the one-text call then fails inside it, as the reference does at that
    read), a text with nothing left ends the reading."""
    recs = (_records(a), _records(b))
    out = []
    p = 0
    while True:
        for full, tail in recs:  # A's turn, then B's
            if p < len(full):
                out.append(b"\n".join(full[p]) + b"\n")
                continue
            if tail:
                out.append(b"\n".join(tail) + b"\n")
            return b"".join(out)
        p += 1


def drop_records(text: bytes, n: int) -> bytes:
    """text without its last n records."""
    recs, _ = _records(text)
    return b"".join(b"\n".join(r) + b"\n" for r in recs[:len(recs) - n])


def cut_tail(text: bytes, lines_kept: int = 2) -> bytes:
    """text whose last record keeps only its first lines_kept lines (a text that ends inside a record)."""
    recs, _ = _records(text)
    return b"".join(b"\n".join(r) + b"\n" for r in recs[:-1]) + b"\n".join(recs[-1][:lines_kept]) + b"\n"


def skew_cases(n_pairs: int = 40, seed: int = 71):
    """name -> (A, B, pairs expected, error expected as (kind, record in the alternating order) or None): the count
    skews and truncations of the rule."""
    a, b = split_mates(c.paired_fastq_text(n_pairs, seed=seed))
    n = n_pairs
    return {
        "equal": (a, b, n, None),
        "a_longer_by_3": (a, drop_records(b, 3), n - 3, None),        # A[n-3] is read and checked, not added
        "b_longer_by_3": (drop_records(a, 3), b, n - 3, None),        # nothing of B[n-3] is read
        "empty_a": (b"", b, 0, None),
        "empty_b": (a, b"", 0, None),                                 # A[0] is read and checked
        "both_empty": (b"", b"", 0, None),
        # A ends inside record n-1 and B has a record n-1... but A's turn comes first
        "cut_a_turn_comes": (cut_tail(a), b, n - 1, ("trunc", 2 * (n - 1))),
        # B ends inside record n-1, A has its record n-1: A[n-1] is read, then B's cut record
        "cut_b_turn_comes": (a, cut_tail(b), n - 1, ("trunc", 2 * (n - 1) + 1)),
        # A ends inside record n-1, but B ran out two records earlier: B's turn n-3 ends the reading first
        "cut_a_turn_does_not_come": (cut_tail(a), drop_records(b, 3), n - 3, None),
        # B ends inside record n-1, A ran out earlier
        "cut_b_turn_does_not_come": (drop_records(a, 3), cut_tail(b), n - 3, None),
    }


def trim_mate2(b_text: bytes, keep: float = 1 / 3) -> bytes:
    """Text B with every record's sequence and quality lines cut to about `keep` of their length (trimmed mates: fewer
    bytes per record than A's)."""
    recs, _ = _records(b_text)
    out = []
    for idl, s, plus, q in recs:
        n = max(1, int(len(s) * keep))
        out.append(b"\n".join((idl, s[:n], plus, q[:n])) + b"\n")
    return b"".join(out)


def assert_equals_oracle(cnt, a: bytes, b: bytes, k: int, qual_offset: int = 33, table: bool = True, what: str = ""):
    """The counter, after a two-text call on (a, b) and before finish, against the oracle's merge of
    interleave_as_read(a, b): PackedReads bytes and offsets, the four pair statistics, reads and bases, and (table) the
    finished table against the oracle's count of those PackedReads."""
    import oracle_lib as O
    pb, po, pst = O.merge_fastq(interleave_as_read(a, b), qual_offset)
    gb, go = cnt.fastq_packed()
    st = cnt.stats()
    assert len(go) == len(po) and (go == po).all(), what
    assert (gb == pb).all(), what
    for key in ("pairs", "merged", "ambiguous", "overlap_bases"):
        assert st["fq_" + key] == pst[key], (what, key)
    assert st["reads"] == len(po) - 1 and st["bases"] == int(po[-1]), what
    if table:
        cnt.finish()
        got = cnt.fetch().sorted()
        keys, counts, left, right = O.kcount(pb, po, k).fetch()
        assert (got.keys == keys).all() and (got.counts == counts).all(), what
        assert (got.left == left).all() and (got.right == right).all(), what
    return pst
