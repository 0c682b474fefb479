"""Single-rank read extraction (k_read_start_bits, load_tile, the walks and the staged scatter inside k_extract_scatter
and k_extract_hist) at its span, group, tile, view and round edges: the cases of
tests/extract_cases.py through KmerCounter, the whole table and the occurrence, distinct and purged counts against the
oracle's. Every case is decisive (each key occurs exactly twice at dmin_thres = 2), so one wrong "extension countable"
bit, neighbour base, key or dropped window changes a row. tests/test_extract_cases.py proves that, and that every case
holds its edge, on the CPU."""
import numpy as np
import pytest

import extract_cases as E
import mhm2_proxy_amd as m
from common import assert_tables_equal

pytestmark = pytest.mark.gpu


def count(batches, k, how="host", **kw):
    """(table, stats) of the batches [(bytes, offsets)] through one KmerCounter: each as a host batch, as five host
    batches of whole reads, or as device tensors."""
    with m.KmerCounter(k, **kw) as c:
        for b, o in batches:
            o = np.asarray(o, dtype=np.uint64)
            if how == "device":
                import torch

                c.add_tensors(torch.from_numpy(b).cuda(), torch.from_numpy(o.astype(np.int64)).cuda(), n_bases=int(o[-1]))
            elif how == "split5":
                n = o.size - 1
                cuts = [n * i // 5 for i in range(6)]
                for a, z in zip(cuts[:-1], cuts[1:]):
                    c.add_packed_reads(b[int(o[a]):int(o[z])], (o[a:z + 1] - o[a]).astype(np.uint64))
            else:
                c.add_packed_reads(b, o)
        c.finish()
        return c.fetch(), c.stats()


def check(got, st, name, k, qcut, what):
    keys, counts, left, right, ost = E.oracle(name, k, qcut)
    assert_tables_equal(got, m.KmerTable(k, keys, counts, left, right), what)
    assert st["count_sum"] == st["owned_records"] == st["occurrences"], what
    assert st["distinct"] == st["n_out"] + st["purged"] and st["dropped"] == 0, what
    got3, want3 = [st[key] for key in ("occurrences", "distinct", "purged")], \
        [ost[key] for key in ("occurrences", "distinct", "purged")]
    assert got3 == want3, f"{what}: (occurrences, distinct, purged) {got3}, the oracle's {want3}"


def run_plain_cases(k, failures):
    """Every case but the host-chunk ones, each batch as one host batch, at every quality cutoff of the case."""
    for name in E.cases_for(k):
        case = E.CASES[name]
        if case.views:
            continue
        batches = [(bt.b, bt.o) for bt in E.built(name, k).batches]
        for qcut in case.qcuts:
            what = f"{name}, k={k}, qual_cutoff={qcut}"
            try:
                got, st = count(batches, k, qual_cutoff=qcut)
                check(got, st, name, k, qcut, what)
            except AssertionError as e:
                failures.append(f"[{what}] {e}")


def run_view_cases(k, knob, failures):
    """The host-chunk cases: as one host batch, in small H2D chunks sent as bytes (h2d_nib 0) and as nibbles (1, 2), as
    five add_packed_reads calls and as device tensors."""
    for name in E.cases_for(k):
        if not E.CASES[name].views:
            continue
        bu = E.built(name, k)
        bt = bu.batches[0]
        runs = [("one host batch", "host", None, None), ("five adds", "split5", None, None),
                ("device tensors", "device", None, None)]
        runs += [(f"chunk_bytes={c}, h2d_nib={nib}", "host", c, nib) for nib in (0, 1, 2)
                 for c in bu.extra["chunks"][min(nib, 1)]]
        for label, how, chunk, nib in runs:
            what = f"{name}, k={k}, {label}"
            knob("chunk_bytes", chunk or 0)
            knob("h2d_nib", -1 if nib is None else nib)
            try:
                got, st = count([(bt.b, bt.o)], k, how=how)
                check(got, st, name, k, E.QCUT, what)
                if chunk:
                    n = len(E.host_chunks(bt.o, chunk, nib))
                    assert n >= 4 and st["h2d_chunks"] == n, \
                        f"{what}: {st['h2d_chunks']} chunks, extract_cases.host_chunks gives {n}"
            except AssertionError as e:
                failures.append(f"[{what}] {e}")
        knob("chunk_bytes", 0)
        knob("h2d_nib", -1)


def report(failures):
    assert not failures, f"{len(failures)} runs failed:\n" + "\n".join(failures)


@pytest.mark.parametrize("k", E.KS)
def test_extract_edges(k, knob):
    """Every case of extract_cases.CASES: span_phases, short_runs, tile_edges, data_end, flags (at qual_cutoff 0, 1, 20,
    31, 32), for two or more key words rounds, and views and views_dry (slice views whose head is 0, 1, 8 and 15 bytes,
    a first chunk without a counted window). The compact walk at k = 10 .. 21, the generic one-word walk at 22 and 31,
    the two-word walk at 33 .. 63 and walk_windows for three and four words, each at the k compiled into it and at
    others."""
    failures = []
    run_plain_cases(k, failures)
    run_view_cases(k, knob, failures)
    report(failures)


@pytest.mark.parametrize("k,name,value", [(21, "wide_records", 1), (63, "wide_records", 1), (33, "cb0_2", 7),
                                          (63, "cb0_2", 7)])
def test_extract_edges_other_walks(k, name, value, knob):
    """The key-word records (wide_records: walk_windows with the stored hash bits at k = 21 and 63), and the two-word
    walk with the coarse bits as a run-time value (cb0_2 = 7: at k = 33 and 63 the default 8 takes the walk with both
    compiled in)."""
    failures = []
    knob(name, value)
    run_plain_cases(k, failures)
    run_view_cases(k, knob, failures)
    report(failures)


@pytest.mark.parametrize("k", [21, 63, 77, 99])
def test_extract_edges_exact_layout(k, knob):
    """One k per key width with exact layouts (the knob exact): k_extract_hist sizes every segment from the same
    windows before k_extract_scatter fills them, so a window the two disagree on corrupts or loses a record."""
    failures = []
    knob("exact", 1)
    run_plain_cases(k, failures)
    report(failures)
