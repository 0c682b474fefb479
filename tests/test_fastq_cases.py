"""The single-end FASTQ front end (k_fq_count, k_fq_lines, k_fq_records, k_fq_pack; FastqReader::get_next_fq_record,
src/fastq.cpp:504-551, and the PackedRead constructor, src/packed_reads.cpp:73-109) on constructed texts
(tests/fastq_cases.py): the lane, wave, chunk and dword edges that the generated texts of tests/test_fastq.py reach by
accident or not at all.

CPU: every case holds what it was built for (check_case reads it from the text's bytes), the C oracle equals the
literal restatement on every case but those of the line limit (the literal one has no line buffer), and the list as
a whole covers the placements, walk-back sources and alignments it names.
GPU: one test per group a-k. Valid texts must equal the oracle in offsets and bytes; error texts must give the
oracle's error kind and record. Texts whose point is an absolute offset go one call each; batches of records (e-h) go
in listed and in a fixed shuffled order, so that a record's place in its wave and its output misalignment change."""
from __future__ import annotations

import functools
import re

import numpy as np
import pytest

import fastq_cases as F
import oracle_lib as O
import test_fastq as TF

CASES = F.all_cases()
GROUPS = "abcdefghi"
# error kind -> (code, what the message says)
MSG = {"id": ("MHMKC_EINVAL", "expected read name"), "plus": ("MHMKC_EINVAL", "expected '+'"),
       "name": ("MHMKC_EINVAL", "incorrect name format"), "len": ("MHMKC_EINVAL", "sequence length != quals length"),
       "trunc": ("MHMKC_EINVAL", "ends inside record"), "char": ("MHMKC_EBADCHAR", "illegal base character"),
       "long": ("MHMKC_EUNSUPPORTED", "line longer than")}
MISALIGN = (1, 2, 3, 4, 8, 15)
TAIL = (b"\n@A" * 6)[:16]  # what stands after a device text instead of zeros


@functools.lru_cache(maxsize=None)
def _ref(text: bytes, qoff: int = 33):
    """the oracle's (bytes, offsets) of a valid text; computed once and shared"""
    b, o = O.fastq_pack(text, qoff)
    b.setflags(write=False)
    o.setflags(write=False)
    return b, o


@functools.lru_cache(maxsize=None)
def _records(g: str, qoff: int):
    return tuple({"e": lambda: F.records_e(qoff)[0], "f": lambda: F.records_f(F.f_groups(), 0),
                  "g": lambda: F.records_g(qoff),
                  "h": lambda: [F.Rec(nm, F.seq_of(3 + i % 5, i), F.qual_of(3 + i % 5, qoff, i))
                                for i, (nm, ok) in enumerate(F.names_h()) if ok]}[g]())


def _batch(g: str, qoff: int, order: str) -> bytes:
    recs = _records(g, qoff)
    return F.batch_text(F.shuffled(recs) if order == "shuffled" else recs)


# --------------------------------------------------------------------------------------------------
# CPU


@pytest.mark.parametrize("n", range(len(CASES)), ids=[c.name for c in CASES])
def test_case_structure(n):
    F.check_case(CASES[n])


@pytest.mark.parametrize("g", [g for g in GROUPS if g != "d"])
def test_oracle_equals_literal_on_cases(g):
    cs = [c for c in F.group(g) if c.literal]
    assert cs
    for c in cs:
        if c.valid:
            b, o = _ref(c.text, c.qoff)
            lb, lo = TF.literal_pack(c.text, c.qoff)
            assert list(o) == list(lo) and b.tobytes() == lb.tobytes(), c.name
        else:
            with pytest.raises(O.FastqError) as e1:
                O.fastq_pack(c.text, c.qoff)
            with pytest.raises(O.FastqError) as e2:
                TF.literal_pack(c.text, c.qoff)
            assert (e1.value.kind, e1.value.record) == (e2.value.kind, e2.value.record) == c.error, c.name
    if g in "efgh":  # the shuffled batches
        for qoff in (33, 64):
            t = _batch(g, qoff, "shuffled")
            b, o = _ref(t, qoff)
            lb, lo = TF.literal_pack(t, qoff)
            assert list(o) == list(lo) and b.tobytes() == lb.tobytes(), (g, qoff)


def test_case_list_covers_what_it_names():
    """The placements, walk-back sources, run lengths, alignments, wave groups, byte values and names over the whole
    list, read from the texts: a later edit to a builder cannot silently drop an edge."""
    assert sum(len(c.text) for c in CASES) < 1_500_000
    placed, walks, runs, edges = set(), set(), set(), set()
    for c in CASES:
        for cl in c.claims:
            line, boundary, end, t = F.measure(c.text, cl.pos)
            if boundary:
                placed.add((line, boundary))
                runs.add((line, boundary, t))
            if end:
                placed.add((line, "end"))
            if cl.edge:
                edges.add((line, cl.edge, cl.rel))
        walks |= F.walk_sources(c)
    for line in F.KINDS:
        for b in F.BOUNDS + ("end",):
            assert (line, b) in placed, (line, b)
        for b in F.BOUNDS:
            for n in F.RUNS:
                assert (line, b, n) in runs, (line, b, n)
    for line in ("id", "seq", "qual"):
        for b in F.BOUNDS:
            for rel in (0, -1, -2):
                assert (line, b, rel) in edges, (line, b, rel)
        for what in ("ws", "stop"):  # the deepest whitespace byte and the byte that ends the walk, from each source
            for src in ("own", "dpp", "mem0", "mem"):
                assert any(w[0] == line and w[2:] == (what, src) for w in walks), (line, what, src)
    # k_fq_pack: (L, s, sequence mod 4, quality mod 4)
    for qoff in (33, 64):
        (c,) = [c for c in F.group("e") if c.qoff == qoff]
        seen = set(F.pack_layout(c.text))
        for L in F.E_LENS:
            for s in range(4):
                assert any(x[:2] == (L, s) for x in seen), (L, s)
        for L in F.E_FULL:
            for s in range(4):
                for sa in range(4):
                    for qa in range(4):
                        assert (L, s, sa, qa) in seen, (L, s, sa, qa)
    # waves of four records: every rotation of every group at a multiple of 4, partial last blocks
    rot = set()
    for c in F.group("f"):
        lens = [x[0] for x in F.pack_layout(c.text)]
        rot |= {tuple(lens[i:i + 4]) for i in range(0, len(lens) - 3, 4)}
    assert {g[i:] + g[:i] for g in F.F_GROUPS for i in range(4)} <= rot
    assert {c.n_rec % 16 for c in F.group("f")} == {0, 1, 15}
    # bases: every byte value but '\n' is in the sweep, as accepted or as refused
    swept = {int(c.name[-2:], 16) for c in F.group("g") if c.name.startswith("g-base-")}
    assert swept | set(F.ACCEPTED) | {10} == set(range(256)) and not swept & set(F.ACCEPTED)
    for qoff in (33, 64):
        (c,) = [c for c in F.group("g", valid=True) if c.qoff == qoff]
        quals = {q for ln in c.text.split(b"\n")[3::4] for q in ln}
        assert set(F.special_quals(qoff)) <= quals and {0x7f, 0x80, 0x81, 0xff, qoff - 1, qoff + 32} <= quals
        assert set(F.ACCEPTED) <= {s for ln in c.text.split(b"\n")[1::4] for s in ln}
    # names: the table, and a first separator at each index around the 16-character steps
    names = dict(F.names_h())
    assert all(names[nm] == ok for nm, ok in F.NAME_TABLE)
    for i in (14, 15, 16, 17, 31, 32):
        for sep in b" \t":
            for ok in (True, False):
                assert any(v == ok and len(nm) > i + 1 and nm[i + 1] == sep and
                           not set(nm[1:i + 1]) & set(b" \t") for nm, v in names.items()), (i, sep, ok)
    kinds = {c.error[0] for c in CASES if not c.valid}
    assert kinds == set(MSG)


# --------------------------------------------------------------------------------------------------
# GPU


def _counter(qoff: int = 33):
    import mhm2_proxy_amd as m
    return m.KmerCounter(21, device=0, qual_offset=qoff)


def _assert_equal(cnt, ref, what):
    pb, po = ref
    gb, go = cnt.fastq_packed()
    assert len(go) == len(po) and (go == po).all(), f"{what}: offsets differ"
    bad = np.flatnonzero(gb != pb)
    if bad.size:  # name the first read that differs
        r = int(np.searchsorted(po, bad[0], side="right")) - 1
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first in read {r} at base {int(bad[0] - po[r])}: "
                             f"{int(gb[bad[0]])} != {int(pb[bad[0]])}")


def _run_valid(cnt, text: bytes, qoff: int, what: str):
    cnt.add_fastq(text)
    _assert_equal(cnt, _ref(text, qoff), what)


def _run_error(cnt, c):
    import mhm2_proxy_amd as m
    with pytest.raises(m.MhmkcError) as got:
        cnt.add_fastq(c.text)
    msg = str(got.value)
    code, says = MSG[c.error[0]]
    assert msg.startswith(code) and says in msg, (c.name, msg)
    assert int(re.search(r"record (\d+)", msg).group(1)) == c.error[1], (c.name, msg)


def _run_group(g: str):
    """every case of a group, one call each, through one counter per quality offset (a failed add_fastq leaves the
    handle as it was: mhmkc::fail only records the message, and the next call recomputes every buffer)"""
    for qoff in (33, 64):
        cs = [c for c in F.group(g) if c.qoff == qoff]
        if not cs:
            continue
        with _counter(qoff) as cnt:
            for c in cs:
                if c.valid:
                    _run_valid(cnt, c.text, qoff, c.name)
                else:
                    _run_error(cnt, c)


@pytest.mark.gpu
def test_gpu_a_first_character_of_next_line():
    """'@' and '+' after a newline on a lane, wave and chunk boundary (own bytes, wave_shl:1 DPP, memory), their twins
    with '#' and '-', the text's last byte on each boundary and the same without the final newline."""
    _run_group("a")


@pytest.mark.gpu
def test_gpu_b_trailing_whitespace():
    """Runs of 1..33 whitespace characters of all five kinds that end on and start around every boundary kind, on
    every line kind; whitespace-only lines; a last line without a newline that ends in whitespace."""
    _run_group("b")


@pytest.mark.gpu
def test_gpu_c_newline_density_and_sizes():
    _run_group("c")


@pytest.mark.gpu
def test_gpu_d_line_length_limit():
    _run_group("d")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["listed", "shuffled"])
@pytest.mark.parametrize("qoff", [33, 64])
def test_gpu_e_pack_alignment_cross(qoff, order):
    with _counter(qoff) as cnt:
        _run_valid(cnt, _batch("e", qoff, order), qoff, f"e {qoff} {order}")


@pytest.mark.gpu
def test_gpu_f_mixed_lengths_in_a_wave():
    with _counter() as cnt:
        for c in F.group("f"):
            _run_valid(cnt, c.text, 33, c.name)
        _run_valid(cnt, _batch("f", 33, "shuffled"), 33, "f shuffled")


@pytest.mark.gpu
def test_gpu_g_pack4_paths():
    """The full sweep runs: every byte value but '\\n' as a base (the refused ones one call each)."""
    for qoff in (33, 64):
        with _counter(qoff) as cnt:
            for order in ("listed", "shuffled"):
                _run_valid(cnt, _batch("g", qoff, order), qoff, f"g {qoff} {order}")
            if qoff == 33:
                for c in F.group("g", valid=False):
                    _run_error(cnt, c)


@pytest.mark.gpu
def test_gpu_h_read_names():
    with _counter() as cnt:
        for order in ("listed", "shuffled"):
            _run_valid(cnt, _batch("h", 33, order), 33, f"h {order}")
        for c in F.group("h", valid=False):
            _run_error(cnt, c)


@pytest.mark.gpu
def test_gpu_i_error_selection():
    _run_group("i")


def _device_texts():
    return [c for g in "abef" for c in F.group(g, valid=True) if c.qoff == 33]


@pytest.mark.gpu
def test_gpu_j_misaligned_device_text():
    """The valid texts of a, b, e and f as device texts that start 0, 1, 2, 3, 4, 8 and 15 bytes past a 16-byte
    boundary (every lane of nl_mask and load16 takes the byte loop, load4 every misalignment), with '\\n', '@' and 'A'
    in the 16 bytes after the text, which the contract lets the kernels read but not use."""
    import torch
    cs = _device_texts()
    with _counter() as cnt:
        for a in (0,) + MISALIGN:
            buf, at = bytearray(), []
            for c in cs:
                buf += b"\n" * (-len(buf) % 16 + a)
                at.append(len(buf))
                buf += c.text + TAIL
            big = torch.frombuffer(buf, dtype=torch.uint8).to("cuda:0")
            assert big.data_ptr() % 16 == 0
            for c, p in zip(cs, at):
                n = len(c.text)
                cnt.add_fastq_tensor(big[p:p + n + 16], n_bytes=n)
                _assert_equal(cnt, _ref(c.text), f"{c.name} at +{a}")


@pytest.mark.gpu
@pytest.mark.parametrize("block", [4096, 4099])
def test_gpu_k_block_file_reader(tmp_path, monkeypatch, block):
    """The texts of a, b and e back to back in one file, read in blocks: the line machinery in its `consumed` mode."""
    t = b"".join(c.text for g in "abe" for c in F.group(g, valid=True) if c.qoff == 33 and c.text.endswith(b"\n"))
    path = tmp_path / "cases.fq"
    path.write_bytes(t)
    monkeypatch.setenv("MHMKC_FQ_BLOCK", str(block))
    with _counter() as cnt:
        cnt.add_fastq_file(path)
        _assert_equal(cnt, _ref(t), f"file in blocks of {block}")
        assert cnt.stats()["fq_file_blocks"] >= len(t) // block
