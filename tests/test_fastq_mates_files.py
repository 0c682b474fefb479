"""Two mate files read in rounds (mhmkc_add_fastq_mates_files, mhmkc_add_fastq_named): blocks that cut the two files at
unrelated places, mates 2 trimmed to a third of mates 1 (the file with the shorter records must read less, not carry
more), a record longer than the block in one file, files that differ in their record counts, the errors with their
round and byte positions. Expected values: the oracle's merge of the text the alternating reader reads
(fastq_mates_cases.interleave_as_read) and the existing one-file call on it at one block."""
from __future__ import annotations

import functools
import re

import pytest

import common as c
import fastq_mates_cases as M

pytestmark = pytest.mark.gpu

BLOCKS = [4093, 7001, 1 << 28]


def pinned_bound(block: int) -> int:
    """include/mhmkc.h: two slots of block + 1 MiB + 64 bytes per file, with the allocator's slack."""
    return int(4.5 * (block + (1 << 20) + 64)) + 4096


def _write(tmp_path, name: str, text: bytes):
    p = tmp_path / name
    p.write_bytes(text)
    return p


@functools.lru_cache(maxsize=None)
def _trimmed(n_pairs: int):
    a, b = M.split_mates(c.paired_fastq_text(n_pairs, seed=91))
    return a, M.trim_mate2(b)


@pytest.mark.parametrize("k,block", [(21, 4093), (63, 7001), (21, 1 << 28)])
def test_trimmed_mates_over_many_rounds(tmp_path, monkeypatch, k, block):
    """Mate 2 at a third of mate 1's length: per round file 2 uses a third of the bytes file 1 uses. The carries stay
    within a block, the pinned memory under the documented bound, which does not depend on the files' sizes."""
    import mhm2_proxy_amd as m
    a, b = _trimmed(3000)
    assert len(b) < 0.55 * len(a)
    pa, pb_ = _write(tmp_path, "r1.fq", a), _write(tmp_path, "r2.fq", b)
    inter = _write(tmp_path, "inter.fq", M.interleave_as_read(a, b))
    monkeypatch.setenv("MHMKC_FQ_BLOCK", str(block))
    with m.KmerCounter(k, device=0) as cnt:
        cnt.add_fastq_mates_files(pa, pb_)
        info = cnt.fastq_mates_info()
        st = cnt.stats()
        assert st["fq_file_blocks"] == info["rounds"] and info["pairs"] == 3000
        M.assert_equals_oracle(cnt, a, b, k, what=f"block {block}")
        table = cnt.fetch()
    if block < len(a):
        assert info["rounds"] >= max(40, len(a) // block), info
        assert info["peak_carry_1"] <= block and info["peak_carry_2"] <= block, info
    else:
        assert info["rounds"] == 1
    assert info["block_bytes"] == block and info["bytes_read_1"] == len(a) and info["bytes_read_2"] == len(b)
    assert info["bytes_used_1"] == len(a) and info["bytes_used_2"] == len(b)
    assert 0 < info["pinned_bytes"] <= pinned_bound(block) == info["pinned_bound"], info
    # the interleaved one-file call, one block
    monkeypatch.setenv("MHMKC_FQ_BLOCK", str(1 << 28))
    with m.KmerCounter(k, device=0) as one:
        one.add_fastq_file(inter, pairs=True)
        one.finish()
        c.assert_tables_equal(table, one.fetch(), "mate files vs the interleaved file")


def test_pinned_bound_does_not_grow_with_the_files(tmp_path, monkeypatch):
    """Twice the pairs: twice the rounds, the same pinned bytes, the same bound on the carries."""
    import mhm2_proxy_amd as m
    block = 4093
    monkeypatch.setenv("MHMKC_FQ_BLOCK", str(block))
    infos = []
    for n in (1500, 3000):
        a, b = _trimmed(n)
        with m.KmerCounter(21, device=0) as cnt:
            cnt.add_fastq_mates_files(_write(tmp_path, f"a{n}.fq", a), _write(tmp_path, f"b{n}.fq", b))
            infos.append(cnt.fastq_mates_info())
            M.assert_equals_oracle(cnt, a, b, 21, table=False)
    small, big = infos
    assert big["rounds"] >= 1.8 * small["rounds"] >= 1.8 * 40
    assert small["pinned_bytes"] == big["pinned_bytes"] <= pinned_bound(block)
    assert max(big["peak_carry_1"], big["peak_carry_2"], small["peak_carry_1"], small["peak_carry_2"]) <= block


def test_pinned_bound_holds_after_a_call_with_a_larger_block(tmp_path, monkeypatch):
    """One handle, a block of 4 MiB and then one of 4093 bytes: the second call gives the larger slots back, so its
    pinned bytes are under its own bound."""
    import mhm2_proxy_amd as m
    a, b = _trimmed(1500)
    pa, pb_ = _write(tmp_path, "r1.fq", a), _write(tmp_path, "r2.fq", b)
    with m.KmerCounter(21, device=0) as cnt:
        held = []
        for block in (1 << 22, 4093, 1 << 22):
            monkeypatch.setenv("MHMKC_FQ_BLOCK", str(block))
            cnt.reset()
            cnt.add_fastq_mates_files(pa, pb_)
            info = cnt.fastq_mates_info()
            assert 0 < info["pinned_bytes"] <= pinned_bound(block) == info["pinned_bound"], info
            held.append(info["pinned_bytes"])
        assert held[1] < held[0] == held[2]
        M.assert_equals_oracle(cnt, a, b, 21)


@pytest.mark.parametrize("block", [2039, 4093])
def test_record_longer_than_the_block_in_a_only(tmp_path, monkeypatch, block):
    """File 1's records are longer than a block (mates of 2040 bases): its rounds take a block more until a record is
    whole, while file 2's short records wait."""
    import mhm2_proxy_amd as m
    a, b = M.split_mates(c.paired_fastq_text(60, seed=92, read_len=2040, frag_mean=3600, frag_sd=100, uneven=False))
    b = M.trim_mate2(b, 0.05)
    assert min(sum(len(ln) + 1 for ln in r) for r in M._records(a)[0]) > block and len(b) < 60 * 400
    monkeypatch.setenv("MHMKC_FQ_BLOCK", str(block))
    with m.KmerCounter(21, device=0) as cnt:
        cnt.add_fastq_mates_files(_write(tmp_path, "long1.fq", a), _write(tmp_path, "short2.fq", b))
        info = cnt.fastq_mates_info()
        pst = M.assert_equals_oracle(cnt, a, b, 21)
    assert pst["pairs"] == 60 and info["rounds"] > 60 and info["pinned_bytes"] <= pinned_bound(block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("short", [1, 2])
def test_one_file_shorter_by_three_records(tmp_path, monkeypatch, block, short):
    import mhm2_proxy_amd as m
    a, b = _trimmed(1500)
    if short == 1:
        a = M.drop_records(a, 3)
    else:
        b = M.drop_records(b, 3)
    monkeypatch.setenv("MHMKC_FQ_BLOCK", str(block))
    with m.KmerCounter(21, device=0) as cnt:
        cnt.add_fastq_mates_files(_write(tmp_path, "r1.fq", a), _write(tmp_path, "r2.fq", b))
        info = cnt.fastq_mates_info()
        pst = M.assert_equals_oracle(cnt, a, b, 21, table=block == 7001)
    assert pst["pairs"] == 1497 and info["unpaired_checked"] == (short == 2)
    if short == 2:  # A[1497] was read, the two records after it were not
        assert info["bytes_used_1"] == len(M.drop_records(a, 2)) and info["bytes_used_2"] == len(b)
    else:
        assert info["bytes_used_1"] == len(a) and info["bytes_used_2"] == len(M.drop_records(b, 3))


def _good_after(cnt, tmp_path, a, b):
    """After an error in a later round: finish refuses the partial round until reset; a good pair of files then gives
    the oracle's table."""
    import mhm2_proxy_amd as m
    with pytest.raises(m.MhmkcError) as e2:
        cnt.finish()
    assert str(e2.value).startswith("MHMKC_ESTATE"), str(e2.value)
    cnt.reset()
    cnt.add_fastq_mates_files(_write(tmp_path, "good1.fq", a), _write(tmp_path, "good2.fq", b))
    M.assert_equals_oracle(cnt, a, b, 21, what="after reset")


WHERE = r"FASTQ mate files round ([1-9]\d*), whose texts start at file 1 byte ([1-9]\d*) and file 2 byte ([1-9]\d*)"


def test_errors_in_a_later_round(tmp_path, monkeypatch):
    import mhm2_proxy_amd as m
    monkeypatch.setenv("MHMKC_FQ_BLOCK", "4093")
    a, b = _trimmed(1500)
    lb = b.split(b"\n")
    recs_b = [b"\n".join(lb[4 * i:4 * i + 4]) + b"\n" for i in range(1500)]
    la = a.split(b"\n")
    offs_a, offs_b = [0], [0]
    for i in range(1500):
        offs_a.append(offs_a[-1] + sum(len(ln) + 1 for ln in la[4 * i:4 * i + 4]))
        offs_b.append(offs_b[-1] + len(recs_b[i]))

    def located(msg, what, rec):
        """The record named in the message, counted from the round's text, is record `rec` of the file."""
        w = re.search(WHERE, msg)
        assert w, msg
        r = re.search(what + r" (\d+)", msg)
        assert r, msg
        start = {1: offs_a, 2: offs_b}
        first = start[2].index(int(w.group(3))) if "file 2" in what or "pair" in what else start[1].index(int(w.group(2)))
        assert first + int(r.group(1)) == rec, msg
        if "pair" in what:  # both texts start at the same record
            assert start[1].index(int(w.group(2))) == first, msg

    with m.KmerCounter(21, device=0) as cnt:
        # B without its record 900: pair 900 has different names
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates_files(_write(tmp_path, "r1.fq", a), _write(tmp_path, "del2.fq", b"".join(recs_b[:900] + recs_b[901:])))
        msg = str(e.value)
        assert msg.startswith("MHMKC_EINVAL") and "mismatched pair names" in msg, msg
        located(msg, "FASTQ pair", 900)
        _good_after(cnt, tmp_path, a, b)
    with m.KmerCounter(21, device=0) as cnt:
        # an illegal base in B's record 1200
        bad = list(lb)
        bad[4 * 1200 + 1] = b"X" + bad[4 * 1200 + 1][1:]
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates_files(_write(tmp_path, "r1.fq", a), _write(tmp_path, "bad2.fq", b"\n".join(bad)))
        msg = str(e.value)
        assert msg.startswith("MHMKC_EBADCHAR"), msg
        located(msg, "file 2 record", 1200)
        _good_after(cnt, tmp_path, a, b)
    with m.KmerCounter(21, device=0) as cnt:
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates_files(_write(tmp_path, "r1.fq", a), tmp_path / "missing2.fq")
        assert str(e.value).startswith("MHMKC_EINVAL") and "file 2" in str(e.value), str(e.value)
        cnt.add_fastq_mates_files(_write(tmp_path, "r1.fq", a), _write(tmp_path, "r2.fq", b))  # nothing was added
        M.assert_equals_oracle(cnt, a, b, 21, what="after a missing file")


@pytest.mark.parametrize("fail_round", [1, 3])
def test_read_failure_in_a_later_round(tmp_path, monkeypatch, knob, fail_round):
    import mhm2_proxy_amd as m
    monkeypatch.setenv("MHMKC_FQ_BLOCK", "7001")
    a, b = _trimmed(1500)
    pa, pb_ = _write(tmp_path, "r1.fq", a), _write(tmp_path, "r2.fq", b)
    knob("fq_read_fail", fail_round)
    try:
        with m.KmerCounter(21, device=0) as cnt:
            with pytest.raises(m.MhmkcError) as e:
                cnt.add_fastq_mates_files(pa, pb_)
            assert str(e.value).startswith("MHMKC_EINVAL") and "read error" in str(e.value), str(e.value)
            knob("fq_read_fail", -1)
            _good_after(cnt, tmp_path, a, b)
    finally:
        knob("fq_read_fail", -1)


def test_named_call_takes_the_three_forms(tmp_path, monkeypatch):
    """"a:b", "a:" and "a" give what mhmkc_add_fastq_mates_files, mhmkc_add_fastq_file and mhmkc_add_fastq_pairs_file give."""
    import mhm2_proxy_amd as m
    monkeypatch.setenv("MHMKC_FQ_BLOCK", "7001")
    a, b = _trimmed(1500)
    pa, pb_ = _write(tmp_path, "r1.fq", a), _write(tmp_path, "r2.fq", b)
    inter = _write(tmp_path, "inter.fq", M.interleave_as_read(a, b))
    calls = [(f"{pa}:{pb_}", lambda cnt: cnt.add_fastq_mates_files(pa, pb_)),
             (f"{pa}:", lambda cnt: cnt.add_fastq_file(pa)),
             (f"{inter}", lambda cnt: cnt.add_fastq_file(inter, pairs=True))]
    for name, direct in calls:
        assert m.split_reads_fname(name)[1] == name.split(":")[0]
        with m.KmerCounter(21, device=0) as named, m.KmerCounter(21, device=0) as plain:
            named.add_fastq_named(name)
            direct(plain)
            (b1, o1), (b2, o2) = named.fastq_packed(), plain.fastq_packed()
            assert (o1 == o2).all() and (b1 == b2).all(), name
            s1, s2 = named.stats(), plain.stats()
            for key in ("fq_pairs", "fq_merged", "fq_ambiguous", "fq_overlap_bases", "reads", "bases", "fq_file_blocks"):
                assert s1[key] == s2[key], (name, key)
            named.finish()
            plain.finish()
            c.assert_tables_equal(named.fetch(), plain.fetch(), name)
    with m.KmerCounter(21, device=0) as cnt:
        for bad in (f":{pb_}", ":", ""):
            with pytest.raises(m.MhmkcError) as e:
                cnt.add_fastq_named(bad)
            assert str(e.value).startswith("MHMKC_EINVAL"), str(e.value)
