"""Read pairs from two mate texts on the device (mhmkc_add_fastq_mates, mhmkc_add_fastq_mates_device; fastq.hip
k_fq_mate_records): host texts and device tensors against the oracle's merge of the text the alternating reader
reads (fastq_mates_cases.interleave_as_read) and against the existing one-text call on it. Compared: the PackedReads
bytes and offsets, the four pair statistics, reads and bases, the sorted table."""
from __future__ import annotations

import functools
import re

import numpy as np
import pytest

import common as c
import fastq_mates_cases as M
import oracle_lib as O

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _mates(n_pairs: int = 3001, seed: int = 81):
    return M.split_mates(c.paired_fastq_text(n_pairs, seed=seed))


def _head(text: bytes, n_records: int) -> bytes:
    return M.drop_records(text, text.count(b"\n") // 4 - n_records)


@pytest.mark.parametrize("k", [21, 63])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 3000])
def test_texts_at_the_record_kernel_grid_edges(P, k):
    """P pairs with and without an unpaired A[P]: P + 1 lanes over blocks of 256, the last lane the scan's end or the
    unpaired record's check."""
    import mhm2_proxy_amd as m
    a, b = _mates()
    for extra in (0, 1):
        ta, tb = _head(a, P + extra), _head(b, P)
        with m.KmerCounter(k, device=0) as cnt:
            cnt.add_fastq_mates(ta, tb)
            info = cnt.fastq_mates_info()
            pst = M.assert_equals_oracle(cnt, ta, tb, k, table=P > 0 and (extra == 0 or P == 257), what=f"P={P} extra={extra}")
        assert pst["pairs"] == P and info["pairs"] == P and info["rounds"] == 1
        assert info["unpaired_checked"] == extra
        assert info["bytes_used_1"] == len(ta) and info["bytes_used_2"] == len(tb)


def test_texts_equal_the_one_text_call():
    """The existing interleaved entry point on the text read, item by item."""
    import mhm2_proxy_amd as m
    a, b = _mates()
    ta, tb = _head(a, 1200), _head(b, 1197)
    with m.KmerCounter(21, device=0) as one, m.KmerCounter(21, device=0) as two:
        one.add_fastq_pairs(M.interleave_as_read(ta, tb))
        two.add_fastq_mates(ta, tb)
        (b1, o1), (b2, o2) = one.fastq_packed(), two.fastq_packed()
        s1, s2 = one.stats(), two.stats()
        assert (o1 == o2).all() and (b1 == b2).all()
        for key in ("fq_pairs", "fq_merged", "fq_ambiguous", "fq_overlap_bases", "reads", "bases"):
            assert s1[key] == s2[key], key
        one.finish()
        two.finish()
        c.assert_tables_equal(one.fetch(), two.fetch(), "mates vs interleaved")


def test_long_mates_take_the_long_pair_instance():
    """A handful of pairs with mates above 504 bases among short ones: the long-pair list is filled by the record pass."""
    import mhm2_proxy_amd as m
    t = b"".join([c.paired_fastq_text(600, seed=82),
                  c.paired_fastq_text(6, seed=83, read_len=506, frag_mean=800, frag_sd=120),
                  c.paired_fastq_text(5, seed=84, read_len=900, frag_mean=1500, frag_sd=300),
                  c.paired_fastq_text(400, seed=85)])
    a, b = M.split_mates(t)
    with m.KmerCounter(21, device=0) as cnt:
        cnt.add_fastq_mates(a, b)
        pst = M.assert_equals_oracle(cnt, a, b, 21)
    assert pst["pairs"] == 1011 and pst["merged"] > 0


def test_crlf_in_b_only_and_no_final_newline_in_a_only():
    import mhm2_proxy_amd as m
    a, b = _mates()
    ta, tb = _head(a, 700)[:-1], _head(b, 700).replace(b"\n", b"\r\n")
    assert not ta.endswith(b"\n") and tb.count(b"\r\n") == 2800
    with m.KmerCounter(21, device=0) as cnt:
        cnt.add_fastq_mates(ta, tb)
        M.assert_equals_oracle(cnt, ta, tb, 21)


@pytest.mark.parametrize("name", sorted(M.skew_cases(8, 1)))
def test_count_skews_and_truncations(name):
    import mhm2_proxy_amd as m
    a, b, pairs, err = M.skew_cases(300, 86)[name]
    with m.KmerCounter(21, device=0) as cnt:
        if err is None:
            cnt.add_fastq_mates(a, b)
            pst = M.assert_equals_oracle(cnt, a, b, 21, what=name)
            assert pst["pairs"] == pairs
            assert cnt.fastq_mates_info()["unpaired_checked"] == (a.count(b"\n") // 4 > pairs)
            return
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates(a, b)
        with pytest.raises(O.FastqError) as oe:
            O.merge_fastq(M.interleave_as_read(a, b))
        assert (oe.value.kind, oe.value.record) == err
        assert str(e.value).startswith("MHMKC_EINVAL"), str(e.value)
        assert f"file {1 + err[1] % 2} ends inside record {err[1] // 2}" in str(e.value), str(e.value)
        # the one-text call fails the same way on the text read
        with pytest.raises(m.MhmkcError) as e1:
            cnt.add_fastq_pairs(M.interleave_as_read(a, b))
        assert str(e1.value).startswith("MHMKC_EINVAL") and f"ends inside record {err[1]}" in str(e1.value)


def test_unpaired_record_is_checked_and_the_rest_is_not():
    """A[P] is read before B runs out, so its faults are found; records after the stop are never looked at."""
    import mhm2_proxy_amd as m
    a, b = _mates()
    ta, tb = _head(a, 304), _head(b, 300)
    la = ta.split(b"\n")
    bad_read = list(la)
    bad_read[4 * 300 + 2] = b"-"          # A[300]: no '+'
    bad_unread = list(la)
    bad_unread[4 * 301 + 2] = b"-"        # A[301]: never read
    with m.KmerCounter(21, device=0) as cnt:
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates(b"\n".join(bad_read), tb)
        assert str(e.value).startswith("MHMKC_EINVAL") and "file 1 record 300: expected '+'" in str(e.value), str(e.value)
        cnt.reset()
        cnt.add_fastq_mates(b"\n".join(bad_unread), tb)
        M.assert_equals_oracle(cnt, ta, tb, 21)
    lb = _head(b, 304).split(b"\n")
    lb[4 * 300] = b"no at sign"            # B[300] with A ending at 300 records: never read
    with m.KmerCounter(21, device=0) as cnt:
        cnt.add_fastq_mates(_head(a, 300), b"\n".join(lb))
        M.assert_equals_oracle(cnt, _head(a, 300), tb, 21)


def test_text_errors_name_the_file_the_record_and_the_pair():
    import mhm2_proxy_amd as m
    a, b = _mates()
    ta, tb = _head(a, 600), _head(b, 600)
    lb = tb.split(b"\n")
    deleted = b"\n".join(lb[:4 * 411] + lb[4 * 412:])  # B without its record 411: pair 411's names differ
    bad_base = list(lb)
    bad_base[4 * 520 + 1] = b"X" + bad_base[4 * 520 + 1][1:]
    la = ta.split(b"\n")
    bad_a = list(la)
    bad_a[4 * 77 + 1] = b"X" + bad_a[4 * 77 + 1][1:]
    with m.KmerCounter(21, device=0) as cnt:
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates(ta, deleted)
        assert str(e.value).startswith("MHMKC_EINVAL") and "mismatched pair names" in str(e.value), str(e.value)
        assert re.search(r"pair 411 \(file 1 record 411, file 2 record 411\)", str(e.value)), str(e.value)
        cnt.reset()
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates(ta, b"\n".join(bad_base))
        assert str(e.value).startswith("MHMKC_EBADCHAR") and "file 2 record 520" in str(e.value), str(e.value)
        cnt.reset()
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates(b"\n".join(bad_a), tb)
        assert str(e.value).startswith("MHMKC_EBADCHAR") and "file 1 record 77" in str(e.value), str(e.value)
        cnt.reset()
        with pytest.raises(m.MhmkcError) as e:
            cnt.add_fastq_mates(tb, ta)  # the mates /2 given as text 1
        assert str(e.value).startswith("MHMKC_EINVAL") and "pair numbers" in str(e.value), str(e.value)
        cnt.reset()
        cnt.add_fastq_mates(ta, tb)  # a good call after the errors
        M.assert_equals_oracle(cnt, ta, tb, 21)
        with pytest.raises(m.MhmkcError) as e:  # finished: MHMKC_ESTATE until reset
            cnt.add_fastq_mates(ta, tb)
        assert str(e.value).startswith("MHMKC_ESTATE"), str(e.value)


@pytest.mark.parametrize("layout", ["b_above_a", "b_below_a", "separate", "separate_unpadded", "odd_addresses"])
def test_tensors_anywhere_in_memory(layout):
    """Device texts at any two addresses: two views of one padded buffer in both orders (B above A, B below A), two
    tensors of their own, tensors without padding (the adapter pads them), and views at odd byte addresses."""
    import torch

    import mhm2_proxy_amd as m
    a, b = _mates()
    ta, tb = _head(a, 900), _head(b, 897)
    na, nb = len(ta), len(tb)
    dev = torch.device("cuda", 0)

    def put(buf, at, text):
        buf[at:at + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy())

    with m.KmerCounter(21, device=0) as cnt:
        if layout in ("b_above_a", "b_below_a", "odd_addresses"):
            first, second = (ta, tb) if layout != "b_below_a" else (tb, ta)
            o1 = 3 if layout == "odd_addresses" else 0
            o2 = o1 + (len(first) + 16 + 255) // 256 * 256 + (6 if layout == "odd_addresses" else 0)
            host = torch.zeros(o2 + len(second) + 16, dtype=torch.uint8)
            put(host, o1, first)
            put(host, o2, second)
            buf = host.to(dev)
            v1, v2 = buf[o1:o1 + len(first) + 4], buf[o2:o2 + len(second) + 4]
            va, vb = (v1, v2) if layout != "b_below_a" else (v2, v1)
            assert (vb.data_ptr() > va.data_ptr()) == (layout != "b_below_a")
            cnt.add_fastq_mates_tensors(va, vb, na, nb)
        elif layout == "separate":
            da, db = torch.zeros(na + 16, dtype=torch.uint8), torch.zeros(nb + 16, dtype=torch.uint8)
            put(da, 0, ta)
            put(db, 0, tb)
            cnt.add_fastq_mates_tensors(da.to(dev), db.to(dev), na, nb)
        else:
            cnt.add_fastq_mates_tensors(torch.from_numpy(np.frombuffer(ta, dtype=np.uint8).copy()).to(dev),
                                        torch.from_numpy(np.frombuffer(tb, dtype=np.uint8).copy()).to(dev))
        assert cnt.fastq_mates_info()["unpaired_checked"] == 1
        M.assert_equals_oracle(cnt, ta, tb, 21, what=layout)
