"""CPU: the two-mate-texts rule (fastq_mates_cases.interleave_as_read) held to the merge restatements, the reads file
name split, and the new entry points in the header, the library and the info struct."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest

import common as c
import fastq_mates_cases as M
import oracle_lib as O
import ref_merge_literal as R

ROOT = Path(__file__).resolve().parents[1]
CALLS = ["mhmkc_add_fastq_mates", "mhmkc_add_fastq_mates_device", "mhmkc_add_fastq_mates_files", "mhmkc_add_fastq_named",
         "mhmkc_fastq_mates_info"]
N_PAIRS, SEED = 40, 71


def test_split_and_interleave_round_trip():
    t = c.paired_fastq_text(N_PAIRS, seed=SEED)
    a, b = M.split_mates(t)
    assert a.count(b"\n") == b.count(b"\n") == 4 * N_PAIRS and M.interleave_as_read(a, b) == t


@pytest.mark.parametrize("name", sorted(M.skew_cases(N_PAIRS, SEED)))
def test_interleave_as_read_against_the_merge_restatements(name):
    """The text read is the first P pairs of the original interleaving (+ an unpaired A[P], + a cut record whose turn
    came): both restatements of merge_reads give, on it, the merge of those P pairs; the cut record is where the C
    restatement stops (the reference's reader fails at that read)."""
    t = c.paired_fastq_text(N_PAIRS, seed=SEED)
    a, b, pairs, err = M.skew_cases(N_PAIRS, SEED)[name]
    read = M.interleave_as_read(a, b)
    head = b"".join(ln + b"\n" for ln in t.split(b"\n")[:8 * pairs])  # the first P pairs, from the original
    assert read.startswith(head)
    rest = read[len(head):].split(b"\n")[:-1]
    eb, eo, est = R.merge_fastq(head)
    assert est["pairs"] == pairs
    gb, go, gst = R.merge_fastq(read)  # (it reads complete records only)
    assert (gb, go, gst) == (eb, eo, est)
    if err is None:
        assert len(rest) in (0, 4)  # nothing, or the unpaired A[P]
        assert (len(rest) == 4) == (name in ("a_longer_by_3", "empty_b", "cut_a_turn_does_not_come"))
        ob, oo, ost = O.merge_fastq(read)
        assert ost == est and list(oo) == eo and ob.tobytes() == eb
    else:
        assert len(rest) % 4 == 2 and len(rest) // 4 == err[1] - 2 * pairs
        with pytest.raises(O.FastqError) as e:
            O.merge_fastq(read)
        assert (e.value.kind, e.value.record) == err


def test_split_reads_fname():
    import mhm2_proxy_amd as m
    assert m.split_reads_fname("a:b") == ("mates", "a", "b")
    assert m.split_reads_fname("a:") == ("single", "a", None)
    assert m.split_reads_fname("a") == ("interleaved", "a", None)
    assert m.split_reads_fname("/d/r1.fq:/d/x:y.fq") == ("mates", "/d/r1.fq", "/d/x:y.fq")  # the first colon splits
    for bad in (":b", ":", ""):
        with pytest.raises(ValueError):
            m.split_reads_fname(bad)


def test_header_exports_the_calls_and_keeps_abi_14():
    from mhm2_proxy_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mhmkc.h").read_text(), flags=re.S)
    for name in CALLS:
        assert re.search(rf"\bint {name}\s*\(", text) and name in N.ABI_SYMBOLS, name
    assert re.search(r"#define\s+MHMKC_ABI_VERSION\s+14\b", text)


def test_library_exports_the_calls():
    from mhm2_proxy_amd import _native as N
    L = N.lib()
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.mhmkc_abi_version() == 14


def test_info_struct_has_only_8_byte_fields(tmp_path):
    """Python's mirror field by field, and the header's struct through the C compiler."""
    import shutil
    import subprocess

    from mhm2_proxy_amd import _native as N
    fields = N.MhmkcFastqMatesInfo._fields_
    assert all(t in (C.c_uint64, C.c_double) for _, t in fields)
    assert C.sizeof(N.MhmkcFastqMatesInfo) == 8 * len(fields)
    for want in ("pairs", "rounds", "bytes_read_1", "bytes_read_2", "bytes_used_1", "bytes_used_2", "peak_carry_1",
                 "peak_carry_2", "pinned_bytes", "unpaired_checked"):
        assert want in dict(fields), want
    if not shutil.which("gcc"):
        pytest.skip("gcc missing: the header's struct was not checked through the C compiler (Python's mirror was)")
    lines = "".join(f'printf("%zu %zu\\n", offsetof(mhmkc_fastq_mates_info_t, {f}), sizeof(((mhmkc_fastq_mates_info_t *)0)->{f}));'
                    for f, _ in fields)
    src = tmp_path / "info.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmkc.h"\nint main(void){' + lines +
                   'printf("%zu\\n", sizeof(mhmkc_fastq_mates_info_t));return 0;}\n')
    exe = tmp_path / "info"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert [ln.split() for ln in out[:-1]] == [[str(8 * i), "8"] for i in range(len(fields))]
    assert int(out[-1]) == 8 * len(fields)
