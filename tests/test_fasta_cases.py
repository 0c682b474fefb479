"""CPU checks of the reference and the inputs of the FASTA / assembly statistics tests (fasta_cases.py), of
assembly_stats_text, and of the C ABI's declarations and their Python mirror. No GPU."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np

import fasta_cases as F
from mhm2_proxy_amd import _native as N
from mhm2_proxy_amd import assembly_stats_text
from mhm2_proxy_amd.kcount import perc_str

ROOT = Path(__file__).resolve().parents[1]
NEW_CALLS = ["mhmkc_ctgs_stats_device", "mhmkc_uutigs_stats", "mhmkc_ctgs_fasta_device", "mhmkc_uutigs_fasta",
             "mhmkc_fasta_device", "mhmkc_fasta_fetch", "mhmkc_fasta_write", "mhmkc_fasta_info"]


def test_integer_scheme_equals_percent_f_on_the_depth_values():
    for d in F.depth_values():
        assert F.fmt_int(d) == "%f" % d, repr(d)


def test_integer_scheme_equals_percent_f_on_random_doubles():
    """200k doubles with every exponent below 2^32 (random bit patterns below 2^32's), subnormals included."""
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 0x41F0000000000000, 199000, dtype=np.uint64)
    sub = rng.integers(0, 1 << 52, 1000, dtype=np.uint64)  # subnormals
    for d in np.concatenate([bits, sub]).view(np.float64).tolist():
        assert F.fmt_int(d) == "%f" % d, repr(d)


def test_builders_hold_their_edges():
    """Every builder asserts its own edges; here: the cases exist, are the same on a second call, and the whole set holds
    the shapes the GPU tests rely on."""
    cases = F.all_cases()
    assert F.all_cases() is cases
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        bases, offsets, depths = F.arrays(c)
        assert offsets[0] == 0 and int(offsets[-1]) == len(bases) and len(depths) == len(c.seqs)
        assert c.first_id + len(c.seqs) <= F.ID_MAX
    lc = F.lengths_case()
    starts = F.seq_starts(lc.seqs, lc.depths, lc.first_id, 0)
    assert len({(s % 16, d % 16) for s, d, n in starts if n >= 48}) == 256
    assert F.stats_ref(lc.seqs, lc.depths, max(lc.min_lens))["n_ctgs"] == 0  # above the maximum: nothing is counted
    assert F.fasta_ref(lc.seqs, lc.depths, 0, max(lc.min_lens)) == b""
    for mn in (499, 500, 501):  # the filter's edge on both sides
        assert F.stats_ref(lc.seqs, lc.depths, mn)["n_ctgs"] != F.stats_ref(lc.seqs, lc.depths, mn + 1)["n_ctgs"]
    fc = F.filter_case()
    assert F.fasta_ref(fc.seqs, fc.depths, fc.first_id, 30).count(b">") == sum(len(s) >= 30 for s in fc.seqs)
    assert F.fasta_ref(fc.seqs, fc.depths, fc.first_id, 30).startswith(b">Contig1001 ")  # the unfiltered index
    # header lengths of the depths case change with the rounding's carry
    assert "%f" % 9.9999995 in ("10.000000", "9.999999")
    assert F.stats_ref((), (), 0) == {"n_ctgs": 0, "tot_len": 0, "max_len": 0, "n_ns": 0, "tot_depth": 0.0,
                                       "len_sums": [0] * 5, "n50": 0, "l50": 0}


def test_fasta_ref_format():
    assert F.fasta_ref((b"ACGT", b"", b"NN"), (2.5, 1.0, 0.0000005), 9, 0) == \
        b">Contig9 2.500000\nACGT\n>Contig10 1.000000\n\n>Contig11 0.000000\nNN\n"
    assert F.fasta_ref((b"ACGT", b"", b"NN"), (2.5, 1.0, 0.0000015), 9, 2) == b">Contig9 2.500000\nACGT\n>Contig11 0.000002\nNN\n"


STATS_A = {"n_ctgs": 3, "tot_len": 61500, "max_len": 50000, "n_ns": 4, "tot_depth": 37.5,
           "len_sums": [61000, 60000, 60000, 50000, 50000], "n50": 50000, "l50": 1}
# written out by hand from the SLOG lines of src/contigs.cpp:151-163 (perc_str: upcxx-utils/src/log.cpp:428-434)
TEXT_A = ("Assembly statistics (contig lengths >= 500)\n"
          "    Number of contigs:       3\n"
          "    Total assembled length:  61500\n"
          "    Average contig depth:    12.5\n"
          "    Number of Ns/100kbp:     6.50407 (4)\n"
          "    Max. contig length:      50000\n"
          "    Contig lengths:\n"
          "        > 1kbp:              61000 (99.19%)\n"
          "        > 5kbp:              60000 (97.56%)\n"
          "        > 10kbp:             60000 (97.56%)\n"
          "        > 25kbp:             50000 (81.30%)\n"
          "        > 50kbp:             50000 (81.30%)\n")
STATS_B = {"n_ctgs": 0, "tot_len": 0, "max_len": 0, "n_ns": 0, "tot_depth": 0.0, "len_sums": [0] * 5, "n50": 0, "l50": 0}
TEXT_B = ("Assembly statistics (contig lengths >= 0)\n"
          "    Number of contigs:       0\n"
          "    Total assembled length:  0\n"
          "    Average contig depth:    -nan\n"
          "    Number of Ns/100kbp:     -nan (0)\n"
          "    Max. contig length:      0\n"
          "    Contig lengths:\n"
          "        > 1kbp:              0 (0.00%)\n"
          "        > 5kbp:              0 (0.00%)\n"
          "        > 10kbp:             0 (0.00%)\n"
          "        > 25kbp:             0 (0.00%)\n"
          "        > 50kbp:             0 (0.00%)\n")


def test_assembly_stats_text_line_for_line():
    assert assembly_stats_text(STATS_A, 500) == TEXT_A
    assert assembly_stats_text(STATS_B, 0) == TEXT_B
    assert F.stats_text_ref(STATS_A, 500) == TEXT_A and F.stats_text_ref(STATS_B, 0) == TEXT_B
    assert perc_str(1, 3) == "1 (33.33%)" and perc_str(0, 0) == "0 (0.00%)" and perc_str(2, 3) == "2 (66.67%)"
    big = dict(STATS_A, tot_len=123456789012, tot_depth=1234567.0 * 3)  # %g: six significant digits, exponent form
    assert "    Average contig depth:    1.23457e+06\n" in assembly_stats_text(big, 0)
    for c in F.all_cases():
        for mn in c.min_lens:
            st = F.stats_ref(c.seqs, c.depths, mn)
            assert assembly_stats_text(st, mn) == F.stats_text_ref(st, mn)


def _struct_fields(text: str, name: str) -> int:
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for item in decl.split(","):
            m = re.search(r"\[(\d+)\]", item)
            n += int(m.group(1)) if m else 1
    return n


def test_header_declares_the_calls_and_native_mirrors_them():
    text = (ROOT / "include" / "mhmkc.h").read_text()
    for sym in NEW_CALLS:
        assert re.search(r"\bint " + sym + r"\(mhmkc_t h", text), sym
        assert sym in N.ABI_SYMBOLS
    assert re.search(r"#define MHMKC_ABI_VERSION 14\b", text)
    assert "MHMKC_EIO = -9" in text and N.ERRORS[-9] == "MHMKC_EIO"
    # the structs: every field is 8 bytes
    assert C.sizeof(N.MhmkcCtgStats) == 8 * _struct_fields(text, "mhmkc_ctg_stats") == 96
    assert C.sizeof(N.MhmkcFastaInfo) == 8 * _struct_fields(text, "mhmkc_fasta_info_t") == 104
    assert [f for f, _ in N.MhmkcCtgStats._fields_] == ["n_ctgs", "tot_len", "max_len", "n_ns", "tot_depth", "len_sums",
                                                         "n50", "l50"]
    assert "fasta_chunk_bytes" in (ROOT / "include" / "mhmkc_debug.h").read_text()


def test_library_exports_the_calls_and_keeps_its_abi_version():
    L = N.lib()
    assert L.mhmkc_abi_version() == 14
    for sym in NEW_CALLS:
        assert hasattr(L, sym), sym
    # no handle: a clean refusal, no GPU touched
    assert L.mhmkc_ctgs_stats_device(None, None, None, None, 0, 0, None, None) == -1
    assert L.mhmkc_uutigs_stats(None, 0, None, None) == -1
    assert L.mhmkc_ctgs_fasta_device(None, None, None, None, 0, 0, 0, None, None, None) == -1
    assert L.mhmkc_uutigs_fasta(None, 0, None, None, None) == -1
    assert L.mhmkc_fasta_device(None, None, None) == -1 and L.mhmkc_fasta_fetch(None, None) == -1
    assert L.mhmkc_fasta_write(None, b"x") == -1 and L.mhmkc_fasta_info(None, None) == -1
    assert L.mhmkc_debug_set(b"fasta_chunk_bytes", 63) == -1 and L.mhmkc_debug_set(b"fasta_chunk_bytes", 64) == 0
    N.debug_reset()
