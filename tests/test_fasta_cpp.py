"""print_stats / dump_contigs of the C++ adapter (include/mhmkc_kcount.hpp): the device path (HashTableInserter::uutigs_stats,
dump_uutigs) against the plain host loops over the Contigs vector (ctg_stats, print_stats, dump_contigs):
tests/cpp/fasta_test.cpp. The host loops are also held to the Python reference of fasta_cases.py."""
import shutil
import subprocess
from pathlib import Path

import pytest

import fasta_cases as F
import mhm2_proxy_amd as m
from common import synth_set

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "fasta_test.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory) -> Path:
    """tests/cpp/fasta_test.cpp, compiled once for the module."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    from mhm2_proxy_amd import build as b

    b.build_lib()
    exe = tmp_path_factory.mktemp("fasta_cpp") / "fasta_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC),
                    f"-L{ROOT / 'mhm2_proxy_amd'}", "-lmhmkc", "-lz", f"-Wl,-rpath,{ROOT / 'mhm2_proxy_amd'}",
                    "-o", str(exe)], check=True)
    return exe


def test_adapter_calls_compile_for_every_max_k(exe):
    """CPU: uutigs_stats, dump_uutigs and the host loops instantiate for MAX_K = 32, 64, 96 and 128."""
    assert subprocess.run([str(exe)], env={"MHMKC_NO_TORCH": "1"}).returncode == 2  # usage: no GPU touched


@pytest.mark.gpu
@pytest.mark.parametrize("k,min_len", [(21, 0), (21, 45), (63, 0)])
def test_device_path_equals_the_host_loops(exe, k, min_len, tmp_path):
    b, o = synth_set(1500, 10000, 7)
    pr = m.PackedReads.from_arrays(b, o)
    reads = tmp_path / "reads.txt"
    with open(reads, "w") as f:
        for i in range(pr.get_local_num_reads()):
            _, s, q = pr.get_read(i)
            f.write(f"{s} {q}\n")
    out = subprocess.run([str(exe), str(k), str(reads), str(min_len), str(tmp_path)], capture_output=True, text=True,
                         cwd=tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    head, block = out.stdout.split("\n", 1)
    words = head.split()
    text = (tmp_path / "host.fasta").read_bytes()
    assert words[0] == "OK" and int(words[1]) > 5 and int(words[2]) == len(text) > 500
    # the host loops against the Python reference: the file parsed back gives the contigs, which give the file and the block
    recs = text.split(b"\n")[:-1]
    ids = [int(h.split()[0][7:]) for h in recs[0::2]]
    seqs, depths = tuple(recs[1::2]), tuple(float(h.split()[1]) for h in recs[0::2])
    assert all(len(s) >= min_len for s in seqs) and ids == sorted(ids) and int(words[1]) == len(seqs)
    if min_len == 0:
        assert ids == list(range(len(ids)))
    st = F.stats_ref(seqs, depths, min_len)
    lines, ref = block.splitlines(), F.stats_text_ref(st, min_len).splitlines()
    assert lines[:3] == ref[:3] and lines[4:] == ref[4:]  # (the depths in the file have six decimals: line 3 apart)
    assert lines[3].startswith("    Average contig depth:    ")
    assert abs(float(lines[3].split()[-1]) - st["tot_depth"] / st["n_ctgs"]) < 1e-3
