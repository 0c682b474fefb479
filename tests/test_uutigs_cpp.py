"""The device traversal of the C++ adapter (include/mhmkc_dbjg.hpp traverse_debruijn_graph_device over
HashTableInserter::uutigs / mhmkc_uutigs) against the host one over the adapter's KmerMap: tests/cpp/uutig_test.cpp."""
import shutil
import subprocess
from pathlib import Path

import pytest

import mhm2_proxy_amd as m
from common import synth_set

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "uutig_test.cpp"


def build(tmp: Path) -> Path:
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    from mhm2_proxy_amd import build as b

    b.build_lib()
    exe = tmp / "uutig_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC),
                    f"-L{ROOT / 'mhm2_proxy_amd'}", "-lmhmkc", "-lz", f"-Wl,-rpath,{ROOT / 'mhm2_proxy_amd'}",
                    "-o", str(exe)], check=True)
    return exe


def test_device_traversal_compiles_for_every_max_k(tmp_path):
    """CPU: HashTableInserter::uutigs and traverse_debruijn_graph_device instantiate for MAX_K = 32, 64, 96 and 128."""
    exe = build(tmp_path)
    assert subprocess.run([str(exe)], env={"MHMKC_NO_TORCH": "1"}).returncode == 2  # usage: no GPU touched


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_device_traversal_equals_the_host_traversal(k, tmp_path):
    exe = build(tmp_path)
    b, o = synth_set(1500, 10000, 7)
    pr = m.PackedReads.from_arrays(b, o)
    reads = tmp_path / "reads.txt"
    with open(reads, "w") as f:
        for i in range(pr.get_local_num_reads()):
            _, s, q = pr.get_read(i)
            f.write(f"{s} {q}\n")
    out = subprocess.run([str(exe), str(k), str(reads)], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    words = out.stdout.split()
    assert words[0] == "OK" and int(words[1]) > 5 and int(words[2]) > 5000
