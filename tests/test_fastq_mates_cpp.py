"""The C++ adapter's read-library call (include/mhmkc_kcount.hpp: HashTableInserter::add_reads_fname, the KmerDHT forward):
tests/cpp/fastq_mates_test.cpp names two mate files as main.cpp does ("r1.fq:r2.fq"), finishes, and prints a digest of
its KmerMap, which must be the digest of the Python adapter's table for the same files."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import common as c
import fastq_mates_cases as M

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "fastq_mates_test.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory) -> Path:
    """tests/cpp/fastq_mates_test.cpp, compiled once for the module."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    from mhm2_proxy_amd import build as b

    b.build_lib()
    exe = tmp_path_factory.mktemp("fastq_mates_cpp") / "fastq_mates_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC),
                    f"-L{ROOT / 'mhm2_proxy_amd'}", "-lmhmkc", "-lz", "-lpthread", f"-Wl,-rpath,{ROOT / 'mhm2_proxy_amd'}",
                    "-o", str(exe)], check=True)
    return exe


def table_digest(t) -> tuple:
    """row_mix of fastq_mates_test.cpp summed over the rows, with the row count and the sum of the counts."""
    M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.asarray(t.keys, dtype=np.uint64)
    h = np.zeros(keys.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(keys.shape[1]):
            h = ((h ^ keys[:, i]) * np.uint64(0x9E3779B97F4A7C15)) & M64
            h ^= h >> np.uint64(29)
        tail = (t.counts.astype(np.uint64) | (t.left.astype(np.uint64) << np.uint64(16)) |
                (t.right.astype(np.uint64) << np.uint64(24)))
        h = ((h ^ tail) * np.uint64(0xD6E8FEB86659FD93)) & M64
        h ^= h >> np.uint64(32)
        return keys.shape[0], int(t.counts.astype(np.uint64).sum()), int(h.sum(dtype=np.uint64))


def test_adapter_calls_compile_for_every_max_k(exe):
    """CPU: add_reads_fname, add_fastq_mates_files and fastq_mates_info instantiate for MAX_K = 32, 64, 96 and 128."""
    assert subprocess.run([str(exe)], env={"MHMKC_NO_TORCH": "1"}).returncode == 2  # usage: no GPU touched


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_add_reads_fname_equals_the_python_adapter(exe, k, tmp_path, monkeypatch):
    import mhm2_proxy_amd as m
    a, b = M.split_mates(c.paired_fastq_text(2000, seed=95))
    b = M.trim_mate2(M.drop_records(b, 3), 0.5)
    (tmp_path / "r1.fq").write_bytes(a)
    (tmp_path / "r2.fq").write_bytes(b)
    name = f"{tmp_path / 'r1.fq'}:{tmp_path / 'r2.fq'}"
    monkeypatch.setenv("MHMKC_FQ_BLOCK", "20011")
    out = subprocess.run([str(exe), str(k), name], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    words = out.stdout.split()
    with m.KmerCounter(k, device=0) as cnt:
        cnt.add_fastq_named(name)
        info = cnt.fastq_mates_info()
        M.assert_equals_oracle(cnt, a, b, k)  # (the Python result is itself the oracle's)
        rows, counts, digest = table_digest(cnt.fetch())
    assert words[0] == "OK" and rows > 1000
    assert [int(w) for w in words[1:]] == [rows, counts, digest, 1997, info["rounds"]] and info["rounds"] > 10
