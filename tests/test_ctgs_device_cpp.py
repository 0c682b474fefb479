"""The host halves of the device contig input (tests/cpp/ctg_pack_check.cpp: the byte map, its SWAR form and the depth
conversion of kmer_ops.hpp) and the C++ adapter's device hand-over between contigging rounds
(tests/cpp/ctg_chain_test.cpp: analyze_kmers with the previous round's KmerDHT)."""
import shutil
import subprocess
from pathlib import Path

import pytest

import mhm2_proxy_amd as m
from common import synth_set

ROOT = Path(__file__).resolve().parents[1]
CPP = ROOT / "tests" / "cpp"


def test_byte_map_and_depth_conversion_on_the_host(tmp_path):
    """CPU: ctg_pack4 over all 256 byte values in every lane against a per-character switch, ctg_depth_u16 against the
    reference's expression; built with the address and undefined-behaviour sanitizers."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path / "ctg_pack_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(CPP / "ctg_pack_check.cpp"), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-2000:] + out.stderr[-2000:]


def build_chain(tmp: Path) -> Path:
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    from mhm2_proxy_amd import build as b

    b.build_lib()
    exe = tmp / "ctg_chain_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(CPP / "ctg_chain_test.cpp"),
                    f"-L{ROOT / 'mhm2_proxy_amd'}", "-lmhmkc", "-lz", f"-Wl,-rpath,{ROOT / 'mhm2_proxy_amd'}",
                    "-o", str(exe)], check=True)
    return exe


def test_device_hand_over_compiles_for_every_max_k_pair(tmp_path):
    """CPU: HashTableInserter::add_ctgs_from and the analyze_kmers overload instantiate for (PREV_MAX_K, MAX_K) in
    {32, 64, 96, 128}^2 with PREV_MAX_K <= MAX_K (ctg_chain_test's dispatch names all ten)."""
    exe = build_chain(tmp_path)
    assert subprocess.run([str(exe)], env={"MHMKC_NO_TORCH": "1"}).returncode == 2  # usage: no GPU touched
    syms = subprocess.run(["nm", "-C", str(exe)], capture_output=True, text=True, check=True).stdout
    for prev, cur in [(p, c) for p in (32, 64, 96, 128) for c in (32, 64, 96, 128) if p <= c]:
        assert f"round_k<{cur}, {prev}>" in syms, (prev, cur)


@pytest.mark.gpu
def test_chain_21_33_55_equals_the_route_through_the_host(tmp_path):
    exe = build_chain(tmp_path)
    b, o = synth_set(1500, 10000, 7)
    pr = m.PackedReads.from_arrays(b, o)
    reads = tmp_path / "reads.txt"
    with open(reads, "w") as f:
        for i in range(pr.get_local_num_reads()):
            _, s, q = pr.get_read(i)
            f.write(f"{s} {q}\n")
    out = subprocess.run([str(exe), str(reads), "21,33,55"], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rounds = [ln.split() for ln in lines if ln.startswith("ROUND")]
    assert [r[1] for r in rounds] == ["33", "55"] and "OK" in lines
    for r in rounds:
        assert int(r[2]) > 5000 and int(r[3]) > 0  # rows, folded contig k-mers
