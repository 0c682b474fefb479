"""Timing of read pairs from two mate files (mhmkc_add_fastq_mates_device, mhmkc_add_fastq_mates_files)
against the interleaved entry points on the same bytes.

  python tools/fastq_mates_bench.py --out profiles/fastq_mates_bench.json

One rank. Input: bench.py's fastq-pairs workload (--pairs pairs of 150-base mates from the C2 genome, seed 2), as two
mate files and as their interleaving, on tmpfs (--dir, default /dev/shm). Every timed run is reset + add + finish, wall
clock with the device drained; --warmup runs per arm, then --reps runs with the arms of a comparison alternated (A B,
B A, ...); min and median are reported, and the spread (max - min) of each arm.
  (a) device   add_fastq_mates_tensors on the two texts in HBM  vs  add_fastq_tensor(pairs=True) on the interleaved text
  (b) files    add_fastq_mates_files(r1, r2)                    vs  add_fastq_file(interleaved, pairs=True)
  (c) today    the host interleave of r1 and r2 into a third file (a plain single-threaded pass, four lines from each
               file in turn) + the one-file call on that file    vs  the two-file call; one warm-up, then --c-reps
               alternated runs (the interleave takes seconds)
After the timed runs every arm's finished table is fetched once and digested (row count, sum of counts, an
order-independent 64-bit mix of the rows): the tool exits non-zero and writes nothing unless all digests are equal.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from itertools import islice
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def table_digest(t) -> list:
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
        return [int(keys.shape[0]), int(t.counts.astype(np.uint64).sum()), int(h.sum(dtype=np.uint64))]


def host_interleave(p1: Path, p2: Path, out: Path) -> float:
    """What a user does today: four lines from each file in turn into a third file, on one thread."""
    t0 = time.perf_counter()
    with open(p1, "rb") as f1, open(p2, "rb") as f2, open(out, "wb", buffering=1 << 24) as fo:
        while True:
            r1 = list(islice(f1, 4))
            r2 = list(islice(f2, 4))
            if len(r1) < 4 or len(r2) < 4:
                break
            fo.writelines(r1)
            fo.writelines(r2)
    return time.perf_counter() - t0


def summary(ms: list) -> dict:
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3),
            "spread_ms": round(max(ms) - min(ms), 3), "runs_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--c-reps", type=int, default=3, help="runs of comparison (c), whose host interleave takes seconds")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fastq_mates_bench.json"))
    args = ap.parse_args()

    import torch

    import bench
    import mhm2_proxy_amd as m

    L, G, seed = 150, 50_000_000, 2
    t0 = time.perf_counter()
    genome = m.synth_genome(G, seed)
    text = bench.paired_fastq_text(genome, args.pairs, L, seed)
    del genome
    rec = text.size // (2 * args.pairs)
    recs = text.reshape(2 * args.pairs, rec)
    t1, t2 = np.ascontiguousarray(recs[0::2]).reshape(-1), np.ascontiguousarray(recs[1::2]).reshape(-1)
    d = Path(args.dir)
    tag = f"mhmkc_mates_{os.getpid()}"
    p1, p2, pi, p3 = (d / f"{tag}_{s}.fq" for s in ("r1", "r2", "inter", "inter_host"))
    files = [p1, p2, pi, p3]
    try:
        t1.tofile(str(p1))
        t2.tofile(str(p2))
        text.tofile(str(pi))
        gen_s = time.perf_counter() - t0
        dev = torch.device("cuda", 0)

        def on_device(a):
            t = torch.zeros(int(a.size) + 16, dtype=torch.uint8, device=dev)
            t[: a.size].copy_(torch.from_numpy(a))
            return t

        d1, d2, di = on_device(t1), on_device(t2), on_device(text)
        n1, n2, ni = int(t1.size), int(t2.size), int(text.size)
        del t1, t2, text, recs
        cnt = m.KmerCounter(args.k, device=0)
        arms = {
            "mates_device": lambda: cnt.add_fastq_mates_tensors(d1, d2, n1, n2),
            "pairs_device": lambda: cnt.add_fastq_tensor(di, n_bytes=ni, pairs=True),
            "mates_files": lambda: cnt.add_fastq_mates_files(p1, p2),
            "pairs_file": lambda: cnt.add_fastq_file(pi, pairs=True),
        }

        def run(name) -> float:
            cnt.reset()
            torch.cuda.synchronize()
            t = time.perf_counter()
            arms[name]()
            cnt.finish()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        times = {name: [] for name in arms}
        infos = {}
        for group in (("mates_device", "pairs_device"), ("mates_files", "pairs_file")):
            for name in group:
                for _ in range(args.warmup):
                    run(name)
            for r in range(args.reps):
                for name in (group if r % 2 == 0 else group[::-1]):
                    times[name].append(run(name))
                    if name.startswith("mates"):
                        infos[name] = cnt.fastq_mates_info()
        # (c): the user's route today, end to end (host interleave into a third file, then the one-file call on it),
        # alternated with the two-file call; one warm-up each
        arms["today_file"] = lambda: cnt.add_fastq_file(p3, pairs=True)
        times["today_interleave"], times["today_total"], times["mates_files_c"] = [], [], []
        for r in range(-1, args.c_reps):
            order = ("today", "mates") if r % 2 == 0 else ("mates", "today")
            for which in order:
                if which == "today":
                    il = host_interleave(p1, p2, p3) * 1e3
                    tot = il + run("today_file")
                    if r >= 0:
                        times["today_interleave"].append(il)
                        times["today_total"].append(tot)
                else:
                    t = run("mates_files")
                    if r >= 0:
                        times["mates_files_c"].append(t)
        same_file = p3.read_bytes() == pi.read_bytes() if args.pairs <= 1_000_000 else p3.stat().st_size == pi.stat().st_size
        digests, stats = {}, {}
        for name in arms:  # (today_file: the table from the host-interleaved file)
            run(name)
            stats[name] = {key: cnt.stats()[key] for key in ("fq_pairs", "fq_merged", "fq_ambiguous", "fq_overlap_bases",
                                                             "reads", "bases", "fq_file_blocks")}
            digests[name] = table_digest(cnt.fetch())
    finally:
        for f in files:
            if f.exists():
                f.unlink()
    ok = len({tuple(v) for v in digests.values()}) == 1 and same_file and \
        len({tuple(sorted((k, v) for k, v in s.items() if k != "fq_file_blocks")) for s in stats.values()}) == 1
    res = {name: summary(ms) for name, ms in times.items()}
    ratio = lambda a, b, key: round(res[a][key] / res[b][key], 4)  # noqa: E731
    out = {
        "tool": "tools/fastq_mates_bench.py", "k": args.k, "pairs": args.pairs, "read_len": L, "text_bytes": ni,
        "file_bytes": [n1, n2], "reps": args.reps, "warmup": args.warmup, "input_build_s": round(gen_s, 2),
        "device": torch.cuda.get_device_name(0),
        "arms": res,
        "a_device_mates_over_pairs": {"min": ratio("mates_device", "pairs_device", "min_ms"),
                                      "median": ratio("mates_device", "pairs_device", "median_ms")},
        "b_files_mates_over_pairs_file": {"min": ratio("mates_files", "pairs_file", "min_ms"),
                                          "median": ratio("mates_files", "pairs_file", "median_ms")},
        "c_two_files_over_today": {"min": ratio("mates_files_c", "today_total", "min_ms"),
                                   "median": ratio("mates_files_c", "today_total", "median_ms")},
        "mates_info": infos, "stats": stats, "table_digests": digests, "tables_equal": ok,
    }
    print(json.dumps(out))
    if not ok:
        print("the arms' tables or statistics differ: nothing written", file=sys.stderr)
        sys.exit(1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
