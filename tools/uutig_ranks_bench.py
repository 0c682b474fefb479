"""Timing of the collective uutig build (mhmkc_uutigs_ranks) with 2 and 4 ranks on one MI355X.

  python tools/uutig_ranks_bench.py --k 21 --out profiles/uutig_ranks_k21.json
  python tools/uutig_ranks_bench.py --k 63 --out profiles/uutig_ranks_k63.json

Workload: bench.py's C2 generator (150 bp reads of a 50 Mbp genome, seed 2), --reads-per-rank reads per rank (rank r
takes reads [r R, (r + 1) R)), counted at --k with MHMKC_OWNER_MINIMIZER. The ranks are processes that SHARE ONE GPU and
exchange through the host transport (gloo, staged through host memory), so the figures show the mechanism and the bytes
moved, not xGMI speed: the kernels of the ranks run one after the other on the one device, and every moved byte crosses
PCIe twice.

Every run counts the reads again (reset, add, finish: the build is dropped with the table) and times the collective
build: wall clock around uutigs_ranks() after a barrier, and the library's stage events (mhmkc_uutigs_ranks_info),
--warmup runs, then the median of --reps. Beside it, on the same box, with the contig lists compared by digest:
  single  mhmkc_uutigs on the union table at one rank (one counter given all the ranks' reads; index + links + uutigs),
  host    the route that exists without the collective: every rank fetches its table, then ONE host thread runs
          mhmkc_dbjg_traverse (tools/cpp/dbjg_lib.cpp) over the union. RUN ONCE (it takes this long); --no-host skips it.
The digest is order-free: the sum of a 64-bit hash of every contig's canonical sequence and Contig::get_uint16_t_depth.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

COMP = str.maketrans("ACGT", "TGCA")
MASK = (1 << 64) - 1


def med(xs):
    return round(statistics.median(xs), 3)


def digest(seqs, depth16) -> tuple:
    """(number of contigs, bases, the wrapping sum of a 64-bit hash of "<canonical sequence> <depth>" per contig)."""
    total = bases = 0
    for s, d in zip(seqs, depth16):
        r = s[::-1].translate(COMP)
        total = (total + int.from_bytes(hashlib.blake2b(f"{min(s, r)} {int(d)}".encode(), digest_size=8).digest(), "little")) & MASK
        bases += len(s)
    return len(depth16), bases, total


def worker(rank: int, world: int, port: int, args, out_dir: str):
    import torch
    import torch.distributed as dist

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd.build import DBJG

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    k, R, dev = args.k, args.reads_per_rank, torch.device("cuda", 0)
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, R, 150, args.seed, first_read=rank * R, threads=max(1, args.threads // world))
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases_in = int(o[-1])
    del b, o
    c = m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                      output_owner=m.MHMKC_OWNER_MINIMIZER)
    wall, infos = [], []
    for r in range(args.warmup + args.reps):
        c.reset()
        c.add_tensors(bt, ot, n_bases_in)
        c.finish()
        dist.barrier()
        t0 = time.perf_counter()
        res = c.uutigs_ranks()
        t1 = time.perf_counter()
        if r >= args.warmup:
            wall.append((t1 - t0) * 1e3)
            infos.append(c.uutigs_ranks_info())
    st = c.stats()
    strs, depths = c.uutig_strings()
    mine = digest(strs, np.minimum(depths, 65535.0).astype(np.uint16))
    del strs, depths
    # the route without the collective: every rank fetches its table ...
    dist.barrier()
    t0 = time.perf_counter()
    t = c.fetch()
    fetch_ms = (time.perf_counter() - t0) * 1e3
    nl = k // 32 + 1
    if not args.no_host:
        np.savez(Path(out_dir) / f"rank{rank}.npz", keys=np.ascontiguousarray(t.keys[:, :nl]), counts=t.counts,
                 left=t.left, right=t.right)
    n_rows = len(t)
    del t
    c.close()
    info = infos[-1]
    out = {"rank": rank, "n_rows": n_rows, "n_ctgs": res["n_ctgs"], "first_id": res["first_id"],
           "n_ctgs_all": res["n_ctgs_all"], "digest": list(mine), "wall_ms": med(wall),
           "wall_runs_ms": [round(x, 1) for x in wall], "fetch_ms": round(fetch_ms, 1),
           "stages_ms": {s: med([i["ms_stage"][s] for i in infos]) for s in info["ms_stage"]},
           "ms_total": med([i["ms_total"] for i in infos]), "rounds": info["rounds"], "cycle_rounds": info["cycle_rounds"],
           "cycle_ports": info["cycle_ports"], "routed_bytes_sent": sum(info["routed_bytes_sent"].values()),
           "routed_bytes_recv": sum(info["routed_bytes_recv"].values()),
           "routed_records_sent": sum(info["routed_records_sent"].values()), "scratch_bytes": info["scratch_bytes"],
           "kept_bytes": info["kept_bytes"], "device_bytes_peak": st["device_bytes_peak"]}
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(out))
    dist.barrier()
    if rank == 0:
        ref = {}
        if not args.no_host:  # ... and one host thread walks the union
            parts = [np.load(Path(out_dir) / f"rank{r}.npz") for r in range(world)]
            keys = np.ascontiguousarray(np.concatenate([p["keys"] for p in parts]), dtype=np.uint64)
            counts = np.ascontiguousarray(np.concatenate([p["counts"] for p in parts]), dtype=np.uint16)
            left = np.ascontiguousarray(np.concatenate([p["left"] for p in parts])).view(np.uint8)
            right = np.ascontiguousarray(np.concatenate([p["right"] for p in parts])).view(np.uint8)
            del parts
            L = C.CDLL(str(DBJG))
            L.mhmkc_dbjg_traverse.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p]
            L.mhmkc_dbjg_traverse.restype = C.c_int64
            path = Path(out_dir) / "host_ctgs.txt"
            t0 = time.perf_counter()
            n = L.mhmkc_dbjg_traverse(k, keys.ctypes.data, counts.ctypes.data, left.ctypes.data, right.ctypes.data,
                                      keys.shape[0], os.fsencode(str(path)))
            ms = (time.perf_counter() - t0) * 1e3
            del keys, counts, left, right
            seqs, d16 = [], []
            with open(path) as f:
                for line in f:
                    s, d = line.split()
                    seqs.append(s)
                    d16.append(int(d))
            ref["host"] = {"traverse_ms": round(ms, 1), "runs": 1, "n_ctgs": int(n), "digest": list(digest(seqs, d16)),
                           "kind": "mhmkc_dbjg_traverse over the union on one host thread (table load, walk, contig file)"}
            del seqs, d16
        # mhmkc_uutigs on the union table at one rank
        b, o = m.synth_reads(genome, world * R, 150, args.seed, threads=args.threads)
        bt = torch.from_numpy(b).to(dev)
        ot = torch.from_numpy(o.view(np.int64)).to(dev)
        nb = int(o[-1])
        del b, o
        s1 = m.KmerCounter(k, device=0)
        runs = []
        for r in range(1 + 3):
            s1.reset()
            s1.add_tensors(bt, ot, nb)
            n1 = s1.finish()
            t0 = time.perf_counter()
            s1.uutigs_device()
            s1.synchronize()
            t1 = time.perf_counter()
            i1 = s1.uutigs_info()
            if r:
                runs.append(((t1 - t0) * 1e3, i1["ms_links"] + i1["ms_total"]))
        strs, depths = s1.uutig_strings()
        ref["single"] = {"n_rows": int(n1), "wall_ms": med([x[0] for x in runs]), "events_ms": med([x[1] for x in runs]),
                         "runs": len(runs), "digest": list(digest(strs, np.minimum(depths, 65535.0).astype(np.uint16))),
                         "kind": "one counter given all ranks' reads: index + links + mhmkc_uutigs"}
        s1.close()
        Path(out_dir, "ref.json").write_text(json.dumps(ref))
    dist.barrier()
    dist.destroy_process_group()


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--worlds", default="2,4")
    ap.add_argument("--reads-per-rank", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.multiprocessing as mp

    from mhm2_proxy_amd.build import source_build_id

    if not torch.cuda.is_available():
        sys.exit("uutig_ranks_bench.py needs the GPU (no fallback)")
    res = {"tool": "tools/uutig_ranks_bench.py", "build_id": source_build_id(), "k": args.k,
           "workload": f"C2's generator: {args.reads_per_rank} x 150 bp reads per rank, genome {args.genome} bp, seed {args.seed}",
           "setting": "the ranks are processes sharing ONE MI355X, exchanging over gloo through host memory: the mechanism "
                      "and the byte counts, not xGMI speed",
           "reps": args.reps, "warmup": args.warmup,
           "statistic": "median over reps; per world the slowest rank's wall clock around uutigs_ranks() after a barrier; "
                        "stage times from device events (mhmkc_uutigs_ranks_info)", "worlds": {}}
    for world in [int(x) for x in args.worlds.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(worker, args=(world, free_port(), args, d), nprocs=world, join=True)
            ranks = [json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(world)]
            ref = json.loads(Path(d, "ref.json").read_text())
        n_rows = sum(r["n_rows"] for r in ranks)
        dg = [sum(r["digest"][0] for r in ranks), sum(r["digest"][1] for r in ranks), sum(r["digest"][2] for r in ranks) & MASK]
        slow = max(ranks, key=lambda r: r["wall_ms"])
        w = {"n_rows": n_rows, "n_ctgs_all": ranks[0]["n_ctgs_all"], "rows_per_rank": [r["n_rows"] for r in ranks],
             "ctgs_per_rank": [r["n_ctgs"] for r in ranks], "collective_wall_ms": slow["wall_ms"],
             "collective_stages_ms": slow["stages_ms"], "collective_events_ms": slow["ms_total"],
             "rounds": ranks[0]["rounds"], "cycle_rounds": ranks[0]["cycle_rounds"], "cycle_ports": ranks[0]["cycle_ports"],
             "routed_bytes": sum(r["routed_bytes_sent"] for r in ranks),
             "routed_bytes_in": sum(r["routed_bytes_recv"] for r in ranks),
             "routed_bytes_per_row": round(sum(r["routed_bytes_sent"] for r in ranks) / max(n_rows, 1), 1),
             "scratch_bytes_per_union_row": round(max(r["scratch_bytes"] for r in ranks) / max(n_rows, 1), 1),
             "kept_bytes": [r["kept_bytes"] for r in ranks], "digest": dg, "single_rank": ref["single"],
             "host_route": None, "ranks": ranks}
        w["digests_equal_single"] = dg == ref["single"]["digest"]
        if "host" in ref:
            h = ref["host"]
            fetch = max(r["fetch_ms"] for r in ranks)
            w["host_route"] = dict(h, fetch_ms=fetch, total_ms=round(fetch + h["traverse_ms"], 1))
            w["digests_equal_host"] = dg == h["digest"]
            w["ratio_host_over_collective"] = round((fetch + h["traverse_ms"]) / slow["wall_ms"], 1)
        res["worlds"][str(world)] = w
        print(f"[uutig_ranks_bench] k={args.k} world {world}: collective {slow['wall_ms']} ms, {n_rows} rows", file=sys.stderr,
              flush=True)
    print(json.dumps({key: v for key, v in res.items() if key != "worlds"} |
                     {"worlds": {x: {key: v for key, v in w.items() if key != "ranks"} for x, w in res["worlds"].items()}}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
