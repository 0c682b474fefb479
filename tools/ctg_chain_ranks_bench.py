"""Timing of the step from one contigging round to the next k over several ranks with 2 and 4 ranks on
one MI355X: the device route (mhmkc_add_ctgs_from after mhmkc_uutigs_ranks, the contigs gathered on the GPUs inside
mhmkc_finish) against the route through the host (uutig_strings() + mhmkc_add_ctgs, gathered by gather_ctgs).

  python tools/ctg_chain_ranks_bench.py --out profiles/ctgs_ranks_k21_33.json

Workload: bench.py's C2 generator (150 bp reads of a 50 Mbp genome, seed 2), --reads-per-rank reads per rank (rank r
takes reads [r R, (r + 1) R)), counted at --k with MHMKC_OWNER_MINIMIZER, its uutigs built by uutigs_ranks(), then counted
at --k2 with every rank's part of those uutigs as contigs. The ranks are processes that SHARE ONE GPU and exchange through
the host transport (gloo, staged through pinned host memory), so the figures show the mechanism and the bytes moved, not
xGMI speed.

Every run: the first counter's round and uutigs_ranks(); the next counter gets its reads; then, after a barrier, the timed
part of each route in turn on that same build: from the hand-over's first call to the end of finish(). --warmup runs, then
the median of --reps, per world the slowest rank's. The two routes' union tables are compared by an order-free digest.
Wire bytes: the device route's from mhmkc_ctgs_ranks_info; the host route's all-gather record rec x g from the sizes
(gather_ctgs: 8 B per contig length, 2 B per depth, 1 B per base, each padded to the largest rank's).
"""
from __future__ import annotations

import argparse
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

MASK = (1 << 64) - 1


def med(xs):
    return round(statistics.median(xs), 3)


def mix64(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def table_digest(t) -> tuple:
    """(rows, the wrapping sum over the rows of a 64-bit hash of key words, count and extensions): order-free."""
    if not len(t):
        return 0, 0
    h = np.zeros(len(t), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for w in range(t.keys.shape[1]):
            h = mix64(h ^ t.keys[:, w].astype(np.uint64)) + np.uint64(w + 1)
        tail = t.counts.astype(np.uint64) | (t.left.view(np.uint8).astype(np.uint64) << np.uint64(16)) | \
            (t.right.view(np.uint8).astype(np.uint64) << np.uint64(24))
        h = mix64(h ^ tail)
        return len(t), int(h.sum(dtype=np.uint64))


def align8(x: int) -> int:
    return (x + 7) // 8 * 8


def worker(rank: int, world: int, port: int, args, out_dir: str):
    import torch
    import torch.distributed as dist

    import mhm2_proxy_amd as m

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    R, dev = args.reads_per_rank, torch.device("cuda", 0)
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, R, 150, args.seed, first_read=rank * R, threads=max(1, args.threads // world))
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases_in = int(o[-1])
    del b, o, genome

    def counter(k):
        return m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                             output_owner=m.MHMKC_OWNER_MINIMIZER)

    a, nxt = counter(args.k), counter(args.k2)
    runs = {"device": [], "host": []}
    hand = {"device": [], "host": []}
    infos, digests, sizes = [], {}, None
    for r in range(args.warmup + args.reps):
        a.reset()
        a.add_tensors(bt, ot, n_bases_in)
        a.finish()
        res = a.uutigs_ranks()
        for route in ("device", "host"):
            nxt.reset()
            nxt.add_tensors(bt, ot, n_bases_in)
            torch.cuda.synchronize()  # (the reads' extraction is enqueued: not part of the timed step)
            dist.barrier()
            t0 = time.perf_counter()
            if route == "device":
                nxt.add_ctgs_from(a)
            else:
                strs, depths = a.uutig_strings()
                nxt.add_ctgs(strs, np.minimum(depths, 65535.0).astype(np.uint16))
            t1 = time.perf_counter()
            nxt.finish()
            t2 = time.perf_counter()
            info = nxt.ctgs_ranks_info()
            assert info["device_route"] == (1 if route == "device" else 0), info
            if r >= args.warmup:
                runs[route].append((t2 - t0) * 1e3)
                hand[route].append((t1 - t0) * 1e3)
                if route == "device":
                    infos.append(info)
            if r == args.warmup + args.reps - 1:
                digests[route] = list(table_digest(nxt.fetch()))
                sizes = info
    st = nxt.stats()
    out = {"rank": rank, "n_ctgs": res["n_ctgs"], "n_bases": sizes["n_bases"], "n_ctgs_all": sizes["n_ctgs_all"],
           "n_bases_all": sizes["n_bases_all"], "windows_all": sizes["windows_all"], "ctg_kmers": st["ctg_kmers"],
           "digest": digests,
           "device": {"wall_ms": med(runs["device"]), "handover_ms": med(hand["device"]),
                      "wall_runs_ms": [round(x, 1) for x in runs["device"]],
                      "stages_ms": {s: med([i[s] for i in infos]) for s in ("ms_pack", "ms_move", "ms_assemble", "ms_total")},
                      "bytes_sent": infos[-1]["bytes_sent"], "bytes_recv": infos[-1]["bytes_recv"],
                      "gathered_bytes": infos[-1]["gathered_bytes"]},
           "host": {"wall_ms": med(runs["host"]), "handover_ms": med(hand["host"]),
                    "wall_runs_ms": [round(x, 1) for x in runs["host"]]}}
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(out))
    a.close()
    nxt.close()
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
    ap.add_argument("--k2", type=int, default=33)
    ap.add_argument("--worlds", default="2,4")
    ap.add_argument("--reads-per-rank", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.multiprocessing as mp

    from mhm2_proxy_amd.build import source_build_id

    if not torch.cuda.is_available():
        sys.exit("ctg_chain_ranks_bench.py needs the GPU (no fallback)")
    res = {"tool": "tools/ctg_chain_ranks_bench.py", "build_id": source_build_id(), "k": args.k, "k2": args.k2,
           "workload": f"C2's generator: {args.reads_per_rank} x 150 bp reads per rank, genome {args.genome} bp, seed {args.seed}",
           "setting": "the ranks are processes sharing ONE MI355X, exchanging over gloo through pinned host memory: the "
                      "mechanism and the byte counts, not xGMI speed",
           "reps": args.reps, "warmup": args.warmup,
           "statistic": "median over reps; per world the slowest rank's wall clock from the hand-over's first call to the end "
                        "of the next finish (its reads added before); stage times from device events (mhmkc_ctgs_ranks_info)",
           "worlds": {}}
    for world in [int(x) for x in args.worlds.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(worker, args=(world, free_port(), args, d), nprocs=world, join=True)
            ranks = [json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(world)]
        dg = {route: [sum(r["digest"][route][0] for r in ranks), sum(r["digest"][route][1] for r in ranks) & MASK]
              for route in ("device", "host")}
        slow_d = max(ranks, key=lambda r: r["device"]["wall_ms"])
        slow_h = max(ranks, key=lambda r: r["host"]["wall_ms"])
        max_c = max(r["n_ctgs"] for r in ranks)
        max_b = max(r["n_bases"] for r in ranks)
        rec = 8 * max_c + align8(2 * max_c) + align8(max_b)
        w = {"n_ctgs_all": ranks[0]["n_ctgs_all"], "n_bases_all": ranks[0]["n_bases_all"],
             "windows_all": ranks[0]["windows_all"], "ctgs_per_rank": [r["n_ctgs"] for r in ranks],
             "bases_per_rank": [r["n_bases"] for r in ranks],
             "device_wall_ms": slow_d["device"]["wall_ms"], "device_handover_ms": slow_d["device"]["handover_ms"],
             "device_stages_ms": slow_d["device"]["stages_ms"],
             "host_wall_ms": slow_h["host"]["wall_ms"], "host_handover_ms": slow_h["host"]["handover_ms"],
             "ratio_host_over_device": round(slow_h["host"]["wall_ms"] / max(slow_d["device"]["wall_ms"], 1e-9), 2),
             "device_wire_bytes_sent": sum(r["device"]["bytes_sent"] for r in ranks),
             "device_wire_bytes_recv_per_rank": [r["device"]["bytes_recv"] for r in ranks],
             "host_gather_record_bytes": rec, "host_gather_bytes_recv_per_rank": rec * world,
             "gathered_bytes": [r["device"]["gathered_bytes"] for r in ranks],
             "digest": dg, "digests_equal": dg["device"] == dg["host"], "ranks": ranks}
        res["worlds"][str(world)] = w
        print(f"[ctg_chain_ranks_bench] world {world}: device {w['device_wall_ms']} ms, host {w['host_wall_ms']} ms, "
              f"digests equal {w['digests_equal']}", file=sys.stderr, flush=True)
    print(json.dumps({key: v for key, v in res.items() if key != "worlds"} |
                     {"worlds": {x: {key: v for key, v in w.items() if key != "ranks"} for x, w in res["worlds"].items()}}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
