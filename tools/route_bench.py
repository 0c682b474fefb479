"""The de Bruijn links across ranks by queries routed to the owner (mhmkc_dbjg_links_ranks), with 2
and 4 ranks on one MI355X, beside the route that existed before: the gather of every rank's rows and the links of the union.

  python tools/route_bench.py --k 21 --out profiles/route_ranks_k21.json
  python tools/route_bench.py --k 63 --out profiles/route_ranks_k63.json

Workload: bench.py's C2 generator (150 bp reads of a 50 Mbp genome, seed 2), --reads-per-rank reads per rank (rank r
takes reads [r R, (r + 1) R)), counted at --k with MHMKC_OWNER_MINIMIZER. The ranks are processes that SHARE ONE GPU and
exchange through the host transport (gloo, staged through host memory). So the TIMES show the mechanism only: the ranks'
kernels run one after the other on the one device and every moved byte crosses PCIe twice; no time here is a claim about
xGMI. The BYTES and the MEMORY do carry over: they are counts, the same on any transport.

Every run counts the reads again (reset, add, finish: the links are dropped with the table), then, on the same table:
  routed  wall clock around dbjg_links_ranks_device() after a barrier, and mhmkc_route_info: stages, rounds, the share
          of queries answered locally, the bytes sent, the scratch;
  gather  the only route to the same links without it: mhmkc_uutigs_ranks's GATHER stage (every rank receives every
          other rank's rows) plus ms_links of the union (its index and links on every rank), from that call's info.
--warmup runs, then the median of --reps. The two link sets are compared by an order-free digest over (key, direction,
neighbour key, status), computed on the host from the fetched arrays: the routed links of all ranks (the neighbour's key read from the
union of the ranks' tables at (next_rank, next_row)) against mhmkc_dbjg_links of ONE counter given all the ranks' reads.
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
NO_ROW, NO_RANK = 0xFFFFFFFF, 0xFF


def med(xs):
    return round(statistics.median(xs), 3)


_C1 = np.uint64(0xBF58476D1CE4E5B9)


def _mix(h, v):
    """One multiply-xorshift step in wrapping uint64 arithmetic."""
    h = (h ^ v) * _C1
    return h ^ (h >> np.uint64(31))


def link_digest(keys, nb_keys, has_nb, status) -> int:
    """The wrapping sum over the 2 n entries of a hash of (key words, direction, neighbour key words or zeros, status).
    keys [n, nl] uint64, nb_keys [2 n, nl] uint64, has_nb [2 n] bool, status [2 n] uint8. On the host, in numpy, one
    direction at a time (a torch version of the same sums on the device did not reproduce its own result from one
    count to the next at two-word keys, while this one does)."""
    n, total = keys.shape[0], 0
    with np.errstate(over="ignore"):
        for d in (0, 1):
            sl = slice(d * n, (d + 1) * n)
            h = np.full(n, 0x9E3779B97F4A7C15, dtype=np.uint64)
            for w in range(keys.shape[1]):
                h = _mix(h, keys[:, w])
            h = _mix(h, np.uint64(d + 1))
            for w in range(keys.shape[1]):
                h = _mix(h, np.where(has_nb[sl], nb_keys[sl, w], np.uint64(0)))
            h = _mix(h, status[sl].astype(np.uint64) + np.uint64(7))
            total = (total + int(h.sum(dtype=np.uint64))) & MASK
    return total


def table_digest(t) -> int:
    """The wrapping sum over the rows of a hash of (key words, count, left, right): are the two tables the same set?"""
    nl = t.k // 32 + 1
    with np.errstate(over="ignore"):
        h = np.full(len(t), 0x9E3779B97F4A7C15, dtype=np.uint64)
        for w in range(nl):
            h = _mix(h, t.keys[:, w])
        h = _mix(h, t.counts.astype(np.uint64))
        h = _mix(h, t.left.view(np.uint8).astype(np.uint64) * np.uint64(256) + t.right.view(np.uint8).astype(np.uint64))
        return int(h.sum(dtype=np.uint64)) & MASK


def status_hist(status) -> list:
    """Entries per status value (OK, DEADEND, FORK, CONFLICT, OK | RC)."""
    b = np.bincount(status.reshape(-1), minlength=256)
    return [int(b[v]) for v in (0, 1, 2, 3, 0x80)]


def worker(rank: int, world: int, port: int, args, out_dir: str):
    import datetime

    import torch
    import torch.distributed as dist

    import mhm2_proxy_amd as m

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    k, R, dev = args.k, args.reads_per_rank, torch.device("cuda", 0)
    nl = k // 32 + 1
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, R, 150, args.seed, first_read=rank * R, threads=max(1, args.threads // world))
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases_in = int(o[-1])
    del b, o
    c = m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                      output_owner=m.MHMKC_OWNER_MINIMIZER)
    wall, infos, gather, gather_bytes, gather_scratch = [], [], [], 0, 0
    for r in range(args.warmup + args.reps):
        c.reset()
        c.add_tensors(bt, ot, n_bases_in)
        c.finish()
        dist.barrier()
        t0 = time.perf_counter()
        c.dbjg_links_ranks_device()
        t1 = time.perf_counter()
        info = c.route_info()
        dist.barrier()
        c.uutigs_ranks()  # (drops the rank's own index; the routed links stay)
        ui, ul = c.uutigs_ranks_info(), c.uutigs_info()
        if r >= args.warmup:
            wall.append((t1 - t0) * 1e3)
            infos.append(info)
            gather.append((ui["ms_stage"]["gather"], ul["ms_links"]))
            gather_bytes, gather_scratch = ui["routed_bytes_sent"]["gather"], ui["scratch_bytes"]
    # the digest of this rank's routed links, the neighbours' keys read from the union of the ranks' tables (host copies)
    t = c.fetch()
    n = len(t)
    next_rank, next_row, status = (x.reshape(-1) for x in c.dbjg_links_ranks())  # (kept: no collective)
    keys = np.ascontiguousarray(t.keys[:, :nl])
    np.save(Path(out_dir) / f"keys{rank}.npy", keys)
    dist.barrier()
    parts = [np.load(Path(out_dir) / f"keys{r}.npy") for r in range(world)]
    bases = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    union = np.concatenate(parts)
    del parts
    dg, tdg, hist = 0, 0, [0] * 5
    if n:
        tdg = table_digest(t)
        has = next_rank != NO_RANK
        gi = np.where(has, bases[np.where(has, next_rank, 0)] + next_row.astype(np.int64), 0)
        dg = link_digest(keys, union[gi], has, status)
        hist = status_hist(status)
        del gi, has
    del union, t
    last = infos[-1]
    out = {"rank": rank, "n_rows": n, "wall_ms": med(wall), "wall_runs_ms": [round(x, 1) for x in wall],
           "stages_ms": {s: med([i["ms_stage"][s] for i in infos]) for s in last["ms_stage"]},
           "rounds": last["rounds"], "chunk": last["chunk"], "entries": last["entries"], "queries": last["queries"],
           "queries_local": last["queries_local"], "queries_sent": last["queries_sent"],
           "queries_recv": last["queries_recv"], "bytes_sent": last["bytes_sent"], "bytes_recv": last["bytes_recv"],
           "scratch_bytes": last["scratch_bytes"], "kept_bytes": last["kept_bytes"], "digest": dg, "table_digest": tdg,
           "status_entries": hist,
           "gather_ms": med([g[0] for g in gather]), "union_links_ms": med([g[1] for g in gather]),
           "gather_route_ms": med([g[0] + g[1] for g in gather]), "gather_bytes_sent": gather_bytes,
           "gather_scratch_bytes": gather_scratch}
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(out))
    c.close()
    dist.barrier()
    if rank == 0:  # mhmkc_dbjg_links of one counter given all the ranks' reads
        del bt, ot
        b, o = m.synth_reads(genome, world * R, 150, args.seed, threads=args.threads)
        bt = torch.from_numpy(b).to(dev)
        ot = torch.from_numpy(o.view(np.int64)).to(dev)
        nb = int(o[-1])
        del b, o
        s1 = m.KmerCounter(k, device=0)
        s1.add_tensors(bt, ot, nb)
        n1 = s1.finish()
        t1 = s1.fetch()
        nxt, st1 = (x.reshape(-1) for x in s1.dbjg_links())
        keys1 = np.ascontiguousarray(t1.keys[:, :nl])
        has = nxt != NO_ROW
        dg1 = link_digest(keys1, keys1[np.where(has, nxt, 0)], has, st1)
        Path(out_dir, "ref.json").write_text(json.dumps({"n_rows": int(n1), "digest": dg1, "table_digest": table_digest(t1),
                                                         "status_entries": status_hist(st1)}))
        s1.close()
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.multiprocessing as mp

    from mhm2_proxy_amd.build import source_build_id

    if not torch.cuda.is_available():
        sys.exit("route_bench.py needs the GPU (no fallback)")
    nl = args.k // 32 + 1
    res = {"tool": "tools/route_bench.py", "build_id": source_build_id(), "k": args.k,
           "workload": f"C2's generator: {args.reads_per_rank} x 150 bp reads per rank, genome {args.genome} bp, seed {args.seed}",
           "setting": "the ranks are processes sharing ONE MI355X, exchanging over gloo through host memory: the times show "
                      "the mechanism only (no time threshold is set on them); the bytes and the memory carry over",
           "reps": args.reps, "warmup": args.warmup,
           "statistic": "median over reps; per world the slowest rank's wall clock around dbjg_links_ranks_device() after a "
                        "barrier; stage times from device events (mhmkc_route_info); the gather route from "
                        "mhmkc_uutigs_ranks_info (GATHER) + mhmkc_uutigs_info (ms_links of the union) in the same run",
           "worlds": {}}
    for world in [int(x) for x in args.worlds.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(worker, args=(world, free_port(), args, d), nprocs=world, join=True)
            ranks = [json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(world)]
            ref = json.loads(Path(d, "ref.json").read_text())
        n_rows = sum(r["n_rows"] for r in ranks)
        slow = max(ranks, key=lambda r: r["wall_ms"])
        gslow = max(ranks, key=lambda r: r["gather_route_ms"])
        queries = sum(r["queries"] for r in ranks)
        dg = sum(r["digest"] for r in ranks) & MASK
        routed_b = sum(r["bytes_sent"] for r in ranks) / max(n_rows, 1)
        gather_b = sum(r["gather_bytes_sent"] for r in ranks) / max(n_rows, 1)
        w = {"n_rows": n_rows, "rows_per_rank": [r["n_rows"] for r in ranks],
             "routed": {"wall_ms": slow["wall_ms"], "stages_ms": slow["stages_ms"], "rounds": ranks[0]["rounds"],
                        "chunk": ranks[0]["chunk"], "queries": queries,
                        "local_share": round(sum(r["queries_local"] for r in ranks) / max(queries, 1), 4),
                        "bytes_per_union_row": round(routed_b, 2),
                        "query_bytes_per_union_row": round(sum(r["queries_sent"] for r in ranks) * 8 * nl / max(n_rows, 1), 2),
                        "scratch_bytes_per_own_row": [round(r["scratch_bytes"] / max(r["n_rows"], 1), 1) for r in ranks],
                        "kept_bytes_per_own_row": [round(r["kept_bytes"] / max(r["n_rows"], 1), 1) for r in ranks]},
             "gather": {"route_ms": gslow["gather_route_ms"], "gather_ms": gslow["gather_ms"],
                        "union_links_ms": gslow["union_links_ms"], "bytes_per_union_row": round(gather_b, 2),
                        "scratch_bytes_per_union_row": round(max(r["gather_scratch_bytes"] for r in ranks) / max(n_rows, 1), 1),
                        "kind": "mhmkc_uutigs_ranks: GATHER stage + ms_links of the union (the scratch is that whole call's)"},
             "digest": dg, "table_digest": sum(r["table_digest"] for r in ranks) & MASK,
             "status_entries": [sum(r["status_entries"][i] for r in ranks) for i in range(5)], "single_rank": ref,
             "tables_equal": (sum(r["table_digest"] for r in ranks) & MASK) == ref["table_digest"] and n_rows == ref["n_rows"],
             "digests_equal": dg == ref["digest"] and n_rows == ref["n_rows"],
             "fewer_routed_bytes_than_gather": routed_b < gather_b, "ranks": ranks}
        res["worlds"][str(world)] = w
        print(f"[route_bench] k={args.k} world {world}: routed {slow['wall_ms']} ms, gather route {gslow['gather_route_ms']} ms, "
              f"{n_rows} rows, digests equal: {w['digests_equal']}", file=sys.stderr, flush=True)
    print(json.dumps({key: v for key, v in res.items() if key != "worlds"} |
                     {"worlds": {x: {key: v for key, v in w.items() if key != "ranks"} for x, w in res["worlds"].items()}}))
    bad = [x for x, w in res["worlds"].items() if not (w["digests_equal"] and w["tables_equal"])]
    if bad:  # a failed check writes no profile
        sys.exit(f"route_bench.py: the link sets or the tables differ at k = {args.k}, worlds {', '.join(bad)}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
