"""The fragment build (mhmkc_uutigs_frags) beside the replicated build (mhmkc_uutigs_ranks, §3.12b)
with 2 and 4 ranks on one MI355X: what each moves and holds, and how long each takes.

  python tools/uutig_frags_bench.py --k 21 --out profiles/uutig_frags_k21.json
  python tools/uutig_frags_bench.py --k 63 --out profiles/uutig_frags_k63.json

Workload and setting as tools/uutig_ranks_bench.py: bench.py's C2 generator (150 bp reads of a 50 Mbp genome, seed 2),
--reads-per-rank reads per rank (rank r takes reads [r R, (r + 1) R)), counted at --k with MHMKC_OWNER_MINIMIZER. The
ranks are processes that SHARE ONE GPU and exchange over gloo through host memory, so the times show the mechanism only;
the bytes moved, the scratch and the fragment counts are what the run is for.

Every run counts the rank's shard on two handles and builds the uutigs twice: mhmkc_uutigs_ranks on one handle,
mhmkc_uutigs_frags (routed links included) on the other, each timed by the wall clock around the call after a barrier
and by the library's stage events; --warmup runs, then the median of --reps, the slowest rank. The two builds' fetched
contig arrays (offsets, bases, depths, n_kmers: blake2b of their bytes) and row maps (an order-free sum of a hash of
every row's key and place) are compared per rank by digest on the host, in numpy: the tool exits non-zero and writes
nothing unless they are equal on every rank.
"""
from __future__ import annotations

import argparse
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


def med(xs):
    return round(statistics.median(xs), 3)


_C1 = np.uint64(0x9E3779B97F4A7C15)


def _mix(h, v):
    """One multiply-xorshift step in wrapping uint64 arithmetic (as tools/route_bench.py)."""
    h = (h ^ v) * _C1
    return h ^ (h >> np.uint64(31))


def digest(c, k: int) -> str:
    """blake2b over the bytes of the contig arrays a counter's kept build gives, and the wrapping sum over its rows of a
    hash of (key words, row_ctg, row_pos, row_rc): the row map by key, since two handles may hold their rows in another
    order. Numpy on the host."""
    h = hashlib.blake2b(digest_size=16)
    for a in c.uutigs():
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype} {a.shape}".encode())
        h.update(a.tobytes())
    t = c.fetch()
    row_ctg, row_pos, row_rc = c.uutig_rows()
    with np.errstate(over="ignore"):
        x = np.full(len(t), 0x9E3779B97F4A7C15, dtype=np.uint64)
        for w in range(k // 32 + 1):
            x = _mix(x, t.keys[:, w])
        x = _mix(x, row_ctg.astype(np.uint64) << np.uint64(32) | row_pos.astype(np.uint64))
        x = _mix(x, row_rc.astype(np.uint64))
        rows = int(x.sum(dtype=np.uint64))
    return f"{h.hexdigest()} {len(t)} {rows:016x}"


def worker(rank: int, world: int, port: int, args, out_dir: str):
    import torch
    import torch.distributed as dist

    import mhm2_proxy_amd as m

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    k, R, dev = args.k, args.reads_per_rank, torch.device("cuda", 0)
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, R, 150, args.seed, first_read=rank * R, threads=max(1, args.threads // world))
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases_in = int(o[-1])
    del b, o, genome

    def counter():
        return m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                             output_owner=m.MHMKC_OWNER_MINIMIZER)

    rep, frg = counter(), counter()
    wall = {"ranks": [], "frags": []}
    infos = {"ranks": [], "frags": [], "route": []}
    res = {}
    for r in range(args.warmup + args.reps):
        for name, c, build, info in (("ranks", rep, rep.uutigs_ranks, rep.uutigs_ranks_info),
                                     ("frags", frg, frg.uutigs_frags, frg.uutigs_frags_info)):
            c.reset()
            c.add_tensors(bt, ot, n_bases_in)
            c.finish()
            dist.barrier()
            t0 = time.perf_counter()
            res[name] = build()
            t1 = time.perf_counter()
            if r >= args.warmup:
                wall[name].append((t1 - t0) * 1e3)
                infos[name].append(info())
                if name == "frags":
                    infos["route"].append(c.route_info())
    dg = {"ranks": digest(rep, k), "frags": digest(frg, k)}
    n_rows = rep.uutigs_device()["n_out"]
    ri, fi, li = infos["ranks"][-1], infos["frags"][-1], infos["route"][-1]
    out = {"rank": rank, "n_rows": int(n_rows), "ids_equal": res["ranks"] == res["frags"], "digest": dg,
           "n_ctgs": res["frags"]["n_ctgs"], "n_ctgs_all": res["frags"]["n_ctgs_all"],
           "replicated": {"wall_ms": med(wall["ranks"]), "wall_runs_ms": [round(x, 1) for x in wall["ranks"]],
                          "stages_ms": {s: med([i["ms_stage"][s] for i in infos["ranks"]]) for s in ri["ms_stage"]},
                          "bytes_sent": sum(ri["routed_bytes_sent"].values()), "scratch_bytes": ri["scratch_bytes"],
                          "kept_bytes": ri["kept_bytes"]},
           "fragments": {"wall_ms": med(wall["frags"]), "wall_runs_ms": [round(x, 1) for x in wall["frags"]],
                         "stages_ms": {s: med([i["ms_stage"][s] for i in infos["frags"]]) for s in fi["ms_stage"]},
                         "ms_total": med([i["ms_total"] for i in infos["frags"]]),
                         "links_ms": med([i["ms_total"] for i in infos["route"]]), "links_built": fi["links_built"],
                         "links_bytes_sent": li["bytes_sent"], "links_scratch_bytes": li["scratch_bytes"],
                         "bytes_sent": fi["bytes_sent"], "records_sent": fi["records_sent"],
                         "scratch_bytes": fi["scratch_bytes"], "kept_bytes": fi["kept_bytes"],
                         **{key: fi[key] for key in ("frags_open", "frags_open_all", "frags_closed", "local_cycles",
                                                     "cross_links", "ctgs_cross_all", "ctgs_cross_mine", "cycles_cross_all",
                                                     "rounds_local", "cycle_rounds_local", "rounds_frags",
                                                     "cycle_rounds_frags")}}}
    rep.close()
    frg.close()
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(out))
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
        sys.exit("uutig_frags_bench.py needs the GPU (no fallback)")
    res = {"tool": "tools/uutig_frags_bench.py", "build_id": source_build_id(), "k": args.k,
           "workload": f"C2's generator: {args.reads_per_rank} x 150 bp reads per rank, genome {args.genome} bp, seed {args.seed}",
           "setting": "the ranks are processes sharing ONE MI355X, exchanging over gloo through host memory: the mechanism "
                      "and the byte counts, not xGMI speed",
           "reps": args.reps, "warmup": args.warmup,
           "statistic": "median over reps; per world the slowest rank's wall clock around each build after a barrier; stage "
                        "times from device events (mhmkc_uutigs_ranks_info, mhmkc_uutigs_frags_info); the fragment build's "
                        "wall clock includes the routed links (mhmkc_route_info) it builds first", "worlds": {}}
    for world in [int(x) for x in args.worlds.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(worker, args=(world, free_port(), args, d), nprocs=world, join=True)
            ranks = [json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(world)]
        bad = [r["rank"] for r in ranks if r["digest"]["ranks"] != r["digest"]["frags"] or not r["ids_equal"]]
        if bad:
            sys.exit(f"uutig_frags_bench.py: world {world}: the two builds differ on ranks {bad}; nothing written")
        n_rows = sum(r["n_rows"] for r in ranks)
        slow_r = max(ranks, key=lambda r: r["replicated"]["wall_ms"])["replicated"]
        slow_f = max(ranks, key=lambda r: r["fragments"]["wall_ms"])["fragments"]
        f_moved = sum(sum(r["fragments"]["bytes_sent"].values()) for r in ranks)
        l_moved = sum(r["fragments"]["links_bytes_sent"] for r in ranks)
        r_moved = sum(r["replicated"]["bytes_sent"] for r in ranks)
        opens = ranks[0]["fragments"]["frags_open_all"]
        w = {"n_rows": n_rows, "n_ctgs_all": ranks[0]["n_ctgs_all"], "rows_per_rank": [r["n_rows"] for r in ranks],
             "digests_equal": True,
             "replicated": {"wall_ms": slow_r["wall_ms"], "stages_ms": slow_r["stages_ms"],
                            "moved_bytes_per_union_row": round(r_moved / max(n_rows, 1), 2),
                            "scratch_bytes_per_rank": [r["replicated"]["scratch_bytes"] for r in ranks]},
             "fragments": {"wall_ms": slow_f["wall_ms"], "stages_ms": slow_f["stages_ms"], "links_ms": slow_f["links_ms"],
                           "moved_bytes_per_union_row": round(f_moved / max(n_rows, 1), 2),
                           "moved_bytes_per_union_row_with_links": round((f_moved + l_moved) / max(n_rows, 1), 2),
                           "moved_bytes_by_stage": {s: sum(r["fragments"]["bytes_sent"][s] for r in ranks)
                                                    for s in ranks[0]["fragments"]["bytes_sent"]},
                           "scratch_bytes_per_rank": [r["fragments"]["scratch_bytes"] for r in ranks],
                           "links_scratch_bytes_per_rank": [r["fragments"]["links_scratch_bytes"] for r in ranks],
                           "frags_open_all": opens, "frags_open_share_of_rows": round(opens / max(n_rows, 1), 4),
                           "frags_open_per_rank": [r["fragments"]["frags_open"] for r in ranks],
                           "frags_closed_per_rank": [r["fragments"]["frags_closed"] for r in ranks],
                           "cross_links_per_rank": [r["fragments"]["cross_links"] for r in ranks],
                           "ctgs_cross_all": ranks[0]["fragments"]["ctgs_cross_all"],
                           "cycles_cross_all": ranks[0]["fragments"]["cycles_cross_all"],
                           "rounds_local": [r["fragments"]["rounds_local"] for r in ranks],
                           "rounds_frags": ranks[0]["fragments"]["rounds_frags"]},
             "scratch_ratio_replicated_over_fragments": round(
                 max(r["replicated"]["scratch_bytes"] for r in ranks) / max(1, max(r["fragments"]["scratch_bytes"] for r in ranks)), 2),
             "ranks": ranks}
        res["worlds"][str(world)] = w
        print(f"[uutig_frags_bench] k={args.k} world {world}: replicated {slow_r['wall_ms']} ms, fragments {slow_f['wall_ms']} ms, "
              f"{n_rows} rows, {opens} open fragments", file=sys.stderr, flush=True)
    print(json.dumps({key: v for key, v in res.items() if key != "worlds"} |
                     {"worlds": {x: {key: v for key, v in w.items() if key != "ranks"} for x, w in res["worlds"].items()}}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
