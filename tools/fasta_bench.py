"""Timing of the assembly statistics and the FASTA output from device-resident contigs (mhmkc_uutigs_stats,
mhmkc_uutigs_fasta, mhmkc_fasta_fetch, mhmkc_fasta_write) against the route that exists without them.

  python tools/fasta_bench.py --k 21 --out profiles/fasta_bench_k21.json
  python tools/fasta_bench.py --k 21 --worlds 2,4 --out profiles/fasta_bench_k21_ranks.json

One rank. Workload: bench.py's C2 (10M synthetic 150 bp reads, genome 50 Mbp, seed 2) counted at --k, its uutigs built
once. Then, --warmup runs and the median of --reps:
  stats_ms            wall clock around uutigs_stats(min_ctg_len) (the call waits for its figures);
  text stages         the library's device events (mhmkc_fasta_info: table = checks + lengths + scan, copy = the bases,
                      headers) and the wall clock around uutigs_fasta();
  fetch_ms            fasta_bytes(): the text into pageable host memory;
  write_ms            fasta_write() into a file on tmpfs (--dir, default /dev/shm);
  d2d_ms              a device-to-device copy of the same byte count (torch, device events): what one read and one write
                      per byte cost at least.
The host route, ONE run on one thread (tools/cpp/fasta_host.cpp): mhmkc_uutigs_fetch, a Contig with its std::string per
contig, the adapter's dump_contigs into a second tmpfs file and ctg_stats. The tool compares the two files byte for byte
and the figures (integers equal, tot_depth within n 2^-52 sum|d|); it exits non-zero and writes nothing if they differ.

--worlds: the same calls on 2 and 4 ranks, processes that SHARE ONE GPU and exchange over gloo, --reads-per-rank reads
each, after uutigs_frags(): the slowest rank's wall clock per call after a barrier, all ranks writing one tmpfs file;
every rank reads its block of the file back and compares it with its kept text.
"""
from __future__ import annotations

import argparse
import ctypes as C
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


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def one_rank(args):
    import torch

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N
    from mhm2_proxy_amd.build import FHOST, source_build_id

    k, dev, mn = args.k, torch.device("cuda", 0), args.min_ctg_len
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, args.reads, 150, args.seed, threads=args.threads)
    del genome
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    c = m.KmerCounter(k, device=0)
    c.add_tensors(bt, ot, int(o[-1]))
    n_out = c.finish()
    ud = c.uutigs_device()
    c.synchronize()
    dev_path, host_path = Path(args.dir) / f"fasta_bench_device_{os.getpid()}.fasta", Path(args.dir) / f"fasta_bench_host_{os.getpid()}.fasta"
    t = {key: [] for key in ("stats", "text_wall", "table", "copy", "headers", "text_total", "fetch", "write", "d2d")}
    try:
        for r in range(args.warmup + args.reps):
            st, ms_stats = timed(lambda: c.uutigs_stats(mn))
            fa, ms_text = timed(lambda: c.uutigs_fasta(mn))
            info = c.fasta_info()
            text, ms_fetch = timed(c.fasta_bytes)
            _, ms_write = timed(lambda: c.fasta_write(dev_path))
            src = c.fasta_tensor()
            dst = torch.empty_like(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                for key, v in (("stats", ms_stats), ("text_wall", ms_text), ("table", info["ms_table"]), ("copy", info["ms_copy"]),
                               ("headers", info["ms_headers"]), ("text_total", info["ms_total"]), ("fetch", ms_fetch),
                               ("write", ms_write), ("d2d", e0.elapsed_time(e1))):
                    t[key].append(v)
            del src, dst
        if not FHOST.exists():
            sys.exit("fasta_bench.py: tools/bin/libmhmkc_fhost.so is missing: python -m mhm2_proxy_amd.build")
        lib = C.CDLL(str(FHOST))
        if lib.mhmkc_fhost_abi() != N.lib().mhmkc_abi_version():
            sys.exit("fasta_bench.py: libmhmkc_fhost.so is of another ABI version")
        lib.mhmkc_fhost.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_double), C.POINTER(N.MhmkcCtgStats)]
        ms, hst = (C.c_double * 4)(), N.MhmkcCtgStats()
        if lib.mhmkc_fhost(c._h, mn, os.fsencode(host_path), ms, C.byref(hst)) != 0:
            sys.exit("mhmkc_fhost failed")
        host = hst.as_dict()
        files_equal = dev_path.read_bytes() == host_path.read_bytes() == text
        _, _, depths, _ = c.uutigs()
        ints_equal = all(st["all"][f] == host[f] for f in ("n_ctgs", "tot_len", "max_len", "n_ns", "len_sums", "n50", "l50"))
        bound = len(depths) * 2.0**-52 * float(np.abs(depths).sum())
        depth_close = abs(st["all"]["tot_depth"] - host["tot_depth"]) <= bound
        if not (files_equal and ints_equal and depth_close):
            sys.exit(f"fasta_bench.py: the two routes differ (files {files_equal}, integers {ints_equal}, depth {depth_close}); "
                     "nothing written")
    finally:
        for p in (dev_path, host_path):
            if p.exists():
                p.unlink()
    d = {key: med(v) for key, v in t.items()}
    nbytes = fa["n_bytes"]
    host_ms = ms[0] + ms[1] + ms[2] + ms[3]
    dev_ms = d["stats"] + d["text_wall"] + d["write"]
    res = {
        "tool": "tools/fasta_bench.py", "build_id": source_build_id(), "k": k, "min_ctg_len": mn,
        "workload": f"C2: {args.reads} x 150 bp reads, genome {args.genome} bp, seed {args.seed}",
        "n_out": n_out, "n_ctgs": ud["n_ctgs"], "n_bases": ud["n_bases"], "n_written": info["n_written"], "text_bytes": nbytes,
        "reps": args.reps, "warmup": args.warmup, "dir": str(args.dir),
        "statistic": "median; wall clock (stats_ms, text_wall_ms, fetch_ms, write_ms), device events (stages, d2d_ms); the "
                     "host route is one run",
        "device": {"stats_ms": d["stats"], "text_wall_ms": d["text_wall"],
                   "text_stages_ms": {"table": d["table"], "copy": d["copy"], "headers": d["headers"], "total": d["text_total"]},
                   "fetch_ms": d["fetch"], "write_ms": d["write"], "d2d_ms": d["d2d"],
                   "copy_GBps_read_plus_write": round(2 * nbytes / max(d["copy"], 1e-6) / 1e6, 1),
                   "d2d_GBps_read_plus_write": round(2 * nbytes / max(d["d2d"], 1e-6) / 1e6, 1),
                   "text_device_bytes": info["text_bytes"], "scratch_bytes": info["scratch_bytes"]},
        "host_route": {"fetch_ms": round(ms[0], 2), "contig_objects_ms": round(ms[1], 2), "dump_contigs_ms": round(ms[2], 2),
                       "ctg_stats_ms": round(ms[3], 2), "total_ms": round(host_ms, 2), "runs": 1,
                       "kind": "mhmkc_uutigs_fetch, a Contig with its std::string per contig, mhm2::dump_contigs into a tmpfs "
                               "file and mhm2::ctg_stats, one thread"},
        "identical": {"files_equal": files_equal, "integer_figures_equal": ints_equal, "tot_depth_within_bound": depth_close,
                      "tot_depth_device": st["all"]["tot_depth"], "tot_depth_host": host["tot_depth"]},
        "stats": st["all"],
        "comparison": {"device_ms_stats_text_write": round(dev_ms, 3), "host_ms_total": round(host_ms, 2),
                       "ratio_host_over_device": round(host_ms / max(dev_ms, 1e-9), 1),
                       "ratio_base_copy_over_d2d": round(d["copy"] / max(d["d2d"], 1e-9), 2),
                       "ratio_text_total_over_d2d": round(d["text_total"] / max(d["d2d"], 1e-9), 2)},
    }
    c.close()
    return res


def worker(rank: int, world: int, port: int, args, out_dir: str):
    import torch
    import torch.distributed as dist

    import mhm2_proxy_amd as m

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    k, R, dev, mn = args.k, args.reads_per_rank, torch.device("cuda", 0), args.min_ctg_len
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, R, 150, args.seed, first_read=rank * R, threads=max(1, args.threads // world))
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    c = m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                      output_owner=m.MHMKC_OWNER_MINIMIZER)
    c.add_tensors(bt, ot, int(o[-1]))
    c.finish()
    r = c.uutigs_frags()
    path = Path(out_dir) / "all_ranks.fasta"
    t = {"stats": [], "text": [], "write": []}
    for i in range(args.warmup + args.reps):
        dist.barrier()
        st, a = timed(lambda: c.uutigs_stats(mn))
        dist.barrier()
        fa, bms = timed(lambda: c.uutigs_fasta(mn))
        dist.barrier()
        _, w = timed(lambda: c.fasta_write(path))
        if i >= args.warmup:
            t["stats"].append(a), t["text"].append(bms), t["write"].append(w)
    text = c.fasta_bytes()
    with open(path, "rb") as f:
        f.seek(fa["file_offset"])
        block_equal = f.read(len(text)) == text
    out = {"rank": rank, "n_ctgs": r["n_ctgs"], "n_ctgs_all": r["n_ctgs_all"], "first_id": r["first_id"], **fa,
           "block_equal": block_equal, "file_bytes": path.stat().st_size, "stats_all": st["all"],
           "stats_ms": med(t["stats"]), "text_ms": med(t["text"]), "write_ms": med(t["write"]), "info": c.fasta_info()}
    c.close()
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reads-per-rank", type=int, default=1_000_000)
    ap.add_argument("--worlds", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--min-ctg-len", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm" if Path("/dev/shm").is_dir() else tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from mhm2_proxy_amd.build import source_build_id

    if not torch.cuda.is_available():
        sys.exit("fasta_bench.py needs the GPU (no fallback)")
    if not args.worlds:
        res = one_rank(args)
        print(json.dumps({key: v for key, v in res.items() if key != "stats"}))
    else:
        import torch.multiprocessing as mp

        res = {"tool": "tools/fasta_bench.py", "build_id": source_build_id(), "k": args.k, "min_ctg_len": args.min_ctg_len,
               "workload": f"C2's generator: {args.reads_per_rank} x 150 bp reads per rank, genome {args.genome} bp, seed {args.seed}",
               "setting": "the ranks are processes sharing ONE MI355X, exchanging over gloo through host memory, writing one "
                          "tmpfs file: the mechanism, not xGMI or file-system speed",
               "reps": args.reps, "warmup": args.warmup,
               "statistic": "median over reps; per world the slowest rank's wall clock around each call after a barrier",
               "worlds": {}}
        for world in [int(x) for x in args.worlds.split(",")]:
            with tempfile.TemporaryDirectory(dir=args.dir) as d:
                mp.spawn(worker, args=(world, free_port(), args, d), nprocs=world, join=True)
                ranks = [json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(world)]
            ok = (all(r["block_equal"] for r in ranks) and all(r["stats_all"] == ranks[0]["stats_all"] for r in ranks)
                  and all(r["file_bytes"] == r["n_bytes_all"] == sum(x["n_bytes"] for x in ranks) for r in ranks))
            if not ok:
                sys.exit(f"fasta_bench.py: world {world}: a rank's block or the figures differ; nothing written")
            res["worlds"][str(world)] = {
                "n_ctgs_all": ranks[0]["n_ctgs_all"], "file_bytes": ranks[0]["file_bytes"], "blocks_equal": True,
                "figures_equal_on_all_ranks": True, "bytes_per_rank": [r["n_bytes"] for r in ranks],
                "stats_ms": max(r["stats_ms"] for r in ranks), "text_ms": max(r["text_ms"] for r in ranks),
                "write_ms": max(r["write_ms"] for r in ranks), "stats_all": ranks[0]["stats_all"], "ranks": ranks}
            w = res["worlds"][str(world)]
            print(f"[fasta_bench] k={args.k} world {world}: stats {w['stats_ms']} ms, text {w['text_ms']} ms, write "
                  f"{w['write_ms']} ms, {w['file_bytes']} bytes", file=sys.stderr, flush=True)
        print(json.dumps({key: v for key, v in res.items() if key != "worlds"} |
                         {"worlds": {x: {key: v for key, v in w.items() if key != "ranks"} for x, w in res["worlds"].items()}}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
