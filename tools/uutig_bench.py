"""Timing of the device traversal (mhmkc_uutigs: the finished table's de Bruijn links turned into the round's uutigs on
the GPU) against the route that exists without it.

  python tools/uutig_bench.py --k 21 --out profiles/uutig_bench_k21.json
  python tools/uutig_bench.py --k 63 --out profiles/uutig_bench_k63.json

Workload: bench.py's C2 (10M synthetic 150 bp reads, genome 50 Mbp, seed 2) counted at --k. Every run counts the reads
again (the uutigs are built once per finish), builds the index and the links, and then times
  (a) links -> uutigs (mhmkc_uutigs) with device events on the counter's stream (the counter is created on a torch
      stream), and the library's own stage events (mhmkc_uutigs_info: port successors, ranking rounds one by one,
      cycles, contig table, row map + bases),
  (b) the fetch of the contig arrays to the host (mhmkc_uutigs_fetch, wall clock),
after --warmup runs, as the median of --reps runs. The comparison, on the same box, is the hand-off of the table into
the C++ adapter's KmerMap (load_ordered, what bench.py --full reports as `kmermap`) plus mhm2::traverse_debruijn_graph
on one thread (tools/cpp/uutig_host.cpp). The host traversal takes seconds to minutes at this size and is run ONCE, not
--reps times (--no-host skips it). The two routes' contig lists are compared in the tool: contig by contig in id order
(sequence, strand, depth bits) and as an order-free digest of canonical sequences and depths.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N
    from mhm2_proxy_amd.build import UHOST, source_build_id

    if not torch.cuda.is_available():
        sys.exit("uutig_bench.py needs the GPU (no fallback)")
    k, dev = args.k, torch.device("cuda", 0)
    t0 = time.perf_counter()
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, args.reads, 150, args.seed, threads=args.threads)
    del genome
    gen_s = time.perf_counter() - t0
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases_in = int(o[-1])
    stream = torch.cuda.Stream(dev)
    counter = m.KmerCounter(k, device=0, stream=stream.cuda_stream)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    runs, infos, fetch_ms = [], [], []
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.reps):
            counter.reset()
            counter.add_tensors(bt, ot, n_bases_in)
            n_out = counter.finish()
            counter.dbjg_links_device()  # index + links
            before = counter.stats()
            e = [ev(), ev()]
            e[0].record(stream)
            counter.uutigs_device()
            e[1].record(stream)
            counter.synchronize()
            t1 = time.perf_counter()
            offsets, seqs, depths, n_kmers = counter.uutigs()
            t2 = time.perf_counter()
            if r >= args.warmup:
                runs.append(e[0].elapsed_time(e[1]))
                infos.append(counter.uutigs_info())
                fetch_ms.append((t2 - t1) * 1e3)
        torch.cuda.synchronize()
        after = counter.stats()
    info = infos[-1]
    n_ctgs, n_b = int(info["n_ctgs"]), int(info["n_bases"])
    stages = {s: med([i[s] for i in infos]) for s in ("ms_succ", "ms_rank", "ms_cycles", "ms_table", "ms_rows", "ms_total")}
    rounds = int(info["rounds"])
    per_round = [med([i["ms_round"][x] for i in infos]) for x in range(min(rounds, len(info["ms_round"])))]
    res = {
        "tool": "tools/uutig_bench.py", "build_id": source_build_id(), "k": k,
        "workload": f"C2: {args.reads} x 150 bp reads, genome {args.genome} bp, seed {args.seed}",
        "n_out": n_out, "n_ctgs": n_ctgs, "n_bases": n_b, "longest_ctg_kmers": int(n_kmers.max()) if n_ctgs else 0,
        "reps": args.reps, "warmup": args.warmup,
        "statistic": "median; device events on the counter's stream (uutigs_ms, stages), wall clock (fetch_ms)",
        "device": {
            "uutigs_ms": med(runs), "uutigs_runs_ms": [round(x, 3) for x in runs],
            "stages_ms": stages, "rounds": rounds, "round_ms": per_round,
            "cycle_ports": int(info["cycle_ports"]), "cycle_rounds": int(info["cycle_rounds"]),
            "fetch_ms": med(fetch_ms), "fetch_runs_ms": [round(x, 1) for x in fetch_ms],
            "fetch_bytes": int(offsets.nbytes + seqs.nbytes + depths.nbytes + n_kmers.nbytes),
            "scratch_bytes": int(info["scratch_bytes"]), "scratch_bytes_per_row": round(info["scratch_bytes"] / max(n_out, 1), 1),
            "kept_bytes": int(info["kept_bytes"]), "kept_bytes_per_row": round(info["kept_bytes"] / max(n_out, 1), 1),
            "device_bytes_before": before["device_bytes"], "device_bytes_after": after["device_bytes"],
            "device_bytes_peak": after["device_bytes_peak"],
        },
        "host_route": None, "synth_seconds": round(gen_s, 2),
    }
    if UHOST.exists():
        lib = C.CDLL(str(UHOST))
        if lib.mhmkc_uhost_abi() == N.lib().mhmkc_abi_version():
            lib.mhmkc_uhost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
            ms = (C.c_double * 4)()
            v = (C.c_uint64 * 8)()
            if lib.mhmkc_uhost(counter._h, k, args.threads, 0 if args.no_host else 1, ms, v) != 0:
                sys.exit("mhmkc_uhost failed")
            res["host_route"] = {
                "handoff_ms": round(ms[0], 1), "traverse_ms": round(ms[2], 1), "traverse_runs": 0 if args.no_host else 1,
                "traverse_table_ms": round(ms[1], 1), "n_ctgs": int(v[0]), "n_bases": int(v[1]),
                "kind": f"load_ordered into KmerMap<MAX_K> with {args.threads} threads (one run), then "
                        "mhm2::traverse_debruijn_graph on one thread, RUN ONCE (it takes this long); traverse_table_ms is "
                        "the fetch + fill of the traversal's own table and is not counted",
            }
            if not args.no_host:
                res["identical"] = {
                    "digest_host": f"{int(v[2]):016x}", "digest_device": f"{int(v[5]):016x}",
                    "digests_equal": int(v[2]) == int(v[5]) and int(v[0]) == int(v[3]) and int(v[1]) == int(v[4]),
                    "equal_in_order_strand_depth": int(v[6]), "equal_as_other_strand": int(v[7]), "of": int(v[3]),
                }
                d = res["device"]
                host_ms = ms[0] + ms[2]
                res["comparison"] = {
                    "device_ms_uutigs": d["uutigs_ms"], "device_ms_uutigs_plus_fetch": round(d["uutigs_ms"] + d["fetch_ms"], 3),
                    "host_ms_handoff_plus_traverse": round(host_ms, 1),
                    "ratio_host_over_device": round(host_ms / d["uutigs_ms"], 1),
                    "ratio_host_over_device_with_fetch": round(host_ms / (d["uutigs_ms"] + d["fetch_ms"]), 1),
                }
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    counter.close()


if __name__ == "__main__":
    main()
