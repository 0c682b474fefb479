"""Timing of the hand-over of one contigging round's uutigs to the next k (src/contigging.cpp:93-158) two ways, on the
same box.

  python tools/ctg_chain_bench.py --out profiles/ctg_chain_k21_33.json

Workload: bench.py's C2 (10M synthetic 150 bp reads, genome 50 Mbp, seed 2) counted at --k (21), its uutigs built on the
device (mhmkc_uutigs), then handed to a counter at --k2 (33) that holds the same reads:
  host    mhmkc_uutigs_fetch into host arrays, the depths cut to uint16 (numpy), mhmkc_add_ctgs (the per-character
          conversion into host vectors); the H2D of the converted contigs then happens inside mhmkc_finish (prepare_ctgs).
          No strings are made on the way: this is the least the route through the host can cost.
  device  mhmkc_add_ctgs_from: the contigs are converted from the source counter's device arrays into the next one's.
Per run the hand-over is timed by the wall clock (both; the device route also by device events around the call) and so is
the finish that follows, which for the host route holds the H2D; after --warmup runs, medians of --reps runs. The two
finished tables are compared by an order-free digest over every row (keys, count, extensions).
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


def _mix(x: np.ndarray) -> np.ndarray:
    """splitmix64's finalizer over a uint64 array (wrapping arithmetic)."""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def table_digest(t) -> dict:
    """Order-free: the wrapping sum and the xor of a 64-bit hash of every row."""
    h = np.full(len(t), 0x9E3779B97F4A7C15, dtype=np.uint64)
    for w in range(t.keys.shape[1]):
        h = _mix(h ^ t.keys[:, w])
    h = _mix(h ^ (t.counts.astype(np.uint64) | (t.left.astype(np.uint64) << np.uint64(16)) |
                  (t.right.astype(np.uint64) << np.uint64(24))))
    return {"rows": int(len(t)), "sum": f"{int(h.sum(dtype=np.uint64)):016x}",
            "xor": f"{int(np.bitwise_xor.reduce(h)) if len(t) else 0:016x}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--k2", type=int, default=33)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N
    from mhm2_proxy_amd.build import source_build_id

    if not torch.cuda.is_available():
        sys.exit("ctg_chain_bench.py needs the GPU (no fallback)")
    L = N.lib()
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, args.reads, 150, args.seed, threads=args.threads)
    del genome
    gen_s = time.perf_counter() - t0
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases_in = int(o[-1])
    stream = torch.cuda.Stream(dev)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    res = {}
    with torch.cuda.stream(stream):
        src = m.KmerCounter(args.k, device=0, stream=stream.cuda_stream)
        src.add_tensors(bt, ot, n_bases_in)
        n_out_src = src.finish()
        src.uutigs_device()
        src.synchronize()
        info = src.uutigs_info()
        n_ctgs, n_b = int(info["n_ctgs"]), int(info["n_bases"])
        host = m.KmerCounter(args.k2, device=0, stream=stream.cuda_stream)
        devc = m.KmerCounter(args.k2, device=0, stream=stream.cuda_stream)
        offs = np.empty(n_ctgs + 1, dtype=np.uint64)
        seqs = np.empty(n_b, dtype=np.uint8)
        depths = np.empty(n_ctgs, dtype=np.float64)
        h_fetch, h_conv, h_add, h_total, h_finish = [], [], [], [], []
        d_wall, d_event, d_finish = [], [], []
        for r in range(args.warmup + args.reps):
            # -- the route through the host
            host.reset()
            host.add_tensors(bt, ot, n_bases_in)
            stream.synchronize()
            t0 = time.perf_counter()
            N.check(L.mhmkc_uutigs_fetch(src._h, offs.ctypes.data, seqs.ctypes.data, depths.ctypes.data, None), src._h)
            t1 = time.perf_counter()
            d16 = np.minimum(depths, 65535).astype(np.uint16)
            t2 = time.perf_counter()
            N.check(L.mhmkc_add_ctgs(host._h, C.cast(seqs.ctypes.data, C.c_char_p), offs.ctypes.data, d16.ctypes.data,
                                     n_ctgs), host._h)
            t3 = time.perf_counter()
            n_host = host.finish()
            stream.synchronize()
            t4 = time.perf_counter()
            # -- the device route
            devc.reset()
            devc.add_tensors(bt, ot, n_bases_in)
            stream.synchronize()
            e = [ev(), ev()]
            t5 = time.perf_counter()
            e[0].record(stream)
            devc.add_ctgs_from(src)
            e[1].record(stream)
            t6 = time.perf_counter()
            n_dev = devc.finish()
            stream.synchronize()
            t7 = time.perf_counter()
            if r >= args.warmup:
                h_fetch.append((t1 - t0) * 1e3)
                h_conv.append((t2 - t1) * 1e3)
                h_add.append((t3 - t2) * 1e3)
                h_total.append((t3 - t0) * 1e3)
                h_finish.append((t4 - t3) * 1e3)
                d_wall.append((t6 - t5) * 1e3)
                d_event.append(e[0].elapsed_time(e[1]))
                d_finish.append((t7 - t6) * 1e3)
        torch.cuda.synchronize()
        st_h, st_d = host.stats(), devc.stats()
        dg_h = table_digest(host.fetch())
        dg_d = table_digest(devc.fetch())
    res = {
        "tool": "tools/ctg_chain_bench.py", "build_id": source_build_id(), "k": args.k, "k2": args.k2,
        "workload": f"C2: {args.reads} x 150 bp reads, genome {args.genome} bp, seed {args.seed}",
        "n_out_k": n_out_src, "n_ctgs": n_ctgs, "n_bases": n_b, "n_out_k2": n_dev,
        "ctg_kmers": {"host": st_h["ctg_kmers"], "device": st_d["ctg_kmers"]},
        "reps": args.reps, "warmup": args.warmup,
        "statistic": "median of reps; wall clock around the calls (ms), device events around add_ctgs_from (event_ms)",
        "host_route": {
            "handover_ms": med(h_total), "handover_runs_ms": [round(x, 2) for x in h_total],
            "fetch_ms": med(h_fetch), "depths_ms": med(h_conv), "add_ctgs_ms": med(h_add),
            "finish_ms": med(h_finish), "finish_runs_ms": [round(x, 2) for x in h_finish],
            "handover_plus_finish_ms": med([a + f for a, f in zip(h_total, h_finish)]),
            "kind": "mhmkc_uutigs_fetch + numpy depth cut + mhmkc_add_ctgs; the H2D of the converted contigs is inside finish",
        },
        "device_route": {
            "handover_ms": med(d_wall), "handover_runs_ms": [round(x, 3) for x in d_wall],
            "event_ms": med(d_event), "event_runs_ms": [round(x, 3) for x in d_event],
            "finish_ms": med(d_finish), "finish_runs_ms": [round(x, 2) for x in d_finish],
            "handover_plus_finish_ms": med([a + f for a, f in zip(d_wall, d_finish)]),
            "kind": "mhmkc_add_ctgs_from (one host wait on the mailbox inside the call)",
        },
        "ratio_host_over_device_handover": round(med(h_total) / max(med(d_wall), 1e-6), 1),
        "ratio_host_over_device_handover_plus_finish": round(
            med([a + f for a, f in zip(h_total, h_finish)]) / max(med([a + f for a, f in zip(d_wall, d_finish)]), 1e-6), 2),
        "tables": {"host": dg_h, "device": dg_d, "identical": dg_h == dg_d and n_host == n_dev},
        "synth_seconds": round(gen_s, 2),
    }
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    for c in (host, devc, src):
        c.close()
    if not res["tables"]["identical"]:
        sys.exit("the two routes' tables differ")


if __name__ == "__main__":
    main()
