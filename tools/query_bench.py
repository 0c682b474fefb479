"""Timing of the device queries on the finished table (mhmkc_lookup_device, mhmkc_dbjg_links_device) against the route
that exists without them.

  python tools/query_bench.py --k 21 --out profiles/query_bench_k21.json
  python tools/query_bench.py --k 63 --out profiles/query_bench_k63.json

Workload: bench.py's C2 (10M synthetic 150 bp reads, genome 50 Mbp, seed 2) counted at --k. After the finish it times
  (a) the build of the query index (the first query after a finish; measured as a one-key lookup),
  (b) lookup_tensors of --queries keys (default 50M): half table keys drawn at random, a quarter reverse complements
      of table keys, a quarter one-base mutants of table keys, shuffled; canonicalize=True,
  (c) dbjg_links (both directions of every row),
each with device events on the counter's stream (the counter is created on a torch stream), after warm-ups, as the
median of --reps runs. (a) and (c) happen once per finish, so every one of their runs counts the reads again first.
The comparison is the hand-off of the table into the C++ adapter's KmerMap (what bench.py --full reports as
`kmermap`) plus KmerMap::find on the same keys with --threads host threads (tools/cpp/query_find.cpp). The host side
is handed the canonical form of the table-key and reverse-complement queries and the mutants as they are, so it pays
for no canonicalisation; its hit count may therefore differ from the device's by the mutants whose reverse complement
is a table key.
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

M64 = (1 << 64) - 1


def _s64(v: int) -> int:
    """A 64-bit pattern as the int64 that torch holds it in."""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _lsr(x, s: int):
    """Logical right shift of int64 words."""
    if s == 0:
        return x
    return (x >> s) & _s64((1 << (64 - s)) - 1)


def _rev2(x):
    """Reverse the 32 two-bit groups of every int64 word (kmer_ops.hpp rev2)."""
    import torch

    x = x.contiguous().view(torch.uint8).reshape(-1, 8).flip(1).contiguous().view(torch.int64).reshape(x.shape)
    x = (_lsr(x, 4) & _s64(0x0F0F0F0F0F0F0F0F)) | ((x & _s64(0x0F0F0F0F0F0F0F0F)) << 4)
    return (_lsr(x, 2) & _s64(0x3333333333333333)) | ((x & _s64(0x3333333333333333)) << 2)


def revcomp_t(keys, k: int):
    """Kmer::revcomp of an (n, nl) int64 tensor of keys (kmer_ops.hpp revcomp), on the tensor's device."""
    import torch

    nl = keys.shape[1]
    t = [_rev2(~keys[:, nl - 1 - i]) for i in range(nl)]
    sh = 2 * (32 * nl - k)
    out = []
    for i in range(nl):
        v = t[i] << sh
        if i + 1 < nl:
            v = v | _lsr(t[i + 1], 64 - sh)
        out.append(v)
    kl = k - 32 * (nl - 1)
    out[-1] = out[-1] & _s64(M64 ^ ((1 << (64 - 2 * kl)) - 1))
    return torch.stack(out, dim=1)


def mutate_t(keys, k: int, gen):
    """Every key with one base at a random position changed."""
    import torch

    n, nl = keys.shape
    pos = torch.randint(0, k, (n,), device=keys.device, generator=gen)
    delta = torch.randint(1, 4, (n,), device=keys.device, generator=gen)
    shift = 2 * (31 - pos % 32)
    out = keys.clone()
    for w in range(nl):
        out[:, w] = torch.where(pos // 32 == w, out[:, w] ^ (delta << shift), out[:, w])
    return out


def median_ms(pairs):
    return round(statistics.median(a.elapsed_time(b) for a, b in pairs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--queries", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    import torch

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N
    from mhm2_proxy_amd.build import QFIND, source_build_id

    if not torch.cuda.is_available():
        sys.exit("query_bench.py needs the GPU (no fallback)")
    k, dev = args.k, torch.device("cuda", 0)
    nl = k // 32 + 1
    t0 = time.perf_counter()
    genome = m.synth_genome(args.genome, args.seed)
    b, o = m.synth_reads(genome, args.reads, 150, args.seed, threads=args.threads)
    del genome
    gen_s = time.perf_counter() - t0
    bt = torch.from_numpy(b).to(dev)
    ot = torch.from_numpy(o.view(np.int64)).to(dev)
    n_bases = int(o[-1])
    stream = torch.cuda.Stream(dev)
    counter = m.KmerCounter(k, device=0, stream=stream.cuda_stream)

    def count():
        counter.reset()
        counter.add_tensors(bt, ot, n_bases)
        return counter.finish()

    def ev():
        return torch.cuda.Event(enable_timing=True)

    one = torch.zeros(nl, dtype=torch.int64, device=dev)
    build, links = [], []
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.reps):
            n_out = count()
            e = [ev(), ev(), ev()]
            e[0].record(stream)
            counter.lookup_tensors(one, sync=False)  # the first query after a finish builds the index
            e[1].record(stream)
            counter.dbjg_links_device()
            e[2].record(stream)
            counter.synchronize()
            if r >= args.warmup:
                build.append((e[0], e[1]))
                links.append((e[1], e[2]))
        torch.cuda.synchronize()
        st = counter.stats()
        bytes_before = st["device_bytes"]  # (with the index and the links)

        # the queries, made on the device from the table itself
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        out = counter.device_output()

        class Dev:
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2}

        table = torch.as_tensor(Dev(out["keys"], n_out * nl), device=dev).reshape(n_out, nl)
        nq = args.queries
        n_hit, n_rc = nq // 2, nq // 4
        n_mut = nq - n_hit - n_rc
        hit_keys = table[torch.randint(0, n_out, (n_hit,), device=dev, generator=gen)]
        rc_src = table[torch.randint(0, n_out, (n_rc,), device=dev, generator=gen)]
        mut_keys = mutate_t(table[torch.randint(0, n_out, (n_mut,), device=dev, generator=gen)], k, gen)
        perm = torch.randperm(nq, device=dev, generator=gen)
        q_dev = torch.cat([hit_keys, revcomp_t(rc_src, k), mut_keys])[perm].contiguous()
        q_host = torch.cat([hit_keys, rc_src, mut_keys])[perm].contiguous()  # the host route's keys (canonical hits)
        del hit_keys, rc_src, mut_keys, perm
        torch.cuda.synchronize()

        look = []
        for r in range(args.warmup + args.reps):
            e = [ev(), ev()]
            e[0].record(stream)
            rows, counts, left, right = counter.lookup_tensors(q_dev, canonicalize=True, sync=False)
            e[1].record(stream)
            counter.synchronize()
            if r >= args.warmup:
                look.append((e[0], e[1]))
        torch.cuda.synchronize()
        dev_hits = int((rows != -1).sum())
        st2 = counter.stats()

    # the host route: hand-off into a KmerMap, then find with 16 threads
    host = None
    if QFIND.exists():
        lib = C.CDLL(str(QFIND))
        if lib.mhmkc_qfind_abi() == N.lib().mhmkc_abi_version():
            qh = q_host.cpu().numpy().view(np.uint64)
            lib.mhmkc_qfind.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_int,
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
            handoffs, finds, hits = [], None, C.c_uint64(0)
            for r in range(3):  # (every call fills a fresh map; the first includes the device sort)
                hm = C.c_double(0)
                fm = (C.c_double * args.reps)()
                if lib.mhmkc_qfind(counter._h, k, args.threads, qh.ctypes.data, nq, args.reps if r == 2 else 1,
                                   C.byref(hm), fm, C.byref(hits)) != 0:
                    sys.exit("mhmkc_qfind failed")
                handoffs.append(hm.value)
                finds = list(fm)
            host = {"handoff_ms": round(statistics.median(handoffs), 1), "handoff_runs_ms": [round(x, 1) for x in handoffs],
                    "find_ms": round(statistics.median(finds), 1), "find_runs_ms": [round(x, 1) for x in finds],
                    "find_threads": args.threads, "hits": int(hits.value),
                    "kind": "load_ordered into KmerMap<MAX_K> (median of 3), then KmerMap::find per key over "
                            f"{args.threads} threads (median of {args.reps}); canonical hit keys, no canonicalisation"}
    res = {
        "tool": "tools/query_bench.py", "build_id": source_build_id(), "k": k,
        "workload": f"C2: {args.reads} x 150 bp reads, genome {args.genome} bp, seed {args.seed}",
        "n_out": n_out, "queries": nq, "query_mix": {"table_keys": n_hit, "reverse_complements": n_rc, "mutants": n_mut},
        "reps": args.reps, "warmup": args.warmup, "statistic": "median, device events on the counter's stream",
        "device": {
            "index_build_ms": median_ms(build), "lookup_ms": median_ms(look), "dbjg_links_ms": median_ms(links),
            "lookup_runs_ms": [round(a.elapsed_time(b_), 3) for a, b_ in look],
            "index_build_runs_ms": [round(a.elapsed_time(b_), 3) for a, b_ in build],
            "dbjg_links_runs_ms": [round(a.elapsed_time(b_), 3) for a, b_ in links],
            "lookups_per_s": round(nq / (median_ms(look) * 1e-3)), "hits": dev_hits,
            "index_slots": 1 << max(1, (2 * n_out - 1).bit_length()),
            "index_bytes": 8 << max(1, (2 * n_out - 1).bit_length()),
            "links_bytes": 10 * n_out, "device_bytes_with_index_and_links": bytes_before,
            "device_bytes_peak": st2["device_bytes_peak"],
        },
        "host_route": host, "synth_seconds": round(gen_s, 2),
    }
    if host:
        d = res["device"]
        res["comparison"] = {
            "device_ms_build_plus_lookup": round(d["index_build_ms"] + d["lookup_ms"], 3),
            "host_ms_handoff_plus_find": round(host["handoff_ms"] + host["find_ms"], 1),
            "ratio_host_over_device": round((host["handoff_ms"] + host["find_ms"]) /
                                            (d["index_build_ms"] + d["lookup_ms"]), 2),
            "lookup_only_ratio_find_over_lookup": round(host["find_ms"] / d["lookup_ms"], 2),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    counter.close()


if __name__ == "__main__":
    main()
