"""Worker of tests/test_ctgs_ranks.py (TEST INFRASTRUCTURE): one rank of a contig pass whose contigs reach the ranks on the
device (mhmkc_add_ctgs_device / mhmkc_add_ctgs_from on handles with n_ranks > 1).

Every rank is a process with its own counter on the same GPU, as in mr_uutig_worker.run, and serves a list of cases in
one process group. A case names its reads, its contigs per rank and how each rank adds them (ROUTES); the rank counts its
shard of the reads with MHMKC_OWNER_MINIMIZER plus its contigs and saves its table, ctgs_ranks_info() and device_bytes
around the round (run_cases). run_chain is the multi-k chain by uutigs_ranks() and add_ctgs_from(prev) on every rank. One
spawn (serve) runs both for its world. The transport is TorchDistTransport (gloo), or with opts["rccl"] libmhmkc's RCCL path.
"""
import functools
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

from mr_uutig_worker import make_counter, rccl_same_gpu_env, shard  # noqa: E402

# how a rank adds its contigs: "dev" in two device adds (float64 depths with a fraction, then uint16), "host" add_ctgs,
# "none" no call at all
ROUTES = ("dev", "host", "none")

# Edge cases: the lengths of every rank's contigs, for three ranks (two ranks take the first and the last list). Per-rank
# byte counts 0, 1, 2, 15, 16, 17, 31, 32, 33, 4097; the offsets at which rank 1 and rank 2 land are odd, even but no
# multiple of 16, and multiples of 16; a rank whose contigs are all shorter than k + 2; a rank with empty contigs; a
# single contig on the last rank only; and sets large enough for the grid-stride loops to turn with the grid capped.
EDGE_K = 21
EDGES = {
    "e1": ([1], [15], [4097]),                      # rank 1 lands at 1, rank 2 at 16
    "e2": ([2], [17], [33]),                        # 2, 19
    "e3": ([16], [16, 16], [31]),                   # 16, 48
    "e4": ([4097], [33], [0, 0]),                   # 4097, 4130; rank 2: empty contigs only
    "e5": ([], [], [100]),                          # a single contig, on the last rank
    "e6": ([10, 12, 22], [15, 0, 2], [32]),         # rank 0: no contig reaches k + 2; 44, 61
    "e7": ([31], [1], [2, 13]),                     # 31, 32
    "e8": ([4097] * 8, [4097] * 7 + [15], [25] * 300 + [3000]),  # 2049 / 1793 vectors, 301 contigs on rank 2
}
EDGE_GRIDS = (0, 1, 3)


def frac(depths: np.ndarray) -> np.ndarray:
    """Float depths whose Contig::get_uint16_t_depth is `depths`."""
    return depths.astype(np.float64) + 0.7


def split_contiguous(n: int, holders: list, world: int):
    """[lo, hi) of n contigs per rank: contiguous pieces, in rank order, for the ranks in `holders`; the others get none."""
    out, j = [], 0
    for r in range(world):
        if r in holders:
            out.append((n * j // len(holders), n * (j + 1) // len(holders)))
            j += 1
        else:
            out.append((0, 0))
    return out


@functools.lru_cache(maxsize=None)
def edge_contigs(name: str):
    """Contigs of the lengths EDGES[name] gives, cut from the genome the reads come from (common.synth_set(300, 6000, 31)),
    every 97th base an N and every 53rd lowercase, depths 2..39. Three lists (ranks 0, 1, 2)."""
    import mhm2_proxy_amd as m

    rng = np.random.default_rng(sum(map(ord, name)))
    gs = "".join("ACGT"[int(x)] for x in m.synth_genome(6000, 31))
    out, pos = [], 0
    for lens in EDGES[name]:
        seqs = []
        for L in lens:
            st = int(rng.integers(0, len(gs) - L)) if L < len(gs) else 0
            s = list(gs[st:st + L])
            for j in range(L):
                if (pos + j) % 97 == 96:
                    s[j] = "N"
                elif (pos + j) % 53 == 52:
                    s[j] = s[j].lower()
            pos += L
            seqs.append("".join(s))
        out.append((seqs, rng.integers(2, 40, len(seqs)).astype(np.uint16)))
    return out


@functools.lru_cache(maxsize=None)
def case_data(name: str, world: int):
    """(k, packed reads, offsets, [(contig strings, uint16 depths, route) per rank], grid knob) of a case. The oracle's
    input is the concatenation of the ranks' contigs in rank order."""
    from common import ctg_set, synth_set

    kind, _, arg = name.partition(":")
    if kind in ("order", "order_host"):  # ctg_set, contiguous shards: rank-major order is the original order
        k = int(arg)
        b, o, seqs, depths = ctg_set()
        cuts = split_contiguous(len(seqs), list(range(world)), world)
        route = "dev" if kind == "order" else "host"
        return k, b, o, [(seqs[lo:hi], depths[lo:hi], route) for lo, hi in cuts], 0
    if kind == "mixed":  # world 3. a: rank 0 host, rank 1 device, rank 2 nothing; b: rank 2 alone, on the device
        k = 33
        b, o, seqs, depths = ctg_set()
        holders, routes = ([0, 1], ["host", "dev", "none"]) if arg == "a" else ([world - 1], ["none"] * (world - 1) + ["dev"])
        if world == 2 and arg == "a":
            routes = ["host", "dev"]
        cuts = split_contiguous(len(seqs), holders, world)
        return k, b, o, [(seqs[lo:hi], depths[lo:hi], routes[r]) for r, (lo, hi) in enumerate(cuts)], 0
    if kind == "edge":
        ename, _, grid = arg.partition("@")
        b, o = synth_set(300, 6000, 31)
        lists = edge_contigs(ename)
        if world == 2:
            lists = [lists[0], lists[2]]
        return EDGE_K, b, o, [(s, d, "dev") for s, d in lists], int(grid or 0)
    if kind == "errors":  # one good device add per rank, then refused ones
        k = 21
        b, o = synth_set(300, 6000, 31)
        lists = edge_contigs("e8")
        return k, b, o, [(lists[r % 3][0][:6], lists[r % 3][1][:6], "dev") for r in range(world)], 0
    raise ValueError(name)


def case_file(out_dir, name: str, rank: int) -> Path:
    return Path(out_dir) / f"{name.replace(':', '_').replace('@', '_g')}_rank{rank}.npz"


def dev_tensors(seqs, depths, f64: bool):
    import torch

    blob = np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8)
    bases = torch.from_numpy(blob.copy()).cuda()
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    d = torch.from_numpy(frac(depths) if f64 else np.asarray(depths, dtype=np.uint16).copy()).cuda()
    return bases, torch.from_numpy(offs).cuda(), d


def add_contigs(c, seqs, depths, route: str):
    if route == "none":
        return
    if route == "host":
        c.add_ctgs(seqs, depths)
        return
    h = len(seqs) // 2
    if h:
        c.add_ctgs_tensors(*dev_tensors(seqs[:h], depths[:h], True))
    c.add_ctgs_tensors(*dev_tensors(seqs[h:], depths[h:], False))  # (an empty second half is a call with no contigs)


def refused_adds(c, N):
    """The single-rank error cases of the device add on this multi-rank handle: their codes; nothing joins the round."""
    seqs, depths = ["ACGTACGTACGTACGTACGTACGTACGTACGTACGT", "TTGACCATGACCATTTGACGGATCAGGATC"], np.array([3, 4], dtype=np.uint16)
    bases, offs, d = dev_tensors(seqs, depths, True)
    nc, total = len(seqs), int(offs[-1])

    def raw(bases_, offs_, d_):
        c._after_torch(bases_)
        return N.lib().mhmkc_add_ctgs_device(c._h, bases_.data_ptr(), offs_.data_ptr(), d_.data_ptr(), N.MHMKC_DEPTH_F64, nc,
                                             total)

    codes = []
    bad = bases.clone()
    bad[5] = ord("X")
    codes.append(raw(bad, offs, d))
    o2 = offs.clone()
    o2[1] = o2[2] + 1
    codes.append(raw(bases, o2, d))
    d2 = d.clone()
    d2[1] = float("nan")
    codes.append(raw(bases, offs, d2))
    import torch

    torch.cuda.synchronize()
    return codes


def one_round(c, N, b, o, rank, world, seqs, depths, route, errors: bool):
    lo, hi = shard(o.size - 1, rank, world)
    before = c.stats()["device_bytes"]
    c.add_packed_reads(b[int(o[lo]):int(o[hi])], (o[lo:hi + 1] - o[lo]).astype(np.uint64))
    add_contigs(c, seqs, depths, route)
    codes = refused_adds(c, N) if errors else []
    c.finish()
    t = c.fetch()
    info = c.ctgs_ranks_info()
    st = c.stats()
    c.reset()
    after = c.stats()["device_bytes"]
    return t, info, st, before, after, codes


def serve(rank: int, world: int, port: int, plan: dict, out_dir: str, opts: dict):
    """One rank of a spawn: plan["cases"] (run_cases), then the chain over plan["chain"] (run_chain), in one process group."""
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if opts.get("rccl"):
        rccl_same_gpu_env(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    run_cases(dist, rank, world, plan.get("cases", []), out_dir, opts)
    if plan.get("chain"):
        run_chain(dist, rank, world, plan["chain"], out_dir, opts)
    dist.destroy_process_group()


def run_cases(dist, rank: int, world: int, cases: list, out_dir: str, opts: dict):
    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N

    for name in cases:
        k, b, o, per_rank, grid = case_data(name, world)
        seqs, depths, route = per_rank[rank]
        c = make_counter(m, dist, k, rank, world, opts)
        try:
            zeros = c.ctgs_ranks_info()  # before any finish
            N.debug_set("ctgx_grid", grid)
            # the round twice on one counter: the first grows the buffers that stay, the second is the one saved
            one_round(c, N, b, o, rank, world, seqs, depths, route, False)
            cleared = c.ctgs_ranks_info()  # after reset
            t, info, st, before, after, codes = one_round(c, N, b, o, rank, world, seqs, depths, route, name.startswith("errors"))
        finally:
            N.debug_set("ctgx_grid", 0)
            c.close()
        np.savez(case_file(out_dir, name, rank), keys=t.keys, counts=t.counts, left=t.left, right=t.right,
                 ctg_kmers=st["ctg_kmers"], device_bytes_peak=st["device_bytes_peak"], before=before, after=after,
                 codes=np.array(codes, dtype=np.int64), zeros=np.array(list(zeros.values()), dtype=np.float64),
                 cleared=np.array(list(cleared.values()), dtype=np.float64),
                 **{"info_" + key: np.array(v) for key, v in info.items()})
        dist.barrier()


def run_chain(dist, rank: int, world: int, ks: list, out_dir: str, opts: dict):
    """k -> next k over the ranks without the host: every round counts the rank's shard of the reads plus, after
    uutigs_ranks() on the round before, that handle's part of the union's uutigs (add_ctgs_from)."""
    import mhm2_proxy_amd as m
    from mr_uutig_worker import case_reads

    b, o = case_reads("synth", 21)
    lo, hi = shard(o.size - 1, rank, world)
    prev = None
    try:
        for k in ks:
            c = make_counter(m, dist, k, rank, world, opts)
            try:
                c.add_packed_reads(b[int(o[lo]):int(o[hi])], (o[lo:hi + 1] - o[lo]).astype(np.uint64))
                if prev is not None:
                    c.add_ctgs_from(prev)
                c.finish()
            except BaseException:
                c.close()
                raise
            if prev is not None:
                prev.close()
            prev = c
            t = c.fetch()
            info = c.ctgs_ranks_info()
            r = c.uutigs_ranks()
            np.savez(Path(out_dir) / f"chain_k{k}_rank{rank}.npz", keys=t.keys, counts=t.counts, left=t.left, right=t.right,
                     n_ctgs=r["n_ctgs"], n_ctgs_all=r["n_ctgs_all"], ctg_kmers=c.stats()["ctg_kmers"],
                     **{"info_" + key: np.array(v) for key, v in info.items()})
            dist.barrier()
    finally:
        if prev is not None:
            prev.close()
