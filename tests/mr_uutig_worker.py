"""Worker of tests/test_uutigs_ranks.py (TEST INFRASTRUCTURE): one rank of mhmkc_uutigs_ranks.

Every rank is a process with its own counter on the same GPU, as in mr_gpu_worker.run, and serves a list of cases in one
process group: it counts its shard of the case's reads with MHMKC_OWNER_MINIMIZER, builds the uutigs of all ranks' tables
(KmerCounter.uutigs_ranks) and saves its table, contig arrays, row map, ids and info. The transport is TorchDistTransport
(gloo), or with opts["rccl"] libmhmkc's RCCL path (each rank with its own NCCL_HOSTID: RCCL refuses two ranks of one
communicator on one device otherwise).
"""
import functools
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))


def shard(n: int, rank: int, world: int):
    return n * rank // world, n * (rank + 1) // world


def rccl_same_gpu_env(rank: int):
    """RCCL refuses two ranks of one communicator on one GPU ("Duplicate GPU detected"), unless the ranks look like
    different hosts: a per-rank NCCL_HOSTID, the socket network transport over loopback, no InfiniBand."""
    os.environ.update(NCCL_HOSTID=f"mhmkc-uutig-ranks-{rank}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1",
                      NCCL_NET="Socket")


@functools.lru_cache(maxsize=None)
def case_reads(setname: str, k: int):
    """The reads of a case: the small sets of tests/test_uutigs.py (tests/uutig_lib.py, tests/common.py)."""
    from common import hot_set, synth_set
    from uutig_lib import circular_set, cycle_set, multi_cycle_set, order_tie_set, palindrome_set, tie_set, tiny_set

    if setname == "synth":
        return synth_set(3000, 20000, 5)
    if setname == "circ":
        return circular_set()
    if setname.startswith("cyc"):
        return cycle_set(int(setname[3:]))
    if setname == "multi":
        return multi_cycle_set()
    if setname == "hot":
        return hot_set()
    if setname.startswith("tiny"):
        return tiny_set(k, int(setname[4:]))
    if setname.startswith("pal"):
        return palindrome_set(k, setname.endswith("+"))
    if setname.startswith("otie"):
        return order_tie_set(int(setname[4:]))
    if setname.startswith("tie"):
        return tie_set(word=int(setname[3:]), read_len=160)
    raise ValueError(setname)


def case_file(out_dir, setname: str, k: int, rank: int) -> Path:
    return Path(out_dir) / f"{setname}_k{k}_rank{rank}.npz"


def make_counter(m, dist, k: int, rank: int, world: int, opts: dict):
    if opts.get("rccl"):
        obj = [m.comm_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        return m.KmerCounter(k, device=0, rank=rank, n_ranks=world, comm_id=obj[0], output_owner=m.MHMKC_OWNER_MINIMIZER)
    return m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                         output_owner=m.MHMKC_OWNER_MINIMIZER)


def info_arrays(info: dict) -> dict:
    """uutigs_ranks_info as flat arrays for an .npz."""
    out = {}
    for key, v in info.items():
        out["info_" + key] = np.array(list(v.values())) if isinstance(v, dict) else np.array(v)
    return out


def run(rank: int, world: int, port: int, cases: list, out_dir: str, opts: dict):
    import torch.distributed as dist

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if opts.get("rccl"):
        rccl_same_gpu_env(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for setname, k in cases:
        b, o = case_reads(setname, k)
        lo, hi = shard(o.size - 1, rank, world)
        c = make_counter(m, dist, k, rank, world, opts)
        try:
            c.add_packed_reads(b[int(o[lo]):int(o[hi])], (o[lo:hi + 1] - o[lo]).astype(np.uint64))
            c.finish()
            t = c.fetch()
            r = c.uutigs_ranks()
            again = c.uutigs_ranks()  # kept: no second build, no collective
            offsets, seqs, depths, n_kmers = c.uutigs()
            row_ctg, row_pos, row_rc = c.uutig_rows()
            strs, sdepths = c.uutig_strings()
            assert strs == [seqs.tobytes().decode("ascii")[int(offsets[j]):int(offsets[j + 1])] for j in range(len(depths))]
            dev = c.uutigs_device()
            info = c.uutigs_ranks_info()
            uinfo = c.uutigs_info()
            st = c.stats()
            c.reset()
            codes = []
            for call in (c.uutigs, c.uutig_rows, c.uutigs_device):  # after reset: a multi-rank handle without a build
                try:
                    call()
                    codes.append(0)
                except N.MhmkcError as e:
                    codes.append(e.code)
        finally:
            c.close()
        np.savez(case_file(out_dir, setname, k, rank), keys=t.keys, counts=t.counts, left=t.left, right=t.right,
                 offsets=offsets, seqs=seqs, depths=depths, n_kmers=n_kmers, row_ctg=row_ctg, row_pos=row_pos, row_rc=row_rc,
                 n_ctgs=r["n_ctgs"], n_bases=r["n_bases"], first_id=r["first_id"], n_ctgs_all=r["n_ctgs_all"],
                 same_again=int(again == r), dev_n_ctgs=dev["n_ctgs"], dev_n_bases=dev["n_bases"], dev_n_out=dev["n_out"],
                 uinfo_n_ctgs=uinfo["n_ctgs"], uinfo_n_bases=uinfo["n_bases"], device_bytes=st["device_bytes"],
                 reset_codes=np.array(codes), **info_arrays(info))
        dist.barrier()
    dist.destroy_process_group()


def run_chain(rank: int, world: int, port: int, ks: list, out_dir: str, opts: dict):
    """The multi-k chain over the ranks: every round counts the rank's shard of the reads plus the rank's own contigs of
    the round before (uutig_strings() after uutigs_ranks(), the depths as Contig::get_uint16_t_depth, src/contigs.hpp:65)
    and saves its table."""
    import torch.distributed as dist

    import mhm2_proxy_amd as m

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    b, o = case_reads("synth", 21)
    lo, hi = shard(o.size - 1, rank, world)
    ctgs, depths = [], np.zeros(0)
    for k in ks:
        c = make_counter(m, dist, k, rank, world, opts)
        try:
            c.add_packed_reads(b[int(o[lo]):int(o[hi])], (o[lo:hi + 1] - o[lo]).astype(np.uint64))
            if k != ks[0]:
                c.add_ctgs(ctgs, np.minimum(depths, 65535.0).astype(np.uint16))
            c.finish()
            t = c.fetch()
            r = c.uutigs_ranks()
            ctgs, depths = c.uutig_strings()
        finally:
            c.close()
        np.savez(Path(out_dir) / f"chain_k{k}_rank{rank}.npz", keys=t.keys, counts=t.counts, left=t.left, right=t.right,
                 n_ctgs=r["n_ctgs"], n_ctgs_all=r["n_ctgs_all"])
        dist.barrier()
    dist.destroy_process_group()
