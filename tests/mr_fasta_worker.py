"""Worker of tests/test_fasta_ranks.py (TEST INFRASTRUCTURE): one rank of the assembly statistics and the FASTA file of
several ranks.

Every rank is a process with its own counter on the same GPU, as in mr_ufrag_worker.run, and serves a list of cases in one
process group: it counts its shard of the case's reads with MHMKC_OWNER_MINIMIZER, asks for the uutigs forms before any
ranks build (refused, and over gloo the transport sees no call), builds the uutigs by uutigs_frags(), and for every
min_ctg_len saves uutigs_stats(), uutigs_fasta(), the kept text, and writes its block of the one file all ranks share.
Then the generic calls: a bad depth on rank 1 only, which must fail every rank, and a good call after it.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))


def case_file(out_dir, setname: str, k: int, rank: int) -> Path:
    return Path(out_dir) / f"{setname}_k{k}_rank{rank}.npz"


def fasta_file(out_dir, setname: str, k: int, min_len: int) -> Path:
    return Path(out_dir) / f"{setname}_k{k}_min{min_len}.fasta"


def min_lens(k: int):
    return (0, k + 20)


def code_of(call) -> int:
    from mhm2_proxy_amd import _native as N

    try:
        call()
        return 0
    except N.MhmkcError as e:
        return e.code


def generic_case(rank: int):
    """A few contigs per rank, different on every rank (rank r has r + 2 of them)."""
    import fasta_cases as F

    rng = np.random.default_rng(100 + rank)
    n = rank + 2
    return F.Case(f"generic{rank}", tuple(F.rand_seq(rng, 30 + 7 * i) for i in range(n)),
                  tuple(float(1.25 * (i + 1) + rank) for i in range(n)), 1000 * rank, (0,))


def run(rank: int, world: int, port: int, cases: list, out_dir: str, opts: dict):
    import torch
    import torch.distributed as dist

    import fasta_cases as F
    import mhm2_proxy_amd as m
    from mr_ufrag_worker import counting_transport, shard_of
    from mr_uutig_worker import make_counter, rccl_same_gpu_env
    from ufrag_lib import case_reads

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if opts.get("rccl"):
        rccl_same_gpu_env(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for setname, k in cases:
        b, o = case_reads(setname, k)
        sb, so = shard_of(b, o, rank, world)
        tr = None
        if opts.get("rccl"):
            c = make_counter(m, dist, k, rank, world, opts)
        else:
            tr = counting_transport(m)
            c = m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=tr, output_owner=m.MHMKC_OWNER_MINIMIZER)
        try:
            c.add_packed_reads(sb, so)
            c.finish()
            calls = tr.calls if tr else 0
            early = [code_of(c.uutigs_stats), code_of(c.uutigs_fasta)]  # no ranks build yet: refused before any collective
            quiet = int(tr.calls == calls) if tr else 1
            r = c.uutigs_frags()
            offsets, seqs, depths, _ = c.uutigs()
            out = {}
            for mn in min_lens(k):
                out[f"stats{mn}"] = c.uutigs_stats(mn)
                out[f"fasta{mn}"] = c.uutigs_fasta(mn)
                text = np.frombuffer(c.fasta_bytes(), dtype=np.uint8)
                c.fasta_write(fasta_file(out_dir, setname, k, mn))
                out[f"info{mn}"] = c.fasta_info()
                np.save(Path(out_dir) / f"{setname}_k{k}_min{mn}_rank{rank}.text.npy", text)
        finally:
            c.close()
        np.savez(case_file(out_dir, setname, k, rank), offsets=offsets, seqs=seqs, depths=depths, first_id=r["first_id"],
                 n_ctgs_all=r["n_ctgs_all"], early=np.array(early), quiet=quiet, results=np.array(json.dumps(out)))
        dist.barrier()
    if opts.get("generic"):  # the generic calls on a handle that never counted
        c = make_counter(m, dist, 21, rank, world, opts)
        try:
            case = generic_case(rank)
            bases, offsets, depths = F.arrays(case)
            st, ot = torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()
            good, bad = torch.from_numpy(depths).cuda(), torch.from_numpy(depths).cuda()
            if rank == 1:
                bad[1] = -1.0
            code = code_of(lambda: c.ctgs_fasta_tensors(st, ot, bad, case.first_id, 0))
            gone = code_of(c.fasta_bytes)  # a failed call leaves no text on any rank
            fa = c.ctgs_fasta_tensors(st, ot, good, case.first_id, 0)
            text = c.fasta_bytes()
            stats = c.ctgs_stats_tensors(st, ot, good, 0)
            path = Path(out_dir) / "generic.fasta"
            c.fasta_write(path)
            missing = code_of(lambda: c.fasta_write(Path(out_dir) / "no-such-dir" / "x.fasta"))  # rank 0 cannot make it
        finally:
            c.close()
        np.savez(Path(out_dir) / f"generic_rank{rank}.npz", code=code, gone=gone, missing=missing,
                 text=np.frombuffer(text, dtype=np.uint8), results=np.array(json.dumps({"fasta": fa, "stats": stats})))
        dist.barrier()
    dist.destroy_process_group()
