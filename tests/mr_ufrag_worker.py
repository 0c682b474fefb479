"""Worker of tests/test_uutigs_frags.py (TEST INFRASTRUCTURE): one rank of mhmkc_uutigs_frags.

Every rank is a process with its own counter on the same GPU, as in mr_uutig_worker.run, and serves a list of cases in one
process group: it counts its shard of the case's reads with MHMKC_OWNER_MINIMIZER, builds the uutigs of all ranks' tables
from rank-local fragments (KmerCounter.uutigs_frags) and saves its table, contig arrays, row map, ids and info. Over gloo
the transport counts its calls, so that the kept build is seen to run no collective; over RCCL (opts["rccl"]) the
unchanged info shows it. opts["equal"]: the cases are built a second time, by uutigs_ranks() on a second counter over
the same shard, and both builds' arrays are saved. run_chain is the step to the next k on every rank.
"""
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))


def case_file(out_dir, setname: str, k: int, rank: int) -> Path:
    return Path(out_dir) / f"{setname}_k{k}_rank{rank}.npz"


def info_arrays(info: dict, prefix: str = "info_") -> dict:
    out = {}
    for key, v in info.items():
        out[prefix + key] = np.array(list(v.values())) if isinstance(v, dict) else np.array(v)
    return out


def counting_transport(m):
    class Counting(m.TorchDistTransport):
        calls = 0

        def _allgather(self, *a):
            self.calls += 1
            return super()._allgather(*a)

        def _alltoallv(self, *a):
            self.calls += 1
            return super()._alltoallv(*a)

    return Counting()


def shard_of(b, o, rank, world):
    from mr_uutig_worker import shard

    lo, hi = shard(o.size - 1, rank, world)
    return b[int(o[lo]):int(o[hi])], (o[lo:hi + 1] - o[lo]).astype(np.uint64)


def arrays_of(c) -> dict:
    offsets, seqs, depths, n_kmers = c.uutigs()
    row_ctg, row_pos, row_rc = c.uutig_rows()
    return {"offsets": offsets, "seqs": seqs, "depths": depths, "n_kmers": n_kmers, "row_ctg": row_ctg, "row_pos": row_pos,
            "row_rc": row_rc}


def run(rank: int, world: int, port: int, cases: list, out_dir: str, opts: dict):
    import torch.distributed as dist

    import mhm2_proxy_amd as m
    from mhm2_proxy_amd import _native as N
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
        extra = {}
        try:
            c.add_packed_reads(sb, so)
            c.finish()
            t = c.fetch()
            r = c.uutigs_frags()
            info = c.uutigs_frags_info()
            calls = tr.calls if tr else 0
            again = c.uutigs_frags()  # kept: no second build, no collective
            by_ranks = c.uutigs_ranks()  # the other call returns the kept build too
            info_again = c.uutigs_frags_info()
            quiet = int(tr.calls == calls) if tr else 1
            arr = arrays_of(c)
            strs, _ = c.uutig_strings()
            blob = arr["seqs"].tobytes().decode("ascii")
            assert strs == [blob[int(arr["offsets"][j]):int(arr["offsets"][j + 1])] for j in range(len(arr["depths"]))]
            dev = c.uutigs_device()
            rinfo = c.uutigs_ranks_info()
            uinfo = c.uutigs_info()
            c.reset()
            codes = []
            for call in (c.uutigs, c.uutig_rows, c.uutigs_device):  # after reset: a multi-rank handle without a build
                try:
                    call()
                    codes.append(0)
                except N.MhmkcError as e:
                    codes.append(e.code)
            if opts.get("equal"):  # the replicated build on a second counter over the same shard
                c2 = make_counter(m, dist, k, rank, world, opts)
                try:
                    c2.add_packed_reads(sb, so)
                    c2.finish()
                    r2 = c2.uutigs_ranks()
                    extra = {"rep_" + key: v for key, v in arrays_of(c2).items()}
                    extra["rep_keys"] = c2.fetch().keys
                    extra["rep_same_ids"] = int(r2 == r)
                    extra["rep_frags_again"] = int(c2.uutigs_frags() == r2)  # kept the other way round
                    extra.update(info_arrays(c2.uutigs_frags_info(), "rep_finfo_"))
                finally:
                    c2.close()
        finally:
            c.close()
        np.savez(case_file(out_dir, setname, k, rank), keys=t.keys, counts=t.counts, left=t.left, right=t.right,
                 n_ctgs=r["n_ctgs"], n_bases=r["n_bases"], first_id=r["first_id"], n_ctgs_all=r["n_ctgs_all"],
                 same_again=int(again == r and by_ranks == r and info_again == info), quiet=quiet, dev_n_ctgs=dev["n_ctgs"],
                 dev_n_bases=dev["n_bases"], dev_n_out=dev["n_out"], uinfo_n_ctgs=uinfo["n_ctgs"],
                 uinfo_n_bases=uinfo["n_bases"], reset_codes=np.array(codes), **arr, **info_arrays(info),
                 **info_arrays(rinfo, "rinfo_"), **extra)
        dist.barrier()
    if opts.get("hash"):  # a finished MHMKC_OWNER_HASH counter: refused, and no collective runs for it
        b, o = case_reads("tiny2", 21)
        sb, so = shard_of(b, o, rank, world)
        tr = counting_transport(m)
        c = m.KmerCounter(21, device=0, rank=rank, n_ranks=world, transport=tr, output_owner=m.MHMKC_OWNER_HASH)
        try:
            c.add_packed_reads(sb, so)
            c.finish()
            calls, code = tr.calls, 0
            try:
                c.uutigs_frags()
            except N.MhmkcError as e:
                code = e.code
            np.savez(Path(out_dir) / f"hash_rank{rank}.npz", code=code, quiet=int(tr.calls == calls), n_out=len(c.fetch()))
        finally:
            c.close()
        dist.barrier()
    dist.destroy_process_group()


def run_chain(rank: int, world: int, port: int, ks: list, out_dir: str, opts: dict):
    """k = ks[0] -> ks[1] on every rank: uutigs_frags() on the first counter, add_ctgs_from into the second."""
    import torch.distributed as dist

    import mhm2_proxy_amd as m
    from mr_uutig_worker import make_counter
    from ufrag_lib import case_reads

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    b, o = case_reads("synth", ks[0])
    sb, so = shard_of(b, o, rank, world)
    a = make_counter(m, dist, ks[0], rank, world, opts)
    c = make_counter(m, dist, ks[1], rank, world, opts)
    try:
        a.add_packed_reads(sb, so)
        a.finish()
        r = a.uutigs_frags()
        c.add_packed_reads(sb, so)
        c.add_ctgs_from(a)
        c.finish()
        t = c.fetch()
    finally:
        c.close()
        a.close()
    np.savez(Path(out_dir) / f"chain_k{ks[1]}_rank{rank}.npz", keys=t.keys, counts=t.counts, left=t.left, right=t.right,
             n_ctgs=r["n_ctgs"], n_ctgs_all=r["n_ctgs_all"])
    dist.barrier()
    dist.destroy_process_group()
