"""Worker of tests/test_route_ranks.py (TEST INFRASTRUCTURE): one rank of mhmkc_lookup_ranks / mhmkc_dbjg_links_ranks.

Every rank is a process with its own counter on the same GPU, as in mr_uutig_worker.run, and serves a list of cases in one
process group (gloo, opened with a timeout, so that a collective the ranks do not all enter ends the worker instead of
hanging it). Per case the rank counts its shard with MHMKC_OWNER_MINIMIZER, learns the other ranks' tables (an
all_gather of the fetched tables: the queries are built from the union), asks its batches and saves the queries with the
answers; the parent compares them with what the union and the oracle's owner function say.
"""
import ctypes as C
import datetime
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

from mr_uutig_worker import case_reads, make_counter, rccl_same_gpu_env, shard  # noqa: E402

SIZES = (1, 63, 64, 65)  # per-rank batch sizes around a wave; the chunk and 3 * chunk + 1 join them
CHUNKS = (64, 257)
GLOO_TIMEOUT_S = 120


def case_file(out_dir, setname: str, k: int, rank: int) -> Path:
    return Path(out_dir) / f"route_{setname}_k{k}_rank{rank}.npz"


def top_mask_words(k: int, nl: int) -> np.ndarray:
    """A key of nl words whose k bases are all T (every used bit set)."""
    w = np.full(nl, 2**64 - 1, dtype=np.uint64)
    kl = k - 32 * (nl - 1)
    w[nl - 1] = np.uint64((2**64 - 1) ^ ((1 << (64 - 2 * kl)) - 1))
    return w


def lookup_batches(u_keys: np.ndarray, k: int, rank: int):
    """The rank's two big batches: (keys looked up as given, keys looked up canonicalized)."""
    from query_lib import mutate_keys, revcomp_keys

    nl = u_keys.shape[1]
    rng = np.random.default_rng(1000 + 17 * rank)
    rc = revcomp_keys(u_keys, k) if len(u_keys) else u_keys
    sample = u_keys[rng.permutation(len(u_keys))[:400]]
    mut = mutate_keys(sample, k, rng) if len(sample) else sample
    ones = top_mask_words(k, nl)
    edge = np.stack([np.zeros(nl, dtype=np.uint64), ones, np.full(nl, 2**64 - 1, dtype=np.uint64)])
    hot = np.repeat((u_keys[rank % len(u_keys)] if len(u_keys) else ones)[None, :], 300, axis=0)
    as_given = np.concatenate([u_keys, rc, mut, hot, edge])
    canon = np.concatenate([rc, mut, edge])
    return (np.ascontiguousarray(as_given[rng.permutation(len(as_given))]),
            np.ascontiguousarray(canon[rng.permutation(len(canon))]))


def sized_batch(pool: np.ndarray, size: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(pool[rng.integers(0, len(pool), size=size)])


def size_plan(rank: int, world: int, chunk: int):
    """The batch size of this rank in every scenario of one chunk: all ranks empty; one rank empty; then the sizes
    rotated over the ranks, so that the ranks need different numbers of rounds and a batch equal to the chunk occurs."""
    sizes = SIZES + (chunk, 3 * chunk + 1)
    plan = [0, 0 if rank == 1 else 65]
    return plan + [sizes[(rank + j) % len(sizes)] for j in range(len(sizes))]


def code_of(call):
    from mhm2_proxy_amd import _native as N

    try:
        call()
        return 0
    except N.MhmkcError as e:
        return e.code


def device_array(ptr, n, typestr):
    import torch

    class DeviceArray:
        def __init__(self):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}

    return torch.as_tensor(DeviceArray(), device="cuda").cpu().numpy()


def info_arrays(prefix: str, info: dict) -> dict:
    out = {}
    for key, v in info.items():
        out[f"{prefix}_{key}"] = np.array(list(v.values())) if isinstance(v, dict) else np.array(v)
    return out


def run_case(m, dist, setname, k, rank, world, opts, out_dir):
    import torch

    from mhm2_proxy_amd import _native as N

    L = N.lib()
    b, o = case_reads(setname, k)
    lo, hi = shard(o.size - 1, rank, world)
    my_b, my_o = b[int(o[lo]):int(o[hi])], (o[lo:hi + 1] - o[lo]).astype(np.uint64)
    out = {}
    os.environ.pop("MHMKC_ROUTE_CHUNK", None)
    c = make_counter(m, dist, k, rank, world, opts)
    try:
        c.add_packed_reads(my_b, my_o)
        out["code_before_finish"] = np.array([code_of(lambda: c.lookup_ranks(np.zeros((1, c.n_longs), np.uint64))),
                                              code_of(c.dbjg_links_ranks)])
        c.finish()
        t = c.fetch()
        tables = [None] * world
        dist.all_gather_object(tables, (t.keys, t.counts, t.left, t.right))
        u_keys = np.concatenate([x[0] for x in tables])
        out.update(keys=t.keys, counts=t.counts, left=t.left, right=t.right)
        # existing behaviour: the local lookup answers for this rank's rows only, the single-rank links refuse
        out["local_rows"] = c.lookup(u_keys)[0] if len(u_keys) else np.zeros(0, np.uint32)
        out["links1_code_before"] = np.array(code_of(c.dbjg_links))

        # the two big batches, host arrays
        qa, qc = lookup_batches(u_keys, k, rank)
        res_a = c.lookup_ranks(qa)
        out.update(info_arrays("ia", c.route_info()))
        res_c = c.lookup_ranks(qc, canonicalize=True)
        for name, q, res in (("a", qa, res_a), ("c", qc, res_c)):
            out["q" + name] = q
            for f, v in zip(("ranks", "rows", "counts", "left", "right"), res):
                out[f"{name}_{f}"] = v
        # some output pointers NULL agree with the full call
        n = len(qa)
        only_ranks = np.empty(n, np.uint8)
        c._check(L.mhmkc_lookup_ranks(c._h, qa.ctypes.data, n, 0, only_ranks.ctypes.data, None, None, None, None))
        rows2, right2 = np.empty(n, np.uint32), np.empty(n, np.uint8)
        c._check(L.mhmkc_lookup_ranks(c._h, qa.ctypes.data, n, 0, None, rows2.ctypes.data, None, None, right2.ctypes.data))
        c._check(L.mhmkc_lookup_ranks(c._h, qa.ctypes.data, n, 0, None, None, None, None, None))
        out["null_ok"] = np.array(int((only_ranks == res_a[0]).all() and (rows2 == res_a[1]).all() and
                                      (right2 == res_a[4]).all()))
        # the device arrays
        qt = torch.from_numpy(qa.view(np.int64)).cuda()
        dev = c.lookup_ranks_tensors(qt)
        dev = [x.cpu().numpy() for x in dev]
        out["tensors_ok"] = np.array(int((dev[0] == res_a[0]).all() and (dev[1].view(np.uint32) == res_a[1]).all() and
                                         (dev[2].view(np.uint16) == res_a[2]).all() and (dev[3] == res_a[3]).all() and
                                         (dev[4] == res_a[4]).all()))
        # one hot owner: every rank asks only for what rank 0 holds
        qh = np.ascontiguousarray(tables[0][0])
        res_h = c.lookup_ranks(qh)
        out.update(info_arrays("ih", c.route_info()))
        out["qh"] = qh
        for f, v in zip(("ranks", "rows", "counts", "left", "right"), res_h):
            out[f"h_{f}"] = v
        # batch sizes around the chunk
        pool = np.concatenate([qa, qc])
        for chunk in CHUNKS:
            os.environ["MHMKC_ROUTE_CHUNK"] = str(chunk)
            for j, size in enumerate(size_plan(rank, world, chunk)):
                q = sized_batch(pool, size, 7000 + 131 * rank + 17 * j + chunk)
                res = c.lookup_ranks(q, canonicalize=bool(j & 1))
                info = c.route_info()
                name = f"s{chunk}_{j}"
                out[name + "_q"] = q
                for f, v in zip(("ranks", "rows", "counts", "left", "right"), res):
                    out[f"{name}_{f}"] = v
                out[name + "_info"] = np.array([info["rounds"], info["chunk"], info["entries"], info["queries"],
                                                info["queries_local"], info["queries_sent"], info["queries_recv"],
                                                info["bytes_sent"], info["bytes_recv"]])
        os.environ.pop("MHMKC_ROUTE_CHUNK", None)

        # the links, at the default chunk
        bytes0 = c.stats()["device_bytes"]
        links = c.dbjg_links_ranks()
        info_l = c.route_info()
        bytes1 = c.stats()["device_bytes"]
        again = c.dbjg_links_ranks()
        out["links_again_ok"] = np.array(int(all((x == y).all() for x, y in zip(links, again)) and
                                             c.route_info() == info_l))
        n_out = len(t)
        dv = c.dbjg_links_ranks_device()
        if n_out:
            c.synchronize()
            dev_ok = (device_array(dv["next_rank"], 2 * n_out, "|u1") == links[0].reshape(-1)).all() and \
                (device_array(dv["next_row"], 2 * n_out, "<i4").view(np.uint32) == links[1].reshape(-1)).all() and \
                (device_array(dv["status"], 2 * n_out, "|u1") == links[2].reshape(-1)).all()
        else:
            dev_ok = dv["next_rank"] is None and dv["next_row"] is None and dv["status"] is None
        out["links_device_ok"] = np.array(int(bool(dev_ok) and dv["n_out"] == n_out))
        out["links1_code_after"] = np.array(code_of(c.dbjg_links))
        out.update(next_rank=links[0], next_row=links[1], status=links[2], bytes0=np.array(bytes0), bytes1=np.array(bytes1))
        out.update(info_arrays("il", info_l))
        c.reset()
        out["bytes2"] = np.array(c.stats()["device_bytes"])
        out["code_after_reset"] = np.array([code_of(lambda: c.lookup_ranks(qa[:1])), code_of(c.dbjg_links_ranks),
                                            code_of(c.dbjg_links_ranks_device)])

        # a second count on the handle, the links in rounds of 64 entries
        os.environ["MHMKC_ROUTE_CHUNK"] = "64"
        c.add_packed_reads(my_b, my_o)
        c.finish()
        t2 = c.fetch()
        links64 = c.dbjg_links_ranks()
        out.update(info_arrays("i64", c.route_info()))
        os.environ.pop("MHMKC_ROUTE_CHUNK", None)
        out.update(keys2=t2.keys, counts2=t2.counts, left2=t2.left, right2=t2.right, next_rank64=links64[0],
                   next_row64=links64[1], status64=links64[2])
    finally:
        c.close()
    np.savez(case_file(out_dir, setname, k, rank), **out)


def run(rank: int, world: int, port: int, cases: list, out_dir: str, opts: dict):
    import torch.distributed as dist

    import mhm2_proxy_amd as m

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if opts.get("rccl"):
        rccl_same_gpu_env(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=GLOO_TIMEOUT_S))
    for setname, k in cases:
        run_case(m, dist, setname, k, rank, world, opts, out_dir)
        dist.barrier()
    dist.destroy_process_group()
