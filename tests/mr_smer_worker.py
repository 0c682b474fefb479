"""Worker of tests/test_supermer_edges.py (TEST INFRASTRUCTURE): one rank of the supermer exchange over a list of cases.

One process group per (k, world), gloo plus the host-staged transport as in mr_gpu_worker.run; inside it one counter
per case, so the processes start once and not once per case. The parent has written every case's batches to
<out_dir>/in_<case>.npz (r<rank>_b<i>_bytes / _offs); the rank adds its batches as host batches (add_packed_reads) or
device batches (add_tensors) as the case says, finishes, fetches and saves the table and the counter's stats to
<out_dir>/<case>_rank<rank>.npz.
"""
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))


def run(rank: int, world: int, port: int, k: int, out_dir: str, cases: list):
    """cases: [{"name", "kinds": {rank: ["host" | "device", ...]}, "env": {...}, "env_by_rank": {rank: {...}}}]."""
    import torch
    import torch.distributed as dist

    import mhm2_proxy_amd as m
    from conftest import apply_env
    from mhm2_proxy_amd import _native as N

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for case in cases:
        env = dict(case.get("env", {}))
        env.update(case.get("env_by_rank", {}).get(rank, {}))
        apply_env(env)
        z = np.load(Path(out_dir) / f"in_{case['name']}.npz")
        c = m.KmerCounter(k, device=0, rank=rank, n_ranks=world, transport=m.TorchDistTransport(),
                          output_owner=m.MHMKC_OWNER_MINIMIZER)
        keep = []
        for i, kind in enumerate(case["kinds"].get(rank, [])):
            b, o = z[f"r{rank}_b{i}_bytes"], z[f"r{rank}_b{i}_offs"]
            if kind == "host":
                c.add_packed_reads(b, o.astype(np.uint64))
            else:
                bt = torch.from_numpy(b.copy()).cuda()
                ot = torch.from_numpy(o.astype(np.int64)).cuda()
                keep.append((bt, ot))  # (the counter reads them on its own stream until finish)
                c.add_tensors(bt, ot)
        c.finish()
        t = c.fetch()
        st = {key: v for key, v in c.stats().items() if np.isscalar(v)}
        np.savez(Path(out_dir) / f"{case['name']}_rank{rank}.npz", keys=t.keys, counts=t.counts, left=t.left,
                 right=t.right, **{f"st_{key}": v for key, v in st.items()})
        c.close()
        del keep
        # the case's switches back to their defaults before the next one
        N.debug_reset()
        for key in env:
            if not key.startswith("knob:"):
                os.environ.pop(key, None)
        dist.barrier()
    dist.destroy_process_group()
