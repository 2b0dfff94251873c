"""GPU: piquant.distributed.compute_quant_params_clipped over two ranks that share the one GPU over gloo, with uneven shards: the MIN all-reduce of
the keys, each rank's histogram against the global keys, one SUM all-reduce of the counts, the search.  Both ranks must return exactly what the
single call on the whole tensor returns, which is the CPU model's (tests/clip_params_model.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle as O
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu

NUMEL, CUT = 90_001, 31_337   # rank 0 holds [0, CUT), rank 1 the rest: uneven, and the second shard starts off a 16-byte boundary
CASES = [("float32", "quint2x4", 63), ("bfloat16", "quint4x2", 63), ("float32", "quint8", 17)]


def _whole(fdt):
    sys.path.insert(0, os.path.dirname(__file__))
    import clip_params_model as M

    return M.as_input(np.random.default_rng(77).standard_normal(NUMEL).astype(np.float32), O.BF16 if fdt == "bfloat16" else O.F32)


def _tensor(x, fdt):
    return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy()).cuda()


def _worker(rank, world, port):
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for p in (str(root), str(root / "pi-quant_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        import piquant.torch as pt

        torch.cuda.set_device(0)
        out = []
        for fdt, qname, steps in CASES:
            x = _whole(fdt)
            shard = x[:CUT] if rank == 0 else x[CUT:]
            sharded = D.compute_quant_params_clipped(_tensor(shard, fdt), dtype=getattr(torch, qname), steps=steps)
            single = pt.compute_quant_params_clipped(_tensor(x, fdt), dtype=getattr(torch, qname), steps=steps)
            out.append((sharded, single))
        return out
    finally:
        dist.destroy_process_group()


def test_two_uneven_shards_give_the_single_call_result(oracle_mod):
    sys.path.insert(0, os.path.dirname(__file__))
    import clip_params_model as M

    results = run_ranks(2, _worker, (), timeout=300)
    for i, (fdt, qname, steps) in enumerate(CASES):
        dt = O.BF16 if fdt == "bfloat16" else O.F32
        qd = {"quint2x4": O.UINT2, "quint4x2": O.UINT4, "quint8": O.UINT8}[qname]
        s, z, k, _, _ = M.compute_quant_params_clipped(_whole(fdt), dt, qd, steps)
        if steps == 63:
            assert k > 0, "the search must have something to choose in this case"
        for rank in (0, 1):
            sharded, single = results[rank][i]
            assert sharded == single == (float(s), z), f"{fdt} {qname} rank {rank}: sharded {sharded}, single {single}, model {(float(s), z)}"
