"""GPU: quantized_reduce_scatter and quantized_all_gather with ``clip_steps=`` and the real HIP kernels.  Two or three processes share the one GPU
over gloo; each rank must equal, bit for bit, a simulation made of the clip model (tests/clip_model.py) and the group model, all ranks end
identical after the all-gather, and ``clip_steps=None`` reproduces the bytes of the simulation without the search
(tests/grouped_scatter_sim.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle as O
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu

G, STEPS = 128, 9


def _rank_input(rank, numel, fdt):
    sys.path.insert(0, os.path.dirname(__file__))
    import clip_cases as CC

    return CC.as_input(CC.spiky_gaussian(numel, 2100 + rank, G), O.BF16 if fdt == "bfloat16" else O.F32)


def _worker(rank, world, port, numel, fdt, qname):
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for p in (str(root), str(root / "pi-quant_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        torch.cuda.set_device(0)
        x = _rank_input(rank, numel, fdt)
        qdtype = getattr(torch, qname)

        def fresh():
            return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy()).cuda()

        def host(t):
            torch.cuda.synchronize()
            return t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy()

        out = []
        for steps in (STEPS, None):
            t = fresh()
            D.quantized_reduce_scatter(t, quant_dtype=qdtype, group_size=G, clip_steps=steps)
            out.append(host(t))
            D.quantized_all_gather(t, quant_dtype=qdtype, group_size=G, clip_steps=steps)
            out.append(host(t))
        return out
    finally:
        dist.destroy_process_group()


def _simulate(xs, dt, qd, chunks, steps):
    """-> (after the reduce-scatter, after the all-gather) per rank: tests/grouped_scatter_sim.py's two schedules with the clipped encode"""
    import clip_model as M
    from grouped_model import dequantize_grouped

    W = len(xs)
    rs = [x.copy() for x in xs]
    for c, (b, e) in enumerate(chunks):
        if e == b:
            continue
        acc = xs[c][b:e].copy()
        for src in range(W):
            if src != c:
                q, s, z, _ = M.quantize_grouped_clipped(xs[src][b:e], dt, qd, G, steps)
                acc = dequantize_grouped(q, qd, dt, e - b, G, s, z, O.ADD, prev=acc)
        rs[c][b:e] = acc
    ag = [x.copy() for x in rs]
    for c, (b, e) in enumerate(chunks):
        if e == b:
            continue
        q, s, z, _ = M.quantize_grouped_clipped(rs[c][b:e], dt, qd, G, steps)
        final = dequantize_grouped(q, qd, dt, e - b, G, s, z)
        for o in ag:
            o[b:e] = final
    return rs, ag


@pytest.mark.parametrize("world,numel,fdt,qname", [(2, 40_007, "float32", "quint2x4"), (3, 30_003, "bfloat16", "quint4x2")])
def test_clipped_reduce_scatter_and_all_gather_with_hip_kernels(oracle_mod, world, numel, fdt, qname):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_scatter_sim import simulate_all_gather, simulate_reduce_scatter

    assert world <= 3   # the ranks share the one GPU; every wait is bounded and ended by the first rank that fails
    results = run_ranks(world, _worker, (numel, fdt, qname), timeout=300)
    qd, bits = {"quint2x4": (O.UINT2, 2), "quint4x2": (O.UINT4, 4)}[qname]
    dt = O.BF16 if fdt == "bfloat16" else O.F32
    u = np.uint16 if dt == O.BF16 else np.uint32
    chunks = D.ring_chunks(numel, world, bits)
    xs = [_rank_input(r, numel, fdt) for r in range(world)]
    want_rs, want_ag = _simulate(xs, dt, qd, chunks, STEPS)
    plain_rs, _ = simulate_reduce_scatter(xs, dt, qd, chunks, G)
    plain_ag, _ = simulate_all_gather(plain_rs, dt, qd, chunks, G)
    assert not np.array_equal(want_ag[0].view(u), plain_ag[0].view(u))   # the search changes the bytes: the comparison below means something
    for r in range(world):
        rs, ag, rs_none, ag_none = results[r]
        assert np.array_equal(rs.view(u), want_rs[r].view(u)), f"rank {r}: clipped reduce-scatter differs from the simulation"
        assert np.array_equal(ag.view(u), want_ag[r].view(u)), f"rank {r}: clipped all-gather differs from the simulation"
        assert np.array_equal(ag.view(u), results[0][1].view(u)), f"rank {r} does not end identical to rank 0"
        assert np.array_equal(rs_none.view(u), plain_rs[r].view(u)), f"rank {r}: clip_steps=None changed the reduce-scatter"
        assert np.array_equal(ag_none.view(u), plain_ag[r].view(u)), f"rank {r}: clip_steps=None changed the all-gather"
