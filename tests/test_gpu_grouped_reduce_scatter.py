"""GPU: quantized_reduce_scatter and quantized_all_gather with the real HIP kernels.  Two or three processes share the one GPU over gloo (the
schedules and every kernel are the real ones, so each rank must equal the simulation of tests/grouped_scatter_sim.py bit for bit, and the two
collectives one after the other must leave the bytes of quantized_all_reduce(algorithm='direct', group_size=128) run in the same workers), and
a one-rank RCCL group runs both schedules through RCCL's collectives."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle as O
from rank_procs import free_port, run_ranks

pytestmark = pytest.mark.gpu

G = 128


def _rank_input(rank, numel, fdt):
    x = np.random.default_rng(1700 + rank).uniform(-1, 1, numel).astype(np.float32)
    idx = np.random.default_rng(1900 + rank).choice(numel, 3, replace=False)
    x[idx] = np.array([1000.0, -1000.0, 1000.0], dtype=np.float32)
    return O.f32_to_bf16(x) if fdt == "bfloat16" else x


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
            return t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy()

        b, e = D.ring_chunks(numel, world, D.torch_to_piquant_dtype(qdtype).bit_size)[rank]
        t = fresh()
        view = D.quantized_reduce_scatter(t, quant_dtype=qdtype, group_size=G)
        is_view = view.numel() == e - b and view.data_ptr() == t.view(-1)[b:e].data_ptr()
        torch.cuda.synchronize()
        scattered = host(t)
        D.quantized_all_gather(t, quant_dtype=qdtype, group_size=G)
        a = fresh()
        D.quantized_all_reduce(a, quant_dtype=qdtype, algorithm="direct", group_size=G)
        torch.cuda.synchronize()
        return is_view, scattered, host(t), host(a)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,numel,fdt,qname", [(2, 300_007, "float32", "uint8"), (3, 200_003, "bfloat16", "quint4x2")])
def test_reduce_scatter_and_all_gather_with_hip_kernels(oracle_mod, world, numel, fdt, qname):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_scatter_sim import simulate_all_gather, simulate_reduce_scatter

    assert world <= 3   # the ranks share the one GPU; every wait is bounded and ended by the first rank that fails
    results = run_ranks(world, _worker, (numel, fdt, qname), timeout=300)
    qd, bits = {"uint8": (O.UINT8, 8), "quint4x2": (O.UINT4, 4)}[qname]
    dt = O.BF16 if fdt == "bfloat16" else O.F32
    u = np.uint16 if dt == O.BF16 else np.uint32
    chunks = D.ring_chunks(numel, world, bits)
    xs = [_rank_input(r, numel, fdt) for r in range(world)]
    want_rs, _ = simulate_reduce_scatter(xs, dt, qd, chunks, G)
    want_both, _ = simulate_all_gather(want_rs, dt, qd, chunks, G)
    for r in range(world):
        is_view, scattered, both, all_reduce = results[r]
        assert is_view, r
        assert np.array_equal(scattered.view(u), want_rs[r].view(u)), f"rank {r}: reduce-scatter differs from the simulation"
        assert np.array_equal(both.view(u), want_both[r].view(u)), f"rank {r}: all-gather differs from the simulation"
        assert np.array_equal(both.view(u), all_reduce.view(u)), f"rank {r}: reduce-scatter + all-gather != quantized_all_reduce(direct)"
        assert np.array_equal(both.view(u), results[0][2].view(u)), r


@pytest.fixture(scope="module")
def pg():
    port = free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_a_one_rank_rccl_group(pg, oracle_mod):
    """Both schedules with RCCL as the transport (test hook: the rank is its own only peer).  The reduce-scatter has no peer record to add and
    leaves the tensor as it is; the all-gather leaves the grouped round trip."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import round_trip_grouped

    numel = 300_001
    g = torch.Generator(device="cuda")
    g.manual_seed(12)
    x = torch.empty(numel, device="cuda").uniform_(-1, 1, generator=g) * torch.linspace(0.1, 10, numel, device="cuda")
    t = x.clone()
    v = D.quantized_reduce_scatter(t, quant_dtype=torch.quint4x2, group_size=G, _single_rank_collectives=True)
    torch.cuda.synchronize()
    assert v.data_ptr() == t.data_ptr() and v.numel() == numel and torch.equal(t, x)
    assert D.quantized_all_gather(t, quant_dtype=torch.quint4x2, group_size=G, _single_rank_collectives=True) is t
    torch.cuda.synchronize()
    want = round_trip_grouped(x.cpu().numpy(), O.F32, O.UINT4, G)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
