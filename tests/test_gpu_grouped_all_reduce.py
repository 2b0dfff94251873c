"""GPU: quantized_all_reduce(group_size=128) with the real HIP kernels.  Two or three processes share the one GPU over gloo (the schedule and
every kernel are the real ones, so each rank must equal the grouped simulation of tests/grouped_ring_sim.py bit for bit), and a one-rank RCCL
group runs the whole schedule through RCCL's collectives (its result is the grouped round trip of the tensor)."""
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


def _rank_input(rank, numel, fdt, outliers=0):
    """float32 values of rank `rank` (bf16 bit patterns as uint16 when fdt is bf16), and the float32 view of them."""
    x = np.random.default_rng(700 + rank).uniform(-1, 1, numel).astype(np.float32)
    if outliers:
        idx = np.random.default_rng(900 + rank).choice(numel, outliers, replace=False)
        x[idx] = np.where(np.arange(outliers) % 2 == 0, 1000.0, -1000.0).astype(np.float32)
    if fdt == "bfloat16":
        b = O.f32_to_bf16(x)
        return b, O.bf16_to_f32(b)
    return x, x


def _worker(rank, world, port, numel, fdt, qname, algorithm, group_sizes, outliers):
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
        x, _ = _rank_input(rank, numel, fdt, outliers)
        outs = []
        for gs in group_sizes:
            if fdt == "bfloat16":
                t = torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16)
            else:
                t = torch.from_numpy(x.copy()).cuda()
            D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=gs)
            outs.append(t)
        torch.cuda.synchronize()
        return [t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy() for t in outs]
    finally:
        dist.destroy_process_group()


def _spawn(world, args):
    """the ranks share the one GPU: at most 3 of them, every wait bounded and ended by the first rank that fails"""
    assert world <= 3
    return run_ranks(world, _worker, args, timeout=300)


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world,numel,fdt,qname", [(2, 300_007, "float32", "uint8"), (3, 200_003, "bfloat16", "quint4x2"),
                                                   (3, 150_001, "float32", "quint4x2"), (2, 100_003, "bfloat16", "uint8")])
def test_grouped_all_reduce_with_hip_kernels(oracle_mod, world, numel, fdt, qname, algorithm):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import simulate_direct_grouped, simulate_ring_grouped

    results = _spawn(world, (numel, fdt, qname, algorithm, [G], 3))
    qd, bits = {"uint8": (O.UINT8, 8), "quint4x2": (O.UINT4, 4)}[qname]
    dt = O.BF16 if fdt == "bfloat16" else O.F32
    xs = [_rank_input(r, numel, fdt, 3)[0] for r in range(world)]
    want = (simulate_ring_grouped if algorithm == "ring" else simulate_direct_grouped)(xs, dt, qd, D.ring_chunks(numel, world, bits), G)
    for r in range(world):
        got = results[r][0]
        assert np.array_equal(got.view(np.uint16 if dt == O.BF16 else np.uint32), want[r].view(np.uint16 if dt == O.BF16 else np.uint32)), r
        assert np.array_equal(got.view(np.uint8), results[0][0].view(np.uint8)), r


def test_grouped_all_reduce_beats_per_chunk_parameters_on_outliers(oracle_mod):
    """The point of the change: ranks of uniform(-1, 1) values with a few +-1000 planted.  A quint4x2 all-reduce with group_size=128 has at least
    4x lower mean absolute error than with group_size=None, against the exact fp32 sum over the elements outside the outliers' groups."""
    world, numel, outliers = 2, 1 << 20, 6
    results = _spawn(world, (numel, "float32", "quint4x2", "direct", [G, None], outliers))
    xs = [_rank_input(r, numel, "float32", outliers)[1] for r in range(world)]
    exact = np.sum(np.stack(xs).astype(np.float64), axis=0)
    keep = np.ones(numel, dtype=bool)
    for x in xs:
        for i in np.flatnonzero(np.abs(x) > 2):
            keep[(i // G) * G: (i // G + 1) * G] = False
    grouped, per_chunk = results[0]
    err_g = np.abs(grouped[keep] - exact[keep]).mean()
    err_t = np.abs(per_chunk[keep] - exact[keep]).mean()
    assert err_g * 4 <= err_t, (err_g, err_t)


@pytest.fixture(scope="module")
def pg():
    port = free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("fdt,qname,numel", [(torch.float32, "uint8", 1_000_003), (torch.bfloat16, "quint4x2", 300_001), (torch.float32, "quint2x4", 4099)])
def test_grouped_all_reduce_on_a_one_rank_rccl_group(pg, oracle_mod, algorithm, fdt, qname, numel):
    """The whole grouped schedule with RCCL as the transport (test hook: the rank is its own only peer): the result is the grouped round trip."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import round_trip_grouped

    qd = {"uint8": O.UINT8, "quint4x2": O.UINT4, "quint2x4": O.UINT2}[qname]
    g = torch.Generator(device="cuda")
    g.manual_seed(12)
    x = (torch.empty(numel, device="cuda").uniform_(-1, 1, generator=g) * torch.linspace(0.1, 10, numel, device="cuda")).to(fdt)
    host = x.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == torch.bfloat16 else x.cpu().numpy()
    dt = O.BF16 if fdt == torch.bfloat16 else O.F32
    t = x.clone()
    D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, _single_rank_collectives=True)
    torch.cuda.synchronize()
    want = round_trip_grouped(host, dt, qd, G)
    got = t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == torch.bfloat16 else t.cpu().numpy()
    assert np.array_equal(got.view(np.uint16 if dt == O.BF16 else np.uint32), want.view(np.uint16 if dt == O.BF16 else np.uint32))
