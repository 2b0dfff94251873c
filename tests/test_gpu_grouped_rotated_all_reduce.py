"""GPU: piquant.distributed's four collectives with rotation_seed= and the real HIP kernels.  Two or three processes share the one GPU over gloo:
the schedules and every kernel are the real ones, so each rank must equal the simulation of tests/grouped_rotated_sim.py bit for bit and all
ranks must agree; a one-rank RCCL group runs the schedules through RCCL's collectives."""
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
SEED = 0x1234_5678_8765_4321
CASES = [(2, 300_007, "float32", "uint8"), (3, 200_003, "bfloat16", "quint4x2")]


def _rank_input(rank, numel, fdt):
    x = np.random.default_rng(2700 + rank).standard_normal(numel).astype(np.float32)
    idx = np.random.default_rng(2900 + rank).choice(numel, numel // 200, replace=False)
    x[idx] *= 40.0   # heavy tails: what the rotation is for
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

        kw = dict(quant_dtype=qdtype, group_size=G, rotation_seed=SEED)
        out = {}
        for algorithm in ("ring", "direct"):
            t = fresh()
            D.quantized_all_reduce(t, algorithm=algorithm, **kw)
            torch.cuda.synchronize()
            out[algorithm] = host(t)
        t = fresh()
        D.quantized_reduce_scatter(t, **kw)
        torch.cuda.synchronize()
        out["scatter"] = host(t)
        D.quantized_all_gather(t, **kw)
        torch.cuda.synchronize()
        out["both"] = host(t)
        return out
    finally:
        dist.destroy_process_group()


_RESULTS = {}


def _results(case):
    if case not in _RESULTS:   # the ranks run once per case
        assert case[0] <= 3    # the ranks share the one GPU; every wait is bounded and ended by the first rank that fails
        _RESULTS[case] = run_ranks(case[0], _worker, case[1:], timeout=300)
    return _RESULTS[case]


def _sim():
    sys.path.insert(0, os.path.dirname(__file__))
    import grouped_rotated_sim as S

    return S


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_rotated_collectives_with_hip_kernels(oracle_mod, case):
    import piquant.distributed as D

    S = _sim()
    world, numel, fdt, qname = case
    results = _results(case)
    qd, bits = {"uint8": (O.UINT8, 8), "quint4x2": (O.UINT4, 4)}[qname]
    dt = O.BF16 if fdt == "bfloat16" else O.F32
    u = np.uint16 if dt == O.BF16 else np.uint32
    chunks = D.ring_chunks(numel, world, bits)
    xs = [_rank_input(r, numel, fdt) for r in range(world)]
    want = {"ring": S.simulate_ring_rotated(xs, dt, qd, chunks, G, SEED), "direct": S.simulate_direct_rotated(xs, dt, qd, chunks, G, SEED),
            "scatter": S.simulate_reduce_scatter_rotated(xs, dt, qd, chunks, G, SEED)}
    want["both"] = S.simulate_all_gather_rotated(want["scatter"], dt, qd, chunks, G, SEED)
    for r in range(world):
        for name in ("ring", "direct", "scatter", "both"):
            assert np.array_equal(results[r][name].view(u), want[name][r].view(u)), f"rank {r}: {name} differs from the simulation"
        for name in ("ring", "direct", "both"):
            assert np.array_equal(results[r][name].view(u), results[0][name].view(u)), f"rank {r}: {name} differs from rank 0"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_reduce_scatter_then_all_gather_leaves_the_bytes_of_the_direct_all_reduce(oracle_mod, case):
    """Bit for bit, on every rank, with the HIP kernels: the direct schedule's owner step in the rotated domain is the reduce-scatter's step
    followed by the all-gather's encode (tests/test_grouped_rotated_collectives_cpu.py has the reason)."""
    results = _results(case)
    u = np.uint16 if case[2] == "bfloat16" else np.uint32
    for r in range(case[0]):
        differing = int(np.sum(results[r]["both"].view(u) != results[r]["direct"].view(u)))
        print(f"rank {r}: {differing} of {case[1]} words differ")
        assert differing == 0, r


@pytest.fixture(scope="module")
def pg():
    port = free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_a_one_rank_rccl_group(pg, oracle_mod):
    """The four schedules with RCCL as the transport (test hook: the rank is its own only peer).  The all-reduces and the all-gather leave the
    rotated round trip of the tensor; the reduce-scatter has no peer record to add and leaves the tensor as it is."""
    import piquant.distributed as D
    import rot_model as RM

    numel = 300_001
    x = _rank_input(0, numel, "float32")
    q, s, z = RM.quantize_grouped_rotated(x, O.F32, O.UINT4, G, SEED)
    want = RM.dequantize_grouped_rotated(q, O.UINT4, O.F32, numel, G, s, z, SEED)
    kw = dict(quant_dtype=torch.quint4x2, group_size=G, rotation_seed=SEED, _single_rank_collectives=True)
    for algorithm in ("ring", "direct"):
        t = torch.from_numpy(x).cuda()
        assert D.quantized_all_reduce(t, algorithm=algorithm, **kw) is t
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32)), algorithm
    t = torch.from_numpy(x).cuda()
    v = D.quantized_reduce_scatter(t, **kw)
    torch.cuda.synchronize()
    assert v.data_ptr() == t.data_ptr() and v.numel() == numel and np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert D.quantized_all_gather(t, **kw) is t
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
