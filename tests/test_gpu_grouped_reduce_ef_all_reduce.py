"""GPU: quantized_all_reduce(group_size=128, error_feedback=residual, error_feedback_requantize=True) with the real HIP kernels.  Two or three
processes share the one GPU over gloo: two consecutive all-reduces with the residual carried over must equal the simulation of
tests/grouped_reduce_ef_sim.py bit for bit on every rank, every rank must hold the same result, and no chunk of any residual keeps the sentinel it
started from.  A one-rank RCCL group runs the mesh's owner step with zero terms through the test hook: quantize_grouped_ef of the whole tensor."""
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
STEPS = 2
SENTINEL = np.float32(2.0 ** -40)   # exact in bfloat16, finite, and far below every quantization step here


def _sentinel(dt):
    return O.f32_to_bf16(np.array([SENTINEL], dtype=np.float32))[0] if dt == O.BF16 else SENTINEL


def _rank_input(rank, numel, fdt, step):
    x = np.random.default_rng(1700 + 31 * step + rank).uniform(-1, 1, numel).astype(np.float32)
    idx = np.random.default_rng(1900 + 31 * step + rank).choice(numel, 3, replace=False)
    x[idx] = np.array([1000.0, -1000.0, 1000.0], dtype=np.float32)
    return O.f32_to_bf16(x) if fdt == "bfloat16" else x


def _initial_residual(numel, dt):
    res = np.zeros(numel, dtype=np.uint16 if dt == O.BF16 else np.float32)
    res[:] = _sentinel(dt)
    return res


def _to_device(a, fdt):
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(a.copy()).cuda()


def _to_host(t, fdt):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy()


def _worker(rank, world, port, numel, fdt, qname, algorithm):
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for p in (str(root), str(root / "pi-quant_amd"), str(root / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        torch.cuda.set_device(0)
        dt = O.BF16 if fdt == "bfloat16" else O.F32
        residual = _to_device(_initial_residual(numel, dt), fdt)
        outs = []
        for step in range(STEPS):
            t = _to_device(_rank_input(rank, numel, fdt, step), fdt)
            D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, error_feedback=residual,
                                   error_feedback_requantize=True)
            outs.append(t)
        torch.cuda.synchronize()
        return [_to_host(t, fdt) for t in outs], _to_host(residual, fdt)
    finally:
        dist.destroy_process_group()


CASES = [(2, 300_007, "float32", "quint4x2", O.UINT4, 4), (3, 200_003, "bfloat16", "quint2x4", O.UINT2, 2)]


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world,numel,fdt,qname,qd,bits", CASES)
def test_all_reduce_with_error_feedback_on_every_quantization(oracle_mod, world, numel, fdt, qname, qd, bits, algorithm):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_reduce_ef_sim import simulate_direct_grouped_ef_all, simulate_ring_grouped_ef_all

    assert world <= 3   # the ranks share the one GPU
    results = run_ranks(world, _worker, (numel, fdt, qname, algorithm), timeout=300)
    dt = O.BF16 if fdt == "bfloat16" else O.F32
    view = np.uint16 if dt == O.BF16 else np.uint32
    chunks = D.ring_chunks(numel, world, bits)
    sim = simulate_ring_grouped_ef_all if algorithm == "ring" else simulate_direct_grouped_ef_all
    rs = [_initial_residual(numel, dt) for _ in range(world)]
    for step in range(STEPS):
        want, rs = sim([_rank_input(r, numel, fdt, step) for r in range(world)], rs, dt, qd, chunks, G)
        for r in range(world):
            got = results[r][0][step]
            assert np.array_equal(got.view(view), want[r].view(view)), (step, r)
            assert np.array_equal(got.view(np.uint8), results[0][0][step].view(np.uint8)), (step, r)
    for r in range(world):
        got = results[r][1]
        assert np.array_equal(got.view(view), rs[r].view(view)), r
        for c, (b, e) in enumerate(chunks):
            assert not np.any(got[b:e] == _sentinel(dt)), f"rank {r}: chunk {c} of the residual was not used"


@pytest.fixture(scope="module")
def pg():
    port = free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("fdt,qname,qd,numel", [(torch.float32, "quint4x2", O.UINT4, 300_001), (torch.bfloat16, "quint2x4", O.UINT2, 4099)])
def test_one_rank_rccl_group_mesh(pg, oracle_mod, fdt, qname, qd, numel):
    """Under the test hook the mesh has no peers to encode for and its owner step has zero terms.  With the flag on that step is
    quantize_grouped_ef of the whole tensor: it WRITES the residual, and two all-reduces are two steps of the error-feedback model.  With the flag
    off the residual stays untouched and the result is the grouped round trip, as before.  Without the hook a one-rank group returns at once."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from ef_model import ef_step
    from grouped_model import dequantize_grouped
    from grouped_ring_sim import round_trip_grouped

    dt = O.BF16 if fdt == torch.bfloat16 else O.F32
    name = "bfloat16" if dt == O.BF16 else "float32"
    view = np.uint16 if dt == O.BF16 else np.uint32
    res0 = _initial_residual(numel, dt)
    res = _to_device(res0, name)
    t = _to_device(_rank_input(0, numel, name, 0), name)
    before = _to_host(t, name).copy()
    D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm="direct", group_size=G, error_feedback=res, error_feedback_requantize=True)
    torch.cuda.synchronize()
    assert np.array_equal(_to_host(t, name).view(view), before.view(view)) and np.array_equal(_to_host(res, name).view(view), res0.view(view))

    # flag off: today's behaviour
    x = _rank_input(0, numel, name, 0)
    t = _to_device(x, name)
    D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm="direct", group_size=G, error_feedback=res, _single_rank_collectives=True)
    torch.cuda.synchronize()
    assert np.array_equal(_to_host(t, name).view(view), round_trip_grouped(x, dt, qd, G).view(view))
    assert np.array_equal(_to_host(res, name).view(view), res0.view(view)), "the flag is off: the residual must stay untouched"

    # flag on: two steps of the model
    r_model = np.zeros(numel, dtype=res0.dtype)
    res = _to_device(r_model, name)
    for step in range(STEPS):
        x = _rank_input(0, numel, name, step)
        t = _to_device(x, name)
        D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm="direct", group_size=G, error_feedback=res,
                               error_feedback_requantize=True, _single_rank_collectives=True)
        torch.cuda.synchronize()
        q, s, z, r_model, _, _ = ef_step(x, r_model, dt, qd, G)
        want = dequantize_grouped(q, qd, dt, numel, G, s, z)
        assert np.array_equal(_to_host(t, name).view(view), want.view(view)), step
        assert np.array_equal(_to_host(res, name).view(view), r_model.view(view)), step
    assert np.any(r_model != 0)
