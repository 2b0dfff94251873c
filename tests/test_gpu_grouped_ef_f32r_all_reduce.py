"""GPU: quantized_all_reduce(bfloat16 tensor, group_size=128, error_feedback=float32 residual[, error_feedback_requantize=True]) with the real
HIP kernels.  Two or three processes share the one GPU over gloo: two consecutive all-reduces with the residual carried over must equal the
simulation of tests/grouped_ef_f32r_sim.py bit for bit on every rank, in results and residuals."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle as O
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu

G = 128
STEPS = 2
SENTINEL = np.float32(2.0 ** -40)   # finite, and far below every quantization step here


def _rank_input(rank, numel, step):
    x = np.random.default_rng(2700 + 31 * step + rank).uniform(-1, 1, numel).astype(np.float32)
    idx = np.random.default_rng(2900 + 31 * step + rank).choice(numel, 3, replace=False)
    x[idx] = np.array([1000.0, -1000.0, 1000.0], dtype=np.float32)
    return O.f32_to_bf16(x)


def _worker(rank, world, port, numel, qname, algorithm, requantize):
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
        residual = torch.full((numel,), float(SENTINEL), dtype=torch.float32, device="cuda")
        outs = []
        for step in range(STEPS):
            t = torch.from_numpy(_rank_input(rank, numel, step).view(np.int16)).cuda().view(torch.bfloat16)
            D.quantized_all_reduce(t, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, error_feedback=residual,
                                   error_feedback_requantize=requantize)
            outs.append(t)
        torch.cuda.synchronize()
        return [t.view(torch.int16).cpu().numpy().view(np.uint16) for t in outs], residual.cpu().numpy()
    finally:
        dist.destroy_process_group()


# a few chunks of 4096 elements plus a ragged end
CASES = [(2, 5 * 4096 + 1003, "uint8", O.UINT8, 8), (3, 7 * 4096 + 77, "quint4x2", O.UINT4, 4)]


@pytest.mark.parametrize("requantize", [False, True])
@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world,numel,qname,qd,bits", CASES)
def test_all_reduce_of_a_bfloat16_tensor_with_a_float32_residual(oracle_mod, world, numel, qname, qd, bits, algorithm, requantize):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ef_f32r_sim import simulate_f32r
    from grouped_ef_sim import untouched_slices

    assert world <= 3   # the ranks share the one GPU
    results = run_ranks(world, _worker, (numel, qname, algorithm, requantize), timeout=300)
    chunks = D.ring_chunks(numel, world, bits)
    rs = [np.full(numel, SENTINEL, dtype=np.float32) for _ in range(world)]
    for step in range(STEPS):
        want, rs = simulate_f32r(algorithm, [_rank_input(r, numel, step) for r in range(world)], rs, qd, chunks, G, requantize)
        for r in range(world):
            got = results[r][0][step]
            assert np.array_equal(got, want[r]), (step, r, np.flatnonzero(got != want[r])[:8])
            assert np.array_equal(got, results[0][0][step]), (step, r)
    for r in range(world):
        got = results[r][1]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), rs[r].view(np.uint32)), (r, np.flatnonzero(got != rs[r])[:8])
        idle = untouched_slices(chunks, r, algorithm)
        for c, (b, e) in enumerate(chunks):
            if not requantize and (b, e) in idle:
                assert np.all(got[b:e] == SENTINEL), (r, b, e)
            else:
                assert not np.any(got[b:e] == SENTINEL), f"rank {r}: chunk {c} of the residual was not used"
