"""GPU: piquant.distributed's four collectives with rotated_error_feedback= and the real HIP kernels.  Two or three processes share the one GPU
over gloo: the schedules and every kernel are the real ones, so over two consecutive calls (the residual carried over) each rank must equal the
simulation of tests/grouped_rotated_ef_sim.py bit for bit in tensor AND residual, and all ranks must agree; a one-rank RCCL group runs the
schedules through RCCL's collectives."""
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
CALLS = 2
CASES = [(2, 40_007, "float32", "quint4x2"), (3, 30_005, "bfloat16", "uint8")]
RUNS = (("ring", "ring", False), ("ring-rq", "ring", True), ("direct", "direct", False), ("direct-rq", "direct", True))


def _rank_input(rank, call, numel, fdt):
    x = np.random.default_rng(3700 + 10 * call + rank).standard_normal(numel).astype(np.float32)
    idx = np.random.default_rng(3900 + 10 * call + rank).choice(numel, numel // 200, replace=False)
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
        qdtype = getattr(torch, qname)

        def tensor(call):
            x = _rank_input(rank, call, numel, fdt)
            return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy()).cuda()

        def host(t):
            return t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy()

        kw = dict(quant_dtype=qdtype, group_size=G, rotation_seed=SEED)
        out = {}
        for name, algorithm, requantize in RUNS:
            r, steps = torch.zeros(numel, device="cuda"), []
            for call in range(CALLS):
                t = tensor(call)
                D.quantized_all_reduce(t, algorithm=algorithm, rotated_error_feedback=r, error_feedback_requantize=requantize, **kw)
                torch.cuda.synchronize()
                steps.append((host(t), r.cpu().numpy()))
            out[name] = steps
        r, scatter, both = torch.zeros(numel, device="cuda"), [], []
        for call in range(CALLS):
            t = tensor(call)
            D.quantized_reduce_scatter(t, rotated_error_feedback=r, **kw)
            torch.cuda.synchronize()
            scatter.append((host(t), r.cpu().numpy()))
            D.quantized_all_gather(t, rotated_error_feedback=r, **kw)
            torch.cuda.synchronize()
            both.append((host(t), r.cpu().numpy()))
        out["scatter"], out["both"] = scatter, both
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
    import grouped_rotated_ef_sim as ES

    return ES


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_rotated_ef_collectives_with_hip_kernels(oracle_mod, case):
    import piquant.distributed as D

    ES = _sim()
    world, numel, fdt, qname = case
    assert numel % G != 0
    results = _results(case)
    qd, bits = {"uint8": (O.UINT8, 8), "quint4x2": (O.UINT4, 4)}[qname]
    dt = O.BF16 if fdt == "bfloat16" else O.F32
    u = np.uint16 if dt == O.BF16 else np.uint32
    chunks = D.ring_chunks(numel, world, bits)
    zeros = [np.zeros(numel, dtype=np.float32) for _ in range(world)]
    want = {}
    for name, algorithm, requantize in RUNS:
        sim = ES.simulate_ring_rotated_ef if algorithm == "ring" else ES.simulate_direct_rotated_ef
        rs, steps = zeros, []
        for call in range(CALLS):
            outs, rs = sim([_rank_input(r, call, numel, fdt) for r in range(world)], rs, dt, qd, chunks, G, SEED, requantize)
            steps.append((outs, rs))
        want[name] = steps
    rs, scatter, both = zeros, [], []
    for call in range(CALLS):
        outs, rs = ES.simulate_reduce_scatter_rotated_ef([_rank_input(r, call, numel, fdt) for r in range(world)], rs, dt, qd, chunks, G, SEED)
        scatter.append((outs, rs))
        outs, rs = ES.simulate_all_gather_rotated_ef(outs, rs, dt, qd, chunks, G, SEED)
        both.append((outs, rs))
    want["scatter"], want["both"] = scatter, both
    for r in range(world):
        for name, steps in want.items():
            for call, (outs, res) in enumerate(steps):
                got_t, got_r = results[r][name][call]
                assert np.array_equal(got_t.view(u), outs[r].view(u)), f"rank {r}, call {call}: {name}: the tensor differs from the simulation"
                assert np.array_equal(got_r.view(np.uint32), res[r].view(np.uint32)), f"rank {r}, call {call}: {name}: the residual differs from the simulation"
                if name != "scatter":
                    assert np.array_equal(got_t.view(u), results[0][name][call][0].view(u)), f"rank {r}, call {call}: {name} differs from rank 0"
        assert np.any(results[r]["ring"][CALLS - 1][1] != 0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_reduce_scatter_then_all_gather_is_the_direct_all_reduce_with_requantize(oracle_mod, case):
    """tensor bytes and residual bytes, on every rank, after each of the two calls, with the HIP kernels"""
    results = _results(case)
    for r in range(case[0]):
        for call in range(CALLS):
            (bt, br), (dt_, dr) = results[r]["both"][call], results[r]["direct-rq"][call]
            assert np.array_equal(bt.view(np.uint8), dt_.view(np.uint8)), (r, call, "tensor")
            assert np.array_equal(br.view(np.uint32), dr.view(np.uint32)), (r, call, "residual")


@pytest.fixture(scope="module")
def pg():
    port = free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_a_one_rank_rccl_group(pg, oracle_mod):
    """The four schedules with RCCL as the transport (test hook: the rank is its own only peer).  The ring's one encode and the all-gather's feed
    the rank's only chunk of the residual; the mesh's owner encode feeds it only with error_feedback_requantize; the reduce-scatter has no peer
    chunk to encode and leaves tensor and residual as they are."""
    import piquant.distributed as D
    import rot_ef_model as RE
    import rot_model as RM

    numel = 30_001
    x = _rank_input(0, 0, numel, "float32")
    r0 = (_rank_input(0, 1, numel, "float32") * np.float32(0.01)).astype(np.float32)
    q, s, z, r1, _, _ = RE.quantize_grouped_rotated_ef(x, O.F32, r0, O.UINT4, G, SEED)
    fed = RM.dequantize_grouped_rotated(q, O.UINT4, O.F32, numel, G, s, z, SEED)
    q, s, z = RM.quantize_grouped_rotated(x, O.F32, O.UINT4, G, SEED)
    unfed = RM.dequantize_grouped_rotated(q, O.UINT4, O.F32, numel, G, s, z, SEED)
    kw = dict(quant_dtype=torch.quint4x2, group_size=G, rotation_seed=SEED, _single_rank_collectives=True)

    def run(fn, **extra):
        t, r = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(r0.copy()).cuda()
        fn(t, rotated_error_feedback=r, **kw, **extra)
        torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32), r.cpu().numpy().view(np.uint32)

    for requantize in (False, True):
        t, r = run(D.quantized_all_reduce, algorithm="ring", error_feedback_requantize=requantize)
        assert np.array_equal(t, fed.view(np.uint32)) and np.array_equal(r, r1.view(np.uint32)), ("ring", requantize)
    t, r = run(D.quantized_all_reduce, algorithm="direct")
    assert np.array_equal(t, unfed.view(np.uint32)) and np.array_equal(r, r0.view(np.uint32))
    t, r = run(D.quantized_all_reduce, algorithm="direct", error_feedback_requantize=True)
    assert np.array_equal(t, fed.view(np.uint32)) and np.array_equal(r, r1.view(np.uint32))
    t, r = run(D.quantized_reduce_scatter)
    assert np.array_equal(t, x.view(np.uint32)) and np.array_equal(r, r0.view(np.uint32))
    t, r = run(D.quantized_all_gather)
    assert np.array_equal(t, fed.view(np.uint32)) and np.array_equal(r, r1.view(np.uint32))
