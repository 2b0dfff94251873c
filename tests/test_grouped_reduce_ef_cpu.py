"""CPU: error feedback on re-quantized partial sums -- the ABI and the Python surface exist and check their arguments, and
quantized_all_reduce(group_size=G, error_feedback=residual, error_feedback_requantize=True) runs both schedules with the residual on EVERY
quantization (wire ops from the oracle: tests/grouped_reduce_ef_sim.py; tests/test_gpu_grouped_reduce_ef*.py run the HIP ones), which is what
makes the all-reduce conservative over steps."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks

ROOT = Path(__file__).resolve().parent.parent
SYMBOL = "piquant_hip_reduce_quantize_grouped_ef"


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    assert re.search(r"PIQUANT_EXPORT\s+void\s+" + SYMBOL + r"\s*\(", header), f"{SYMBOL} is not declared in piquant_hip.h"
    import piquant
    import piquant.torch as pt
    from piquant._bootstrap import C_LIB, library_path

    assert len(getattr(C_LIB, SYMBOL).argtypes) == 15
    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert SYMBOL in exported, f"libpiquant.so does not export {SYMBOL}"
    assert callable(piquant.Context.reduce_quantize_grouped_ef_ptr) and callable(pt.reduce_quantize_grouped_ef)
    assert "quantize_grouped_ef(acc, residual)" in pt.reduce_quantize_grouped_ef.__doc__, "the docstring states the two-call identity"


def test_torch_wrapper_refuses_bad_arguments():
    """Every refusal is a ValueError raised in Python, before a native call could abort (host tensors: nothing here touches a device)."""
    import piquant.torch as pt

    acc = torch.zeros(1000)
    r = torch.zeros(1000)
    q = torch.zeros(1000, dtype=torch.uint8)
    sc, zp = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    f = pt.reduce_quantize_grouped_ef
    with pytest.raises(ValueError, match="dtype"):
        f(acc, r.to(torch.bfloat16), [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="numel"):
        f(acc, torch.zeros(999), [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="device"):
        f(acc, torch.zeros(1000, device="meta"), [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        f(acc, torch.zeros(2000)[::2], [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="Tensor"):
        f(acc, None, [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="same length"):
        f(acc, r, [q, q], [sc], [zp, zp], dtype=torch.uint8)
    with pytest.raises(ValueError, match="same length"):
        f(acc, r, [q], [sc], [], dtype=torch.uint8)
    for bad in (100, 16, 8192, None, 128.0, True):
        with pytest.raises(ValueError, match="group_size"):
            f(acc, r, [q], [sc], [zp], dtype=torch.uint8, group_size=bad)
    with pytest.raises(ValueError, match="quantized dtype"):
        f(acc, r, [], [], [], dtype=torch.float32)
    with pytest.raises(ValueError, match="round_mode"):
        f(acc, r, [], [], [], dtype=torch.uint8, round_mode="up")
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        f(acc.to(torch.float64), r.to(torch.float64), [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="ROCm"):
        f(acc, r, [], [], [], dtype=torch.uint8)                   # a matching residual, but host tensors


# ---- the all-reduce ---------------------------------------------------------------------------------------------------------------------
QDTYPES = {"uint8": 8, "quint4x2": 4, "quint2x4": 2}
SENTINEL = np.float32(1.2345e-12)   # finite, and far below every quantization step here: a slice that was used cannot end on it by accident


def _inputs(world, numel, step):
    xs = [np.random.default_rng(900 + 17 * step + r).uniform(-1, 1, numel).astype(np.float32) for r in range(world)]
    for r, x in enumerate(xs):   # one outlier per rank, in different groups
        x[(r * 7919 + 13 + step) % numel] = 50.0 * (1 if r % 2 else -1)
    return xs


def _worker(rank, world, port, numel, qname, algorithm, G, steps, requantize):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_reduce_ef_sim import GroupedReduceEfOracleOps

        residual = torch.full((numel,), float(SENTINEL))
        outs = []
        for step in range(steps):
            x = torch.from_numpy(_inputs(world, numel, step)[rank])
            D.quantized_all_reduce(x, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, error_feedback=residual,
                                   error_feedback_requantize=requantize, _ops=GroupedReduceEfOracleOps())
            outs.append(x.numpy().copy())
        return outs, residual.numpy().copy()
    finally:
        dist.destroy_process_group()


def _qd(O, qname):
    return {8: O.UINT8, 4: O.UINT4, 2: O.UINT2}[QDTYPES[qname]]


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world,numel,qname,G", [(2, 12_345, "uint8", 128), (3, 20_001, "quint4x2", 128), (3, 9_001, "quint2x4", 64),
                                                 (2, 9_001, "quint2x4", 128), (2, 12_345, "quint4x2", 64), (3, 13_001, "uint8", 64)])
def test_all_reduce_with_error_feedback_on_every_quantization(oracle_mod, world, numel, qname, G, algorithm):
    """Two consecutive all-reduces with the flag on and the residual carried over, from a residual filled with a sentinel: every rank equals the
    simulation and rank 0 bit for bit, the residual too, and no chunk of any rank's residual still holds the sentinel -- with the flag off the
    slices of grouped_ef_sim.untouched_slices would."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_reduce_ef_sim import simulate_direct_grouped_ef_all, simulate_ring_grouped_ef_all

    O = oracle_mod
    steps = 2
    results = run_ranks(world, _worker, (numel, qname, algorithm, G, steps, True), timeout=240)
    chunks = D.ring_chunks(numel, world, QDTYPES[qname])
    sim = simulate_ring_grouped_ef_all if algorithm == "ring" else simulate_direct_grouped_ef_all
    rs = [np.full(numel, SENTINEL, dtype=np.float32) for _ in range(world)]
    for step in range(steps):
        want, rs = sim(_inputs(world, numel, step), rs, O.F32, _qd(O, qname), chunks, G)
        for r in range(world):
            assert np.array_equal(results[r][0][step].view(np.uint32), want[r].view(np.uint32)), (step, r)
            assert np.array_equal(results[r][0][step].view(np.uint32), results[0][0][step].view(np.uint32)), (step, r)
    for r in range(world):
        assert np.array_equal(results[r][1].view(np.uint32), rs[r].view(np.uint32)), r
        assert np.all(np.isfinite(results[r][1]))
        for c, (b, e) in enumerate(chunks):
            assert not np.any(results[r][1][b:e] == SENTINEL), f"rank {r}: chunk {c} of the residual was not used"


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
def test_flag_off_is_the_existing_error_feedback_path(oracle_mod, algorithm):
    """error_feedback_requantize=False: the bytes of the existing simulation, and the slices it leaves alone keep the sentinel."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ef_sim import simulate_direct_grouped_ef, simulate_ring_grouped_ef, untouched_slices

    O = oracle_mod
    world, numel, qname, G, steps = 3, 20_001, "quint4x2", 128, 2
    results = run_ranks(world, _worker, (numel, qname, algorithm, G, steps, False), timeout=240)
    chunks = D.ring_chunks(numel, world, 4)
    sim = simulate_ring_grouped_ef if algorithm == "ring" else simulate_direct_grouped_ef
    rs = [np.full(numel, SENTINEL, dtype=np.float32) for _ in range(world)]
    for step in range(steps):
        want, rs = sim(_inputs(world, numel, step), rs, O.F32, O.UINT4, chunks, G)
        for r in range(world):
            assert np.array_equal(results[r][0][step].view(np.uint32), want[r].view(np.uint32)), (step, r)
    for r in range(world):
        assert np.array_equal(results[r][1].view(np.uint32), rs[r].view(np.uint32)), r
        for b, e in untouched_slices(chunks, r, algorithm):
            assert np.all(results[r][1][b:e] == SENTINEL), (r, b, e)


# ---- conservation: the point of the feature -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world", [2, 3])
def test_the_all_reduce_is_conservative_over_steps(oracle_mod, world, algorithm, dt_name):
    """K = 16 all-reduces of U(-1, 1) inputs over a quint4x2 wire, simulated in-process.  In float64,
        S = sum_t out_t + sum_ranks residual_final - sum_t sum_ranks x_t
    and with the flag on max|S| <= K (3W - 1)/2 eps_T M, M the largest magnitude among inputs, partial sums, y and d seen.  3W - 1 counts the
    roundings to T that an element meets per step, each off by at most eps_T / 2 relative to a value of magnitude <= M:
      mesh  W - 1 own-contribution encodes with two each (y = rn(x + r), r' = rn(y - d)); the owner's W - 1 term adds, its residual add and its
            subtraction: 2 (W - 1) + (W - 1) + 2 = 3W - 1;
      ring  two for the first encode, and per hop the term add, the residual add and the subtraction: 2 + 3 (W - 1) = 3W - 1.
    Everything else telescopes exactly: what a quantization sends is d, what it keeps is y - d, and the value a receiver adds is the sender's d.
    For float32 that last identity is exact (the receiver's dequantize ADD forms the same float32 d the sender subtracted).  For bfloat16 the
    sender subtracts d rounded to bfloat16 (what a dequantize SET stores) while a dequantize ADD adds the unrounded float32 product and rounds the
    sum once, so every received term is off by up to one more eps_T / 2 |d|: the worst case is 4W - 2 per step there.  The measured defect stays
    below the 3W - 1 bound for bfloat16 as well (the errors do not line up), so the test asserts 3W - 1 for both types.
    With the flag off the owner's (every hop's) rounding error is thrown away: the uint4 step alone loses about range / 30 per step, and max|S|
    exceeds the bound by orders of magnitude -- asserted too, so that the test cannot pass on a schedule that compensates nothing."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from ef_model import EPS, narrow, widen
    from grouped_ef_sim import simulate_direct_grouped_ef, simulate_ring_grouped_ef
    from grouped_reduce_ef_sim import simulate_direct_grouped_ef_all, simulate_ring_grouped_ef_all

    O = oracle_mod
    dt, qd = (O.F32 if dt_name == "f32" else O.BF16), O.UINT4
    numel, G, K = 5_003, 128, 16
    chunks = D.ring_chunks(numel, world, 4, align=1024)              # several non-empty chunks at a few thousand elements
    assert sum(1 for b, e in chunks if e > b) == world
    rng = np.random.default_rng(4242 + world)
    steps = [[narrow(rng.uniform(-1, 1, numel).astype(np.float32), dt) for _ in range(world)] for _ in range(K)]
    on = simulate_ring_grouped_ef_all if algorithm == "ring" else simulate_direct_grouped_ef_all
    off = simulate_ring_grouped_ef if algorithm == "ring" else simulate_direct_grouped_ef

    def defect(sim, seen):
        rs = [narrow(np.zeros(numel, dtype=np.float32), dt) for _ in range(world)]
        S = np.zeros(numel, dtype=np.float64)
        for xs in steps:
            outs, rs = sim(xs, rs, dt, qd, chunks, G, seen) if seen is not None else sim(xs, rs, dt, qd, chunks, G)
            for o in outs[1:]:
                assert np.array_equal(o, outs[0])
            S += widen(outs[0], dt).astype(np.float64)
            for x in xs:
                S -= widen(x, dt).astype(np.float64)
        for r in rs:
            S += widen(r, dt).astype(np.float64)
        return float(np.abs(S).max())

    seen = [max(float(np.abs(widen(x, dt)).max()) for xs in steps for x in xs)]
    d_on = defect(on, seen)
    M = max(seen)
    bound = K * (3 * world - 1) / 2 * EPS[dt] * M
    d_off = defect(off, None)
    print(f"W={world} {algorithm} {dt_name}: flag on max|S| = {d_on:.4g}, flag off max|S| = {d_off:.4g}, bound = {bound:.4g} (M = {M:.4g})")
    assert d_on <= bound, (d_on, bound)
    assert d_off > bound, (d_off, bound)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def _args_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_reduce_ef_sim import GroupedReduceEfOracleOps

        n = 5000
        good = torch.zeros(n)
        cases = [dict(group_size=128), dict(error_feedback=good), dict(),
                 dict(error_feedback=good, group_size=128, algorithm="direct", transport="p2p"),
                 dict(error_feedback=good, group_size=128, algorithm="ring", transport="p2p"),
                 dict(error_feedback=good, group_size=128, algorithm="ring")]   # the good call last
        seen = []
        for kwargs in cases:
            x = torch.ones(n)
            try:
                D.quantized_all_reduce(x, quant_dtype=torch.uint8, error_feedback_requantize=True, _ops=GroupedReduceEfOracleOps(), **kwargs)
                seen.append("no error")
            except (ValueError, RuntimeError) as exc:
                seen.append(type(exc).__name__ + ": " + str(exc))
            seen.append(bool((x == 1).all()) and bool((good == 0).all()) if seen[-1] != "no error" else True)
        direct = []
        for kwargs in (dict(group_size=128), dict(error_feedback=torch.zeros(10)), dict(error_feedback=torch.zeros(10), group_size=128, transport="p2p")):
            try:
                D.quantized_all_reduce_direct(torch.ones(10), quant_dtype=torch.uint8, error_feedback_requantize=True, _ops=GroupedReduceEfOracleOps(),
                                              **kwargs)
                direct.append("no error")
            except ValueError as exc:
                direct.append("ValueError: " + str(exc))
        return seen, direct
    finally:
        dist.destroy_process_group()


def test_requantize_arguments_are_checked_before_anything_moves():
    """error_feedback_requantize=True without error_feedback, without group_size or with transport='p2p' raises ValueError on every rank alike
    with the tensor and the residual untouched; a good call goes through."""
    results = run_ranks(2, _args_worker, (), timeout=240)
    for r in range(2):
        seen, direct = results[r]
        msgs, ok = seen[0::2], seen[1::2]
        assert msgs[0].startswith("ValueError") and "error_feedback" in msgs[0], msgs[0]
        assert msgs[1].startswith("ValueError") and "group_size" in msgs[1], msgs[1]
        assert msgs[2].startswith("ValueError"), msgs[2]
        assert msgs[3].startswith("ValueError") and "p2p" in msgs[3], msgs[3]
        assert msgs[4].startswith("ValueError"), msgs[4]
        assert msgs[5] == "no error", msgs[5]
        assert all(ok), ok
        assert direct[0].startswith("ValueError") and "error_feedback" in direct[0]
        assert direct[1].startswith("ValueError") and "group_size" in direct[1]
        assert direct[2].startswith("ValueError") and "p2p" in direct[2]


def _one_rank_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        ok = True
        for algorithm in ("ring", "direct"):
            x = torch.arange(5000, dtype=torch.float32)
            res = torch.full((5000,), 3.0)
            D.quantized_all_reduce(x, quant_dtype=torch.quint4x2, algorithm=algorithm, group_size=128, error_feedback=res, error_feedback_requantize=True)
            ok = ok and bool((res == 3.0).all()) and bool((x == torch.arange(5000, dtype=torch.float32)).all())
        return ok
    finally:
        dist.destroy_process_group()


def test_a_one_rank_group_leaves_the_residual_alone():
    results = run_ranks(1, _one_rank_worker, (), timeout=120)
    assert results[0] is True
