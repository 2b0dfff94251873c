"""CPU: error-feedback group-wise quantization -- the ABI and the Python surface exist and check their arguments, the CPU model
(tests/ef_model.py) conserves what it quantizes, and quantized_all_reduce(group_size=G, error_feedback=residual) runs both schedules with the
residual on exactly the slices a rank quantizes itself (wire ops from the oracle: tests/grouped_ef_sim.py; tests/test_gpu_grouped_ef*.py run
the HIP ones)."""
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
NEW_SYMBOLS = ("piquant_hip_quantize_grouped_ef", "piquant_hip_quantize_grouped_ef_batch")


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r"PIQUANT_EXPORT\s+void\s+" + name + r"\s*\(", header), f"{name} is not declared in piquant_hip.h"
    import piquant
    from piquant._bootstrap import C_LIB, library_path

    for name in NEW_SYMBOLS:
        assert getattr(C_LIB, name).argtypes is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, f"libpiquant.so does not export {name}"
    assert callable(piquant.Context.quantize_grouped_ef_ptr) and callable(piquant.Context.quantize_grouped_ef_batch_ptr)


def test_torch_wrappers_refuse_bad_arguments():
    """Every refusal is a ValueError raised in Python, before a native call could abort (host tensors: nothing here touches a device)."""
    import piquant.torch as pt

    x = torch.zeros(1000)
    r = torch.zeros(1000)
    with pytest.raises(ValueError, match="dtype"):
        pt.quantize_grouped_ef(x, r.to(torch.bfloat16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="numel"):
        pt.quantize_grouped_ef(x, torch.zeros(999), dtype=torch.uint8)
    with pytest.raises(ValueError, match="device"):
        pt.quantize_grouped_ef(x, torch.zeros(1000, device="meta"), dtype=torch.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        pt.quantize_grouped_ef(x, torch.zeros(2000)[::2], dtype=torch.uint8)
    with pytest.raises(ValueError, match="Tensor"):
        pt.quantize_grouped_ef(x, None, dtype=torch.uint8)
    for bad in (100, 16, 8192, None, 128.0, True):
        with pytest.raises(ValueError, match="group_size"):
            pt.quantize_grouped_ef(x, r, dtype=torch.uint8, group_size=bad)
        with pytest.raises(ValueError, match="group_size"):
            pt.quantize_grouped_ef_batch([x], [r], dtype=torch.uint8, group_size=bad)
    with pytest.raises(ValueError, match="quantized dtype"):
        pt.quantize_grouped_ef(x, r, dtype=torch.float32)
    with pytest.raises(ValueError, match="round_mode"):
        pt.quantize_grouped_ef(x, r, dtype=torch.uint8, round_mode="up")
    with pytest.raises(ValueError, match="ROCm"):
        pt.quantize_grouped_ef(x, r, dtype=torch.uint8)          # a matching residual, but host tensors
    with pytest.raises(ValueError, match="empty"):
        pt.quantize_grouped_ef_batch([], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="same length"):
        pt.quantize_grouped_ef_batch([x, x], [r], dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"residuals\[1\].*numel"):
        pt.quantize_grouped_ef_batch([x, x], [r, torch.zeros(7)], dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"residuals\[0\].*contiguous"):
        pt.quantize_grouped_ef_batch([x], [torch.zeros(2000)[::2]], dtype=torch.uint8)
    with pytest.raises(ValueError, match="both"):
        pt.quantize_grouped_ef(x, r, dtype=torch.uint8, out_scales=torch.zeros(8))
    with pytest.raises(ValueError, match="ROCm"):
        pt.quantize_grouped_ef_batch([x], [r], dtype=torch.uint8)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _chain_inputs(n, G, K, seed):
    rng = np.random.default_rng(seed)
    fixed = (rng.standard_normal(n) * 3.0).astype(np.float32)
    fixed[G: 2 * G] = 7.25                                           # one constant group, far from zero
    xs = []
    for t in range(K):
        if t % 2 == 0:
            xs.append(fixed.copy())
        else:
            xs.append((rng.standard_normal(n) * np.repeat(rng.uniform(0.01, 50.0, n // 97 + 1), 97)[:n]).astype(np.float32))
    return xs


@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
@pytest.mark.parametrize("qd_name", ["UINT8", "UINT4", "UINT2"])
def test_model_conserves_what_it_quantizes(oracle_mod, dt_name, qd_name):
    """K = 32 chained steps: sum of what was sent + the last residual - sum of the inputs stays within K eps_T M (two roundings to T per step)."""
    sys.path.insert(0, os.path.dirname(__file__))
    from ef_model import conservation_defect, ef_step, narrow

    O = oracle_mod
    dt, qd = (O.F32 if dt_name == "f32" else O.BF16), getattr(O, qd_name)
    n, G, K = 1000, 128, 32
    xs = [narrow(x, dt) for x in _chain_inputs(n, G, K, 77)]
    r = narrow(np.zeros(n, dtype=np.float32), dt)
    ds, ys = [], []
    for x in xs:
        _, _, _, r, y, d = ef_step(x, r, dt, qd, G)
        ds.append(d)
        ys.append(y)
    defect, bound = conservation_defect(xs, ds, r, ys, dt)
    print(f"{dt_name} {qd_name}: max|S| = {defect:.3g}, bound = {bound:.3g}")
    assert defect <= bound, (defect, bound)


def test_model_properties_of_the_parameter_epilogue(oracle_mod):
    """Documented, not fixed: a constant group gets the degenerate (1.0, qmax >> 1), so a group of 7.25 sends 7 (fp32 / uint8: 134 - 127) and
    keeps 0.25; a group whose range lies far from zero has its zero point clamped and most of its mass stays in the residual."""
    sys.path.insert(0, os.path.dirname(__file__))
    from ef_model import ef_step

    O = oracle_mod
    G = 128
    x = np.full(2 * G, 7.25, dtype=np.float32)
    x[G:] += np.linspace(-0.01, 0.01, G, dtype=np.float32)           # second group: values near 7.25, a narrow range far from zero
    q, s, z, r, y, d = ef_step(x, np.zeros_like(x), O.F32, O.UINT8, G)
    assert (float(s[0]), int(z[0])) == (1.0, 127)
    assert np.all(d[:G] + r[:G] == x[:G])
    assert np.all(np.abs(r[G:]) > 6.5), "a group far from zero is carried by the residual"
    assert np.allclose(d[G:].astype(np.float64) + r[G:], x[G:], rtol=0, atol=1e-5)


# ---- the all-reduce ---------------------------------------------------------------------------------------------------------------------
QDTYPES = {"uint8": 8, "quint4x2": 4, "quint2x4": 2}
SENTINEL = np.float32(-12345.5)


def _inputs(world, numel, step):
    xs = [np.random.default_rng(300 + 17 * step + r).uniform(-1, 1, numel).astype(np.float32) for r in range(world)]
    for r, x in enumerate(xs):   # one outlier per rank, in different groups
        x[(r * 7919 + 13 + step) % numel] = 50.0 * (1 if r % 2 else -1)
    return xs


def _initial_residual(world, numel, chunks, algorithm):
    """Zeros where the schedule applies error feedback, a sentinel where it must not look."""
    from grouped_ef_sim import untouched_slices

    rs = []
    for r in range(world):
        res = np.zeros(numel, dtype=np.float32)
        for b, e in untouched_slices(chunks, r, algorithm):
            res[b:e] = SENTINEL
        rs.append(res)
    return rs


def _ef_worker(rank, world, port, numel, qname, algorithm, G, steps, with_residual):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_ef_sim import GroupedEfOracleOps

        chunks = D.ring_chunks(numel, world, QDTYPES[qname])
        residual = torch.from_numpy(_initial_residual(world, numel, chunks, algorithm)[rank]) if with_residual else None
        outs = []
        for step in range(steps):
            x = torch.from_numpy(_inputs(world, numel, step)[rank])
            D.quantized_all_reduce(x, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, error_feedback=residual,
                                   _ops=GroupedEfOracleOps())
            outs.append(x.numpy().copy())
        return outs, (residual.numpy().copy() if with_residual else None)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world,numel,qname,G", [(2, 12_345, "uint8", 128), (3, 20_001, "quint4x2", 128), (3, 9_001, "quint2x4", 64)])
def test_all_reduce_schedules_with_error_feedback(oracle_mod, world, numel, qname, G, algorithm):
    """Two consecutive all-reduces with the residual carried over: every rank equals the simulation byte for byte, the residual too, and the
    slices of the residual that the schedule does not quantize keep their sentinel."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ef_sim import simulate_direct_grouped_ef, simulate_ring_grouped_ef, untouched_slices

    O = oracle_mod
    steps = 2
    results = run_ranks(world, _ef_worker, (numel, qname, algorithm, G, steps, True), timeout=240)
    bits = QDTYPES[qname]
    qd = {8: O.UINT8, 4: O.UINT4, 2: O.UINT2}[bits]
    chunks = D.ring_chunks(numel, world, bits)
    sim = simulate_ring_grouped_ef if algorithm == "ring" else simulate_direct_grouped_ef
    rs = _initial_residual(world, numel, chunks, algorithm)
    for step in range(steps):
        want, rs = sim(_inputs(world, numel, step), rs, O.F32, qd, chunks, G)
        for r in range(world):
            assert np.array_equal(results[r][0][step].view(np.uint32), want[r].view(np.uint32)), (step, r)
            assert np.array_equal(results[r][0][step].view(np.uint32), results[0][0][step].view(np.uint32)), (step, r)
    for r in range(world):
        assert np.array_equal(results[r][1].view(np.uint32), rs[r].view(np.uint32)), r
        for b, e in untouched_slices(chunks, r, algorithm):
            assert np.all(results[r][1][b:e] == SENTINEL), (r, b, e)
        touched = np.ones(numel, dtype=bool)
        for b, e in untouched_slices(chunks, r, algorithm):
            touched[b:e] = False
        assert np.any(results[r][1][touched] != 0), "the residual was never written"


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
def test_error_feedback_none_is_the_existing_grouped_path(oracle_mod, algorithm):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import simulate_direct_grouped, simulate_ring_grouped

    O = oracle_mod
    world, numel, qname, G = 2, 12_345, "quint4x2", 128
    results = run_ranks(world, _ef_worker, (numel, qname, algorithm, G, 1, False), timeout=240)
    sim = simulate_ring_grouped if algorithm == "ring" else simulate_direct_grouped
    want = sim(_inputs(world, numel, 0), O.F32, O.UINT4, D.ring_chunks(numel, world, 4), G)
    for r in range(world):
        assert np.array_equal(results[r][0][0].view(np.uint32), want[r].view(np.uint32)), r


def _args_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_ef_sim import GroupedEfOracleOps

        n = 5000
        good = torch.zeros(n)
        cases = [dict(error_feedback=good), dict(error_feedback=good, group_size=128, algorithm="direct", transport="p2p"),
                 dict(error_feedback=good, group_size=128, algorithm="ring", transport="p2p"),
                 dict(error_feedback=torch.zeros(n, dtype=torch.bfloat16), group_size=128), dict(error_feedback=torch.zeros(n - 1), group_size=128),
                 dict(error_feedback=torch.zeros(2 * n)[::2], group_size=128), dict(error_feedback=torch.zeros(n, device="meta"), group_size=128),
                 dict(error_feedback=good, group_size=100), dict(error_feedback=good, group_size=128, algorithm="ring")]   # the good call last
        seen = []
        for kwargs in cases:
            x = torch.ones(n)
            try:
                D.quantized_all_reduce(x, quant_dtype=torch.uint8, _ops=GroupedEfOracleOps(), **kwargs)
                seen.append("no error")
            except (ValueError, RuntimeError) as exc:
                seen.append(type(exc).__name__ + ": " + str(exc))
            seen.append(bool((x == 1).all()) and bool((good == 0).all()) if seen[-1] != "no error" else None)
        direct = []
        for kwargs in (dict(error_feedback=torch.zeros(10)), dict(error_feedback=torch.zeros(10), group_size=128, transport="p2p"),
                       dict(error_feedback=torch.zeros(9), group_size=128)):
            try:
                D.quantized_all_reduce_direct(torch.ones(10), quant_dtype=torch.uint8, _ops=GroupedEfOracleOps(), **kwargs)
                direct.append("no error")
            except ValueError as exc:
                direct.append("ValueError: " + str(exc))
        return seen, direct
    finally:
        dist.destroy_process_group()


def test_error_feedback_arguments_are_checked_before_anything_moves():
    """error_feedback without group_size or with transport='p2p', and a residual of the wrong dtype / numel / layout / device, raise ValueError on
    every rank alike with the tensor and the residual untouched; a good call goes through."""
    results = run_ranks(2, _args_worker, (), timeout=240)
    for r in range(2):
        seen, direct = results[r]
        msgs, untouched = seen[0::2], seen[1::2]
        assert msgs[0].startswith("ValueError") and "group_size" in msgs[0], msgs[0]
        assert msgs[1].startswith("ValueError") and "p2p" in msgs[1], msgs[1]
        assert msgs[2].startswith("ValueError"), msgs[2]
        assert msgs[3].startswith("ValueError") and "dtype" in msgs[3], msgs[3]
        assert msgs[4].startswith("ValueError") and "numel" in msgs[4], msgs[4]
        assert msgs[5].startswith("ValueError") and "contiguous" in msgs[5], msgs[5]
        assert msgs[6].startswith("ValueError") and "device" in msgs[6], msgs[6]
        assert msgs[7].startswith("ValueError") and "group_size" in msgs[7], msgs[7]
        assert msgs[8] == "no error", msgs[8]
        assert all(u for m, u in zip(msgs, untouched) if m != "no error")
        assert direct[0].startswith("ValueError") and "group_size" in direct[0]
        assert direct[1].startswith("ValueError") and "p2p" in direct[1]
        assert direct[2].startswith("ValueError") and "numel" in direct[2]


def test_a_one_rank_group_leaves_the_residual_alone():
    results = run_ranks(1, _one_rank_worker, (), timeout=120)
    assert results[0] is True


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
            D.quantized_all_reduce(x, quant_dtype=torch.quint4x2, algorithm=algorithm, group_size=128, error_feedback=res)
            ok = ok and bool((res == 3.0).all()) and bool((x == torch.arange(5000, dtype=torch.float32)).all())
        return ok
    finally:
        dist.destroy_process_group()
