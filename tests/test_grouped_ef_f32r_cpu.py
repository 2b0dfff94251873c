"""CPU: the float32 residual for bfloat16 tensors -- the ABI and the Python surface exist and accept exactly that pair beside equal dtypes, the
model conserves to float32 precision, and quantized_all_reduce(bf16 tensor, group_size=G, error_feedback=float32 residual) runs both schedules
with the flag on and off (wire ops from the oracle: tests/grouped_ef_f32r_sim.py; tests/test_gpu_grouped_ef_f32r*.py run the HIP ones)."""
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
SYMBOLS = {"piquant_hip_quantize_grouped_ef_mixed": 12, "piquant_hip_quantize_grouped_ef_mixed_batch": 13,
           "piquant_hip_reduce_quantize_grouped_ef_mixed": 16}


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    import piquant
    from piquant._bootstrap import C_LIB, library_path

    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for symbol, nargs in SYMBOLS.items():
        assert re.search(r"PIQUANT_EXPORT\s+void\s+" + symbol + r"\s*\(", header), f"{symbol} is not declared in piquant_hip.h"
        assert len(getattr(C_LIB, symbol).argtypes) == nargs, symbol
        assert symbol in exported, f"libpiquant.so does not export {symbol}"
    import inspect

    for name in ("quantize_grouped_ef_ptr", "quantize_grouped_ef_batch_ptr", "reduce_quantize_grouped_ef_ptr"):
        p = inspect.signature(getattr(piquant.Context, name)).parameters
        assert "residual_dtype" in p and p["residual_dtype"].default is None, name


def _calls(x, r):
    """the three wrappers on one (tensor, residual) pair"""
    import piquant.torch as pt

    return [lambda: pt.quantize_grouped_ef(x, r, dtype=torch.uint8),
            lambda: pt.quantize_grouped_ef_batch([x], [r], dtype=torch.quint4x2),
            lambda: pt.reduce_quantize_grouped_ef(x, r, [], [], [], dtype=torch.quint2x4)]


def test_wrappers_accept_a_float32_residual_for_a_bfloat16_tensor():
    """Host tensors: the pair passes every argument check and the call ends at the refusal to run without a device, which comes after them."""
    x = torch.zeros(1000, dtype=torch.bfloat16)
    r = torch.zeros(1000, dtype=torch.float32)
    for call in _calls(x, r):
        with pytest.raises(ValueError, match="ROCm"):
            call()
    for call in _calls(x, torch.zeros(999)):   # the other checks still apply to the pair
        with pytest.raises(ValueError, match="numel"):
            call()


@pytest.mark.parametrize("xdt,rdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.bfloat16, torch.float64),
                                     (torch.float32, torch.float16), (torch.float32, torch.float64)])
def test_every_other_pair_of_dtypes_is_refused(xdt, rdt):
    for call in _calls(torch.zeros(1000, dtype=xdt), torch.zeros(1000, dtype=rdt)):
        with pytest.raises(ValueError, match="dtype"):
            call()


def test_a_batch_shares_one_residual_dtype():
    import piquant.torch as pt

    xs = [torch.zeros(256, dtype=torch.bfloat16) for _ in range(2)]
    for rdts in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        with pytest.raises(ValueError, match="dtype"):
            pt.quantize_grouped_ef_batch(xs, [torch.zeros(256, dtype=d) for d in rdts], dtype=torch.uint8)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["UINT8", "UINT4", "UINT2"])
def test_model_is_the_float32_step_on_the_widened_tensor_and_conserves_to_float32_precision(oracle_mod, qname):
    """K = 16 chained steps: S = sum d_t + r_K - sum widen(x_t) stays within K 2^-23 M (two float32 roundings of half an ulp per step)."""
    sys.path.insert(0, os.path.dirname(__file__))
    from ef_f32r_model import ef_f32r_step
    from ef_model import conservation_defect, ef_step, widen

    O = oracle_mod
    qd, G, n, K = getattr(O, qname), 64, 1000, 16
    rng = np.random.default_rng(77)
    xs = [O.f32_to_bf16(rng.uniform(-1, 1, n).astype(np.float32)) for _ in range(K)]
    r = np.zeros(n, dtype=np.float32)
    ds, ys = [], []
    for t, x in enumerate(xs):
        q, s, z, r_new, y, d = ef_f32r_step(x, r, qd, G)
        if t == 0:
            want = ef_step(widen(x, O.BF16), r, O.F32, qd, G)
            assert all(np.array_equal(a, b) for a, b in zip((q, s, z, r_new.view(np.uint32)), (want[0], want[1], want[2], want[3].view(np.uint32))))
        assert r_new.dtype == np.float32 and y.dtype == np.float32
        r = r_new
        ds.append(d)
        ys.append(y)
    defect, bound = conservation_defect([widen(x, O.BF16) for x in xs], ds, r, ys, O.F32)
    print(f"{qname}: max|S| = {defect:.4g}, bound = {bound:.4g}")
    assert defect <= bound, (defect, bound)


# ---- the all-reduce ---------------------------------------------------------------------------------------------------------------------
QDTYPES = {"uint8": 8, "quint4x2": 4, "quint2x4": 2}
SENTINEL = np.float32(1.2345e-12)   # finite, and far below every quantization step here
STEPS = 2
# (numel, wire, group size, requantize): 5000 elements, and 4000, which leaves the last rank an empty chunk
CONFIGS = [(5000, "uint8", 128, False), (5000, "quint4x2", 64, True), (4000, "quint4x2", 128, False), (4000, "uint8", 128, True)]


def _inputs(O, world, numel, step):
    xs = [np.random.default_rng(300 + 17 * step + r).uniform(-1, 1, numel).astype(np.float32) for r in range(world)]
    for r, x in enumerate(xs):   # one outlier per rank, in different groups
        x[(r * 7919 + 13 + step) % numel] = 50.0 * (1 if r % 2 else -1)
    return [O.f32_to_bf16(x) for x in xs]


def _worker(rank, world, port, algorithm):
    sys.path.insert(0, os.path.dirname(__file__))
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import oracle as O
        import piquant.distributed as D
        from grouped_ef_f32r_sim import GroupedEfF32rOracleOps, bf16_bits, bf16_tensor

        got = []
        for numel, qname, G, requantize in CONFIGS:
            residual = torch.full((numel,), float(SENTINEL))
            outs = []
            for step in range(STEPS):
                x = bf16_tensor(_inputs(O, world, numel, step)[rank])
                D.quantized_all_reduce(x, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, error_feedback=residual,
                                       error_feedback_requantize=requantize, _ops=GroupedEfF32rOracleOps())
                outs.append(bf16_bits(x))
            got.append((outs, residual.numpy().copy()))
        return got
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world", [2, 3])
def test_all_reduce_of_a_bfloat16_tensor_with_a_float32_residual_equals_the_simulation(oracle_mod, world, algorithm):
    """Two consecutive all-reduces carrying the residual, flag on and off: results and residuals of every rank equal the simulation bit for
    bit; with the flag off the slices the schedule does not use keep their sentinel, with it on none does."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ef_f32r_sim import simulate_f32r
    from grouped_ef_sim import untouched_slices

    O = oracle_mod
    results = run_ranks(world, _worker, (algorithm,), timeout=240)
    empty_seen = False
    for i, (numel, qname, G, requantize) in enumerate(CONFIGS):
        chunks = D.ring_chunks(numel, world, QDTYPES[qname])
        empty_seen = empty_seen or any(e == b for b, e in chunks)
        qd = {8: O.UINT8, 4: O.UINT4, 2: O.UINT2}[QDTYPES[qname]]
        rs = [np.full(numel, SENTINEL, dtype=np.float32) for _ in range(world)]
        for step in range(STEPS):
            want, rs = simulate_f32r(algorithm, _inputs(O, world, numel, step), rs, qd, chunks, G, requantize)
            for r in range(world):
                assert np.array_equal(results[r][i][0][step], want[r]), (numel, qname, requantize, step, r)
        for r in range(world):
            res = results[r][i][1]
            assert res.dtype == np.float32 and np.array_equal(res.view(np.uint32), rs[r].view(np.uint32)), (numel, qname, requantize, r)
            idle = untouched_slices(chunks, r, algorithm)
            for c, (b, e) in enumerate(chunks):
                if not requantize and (b, e) in idle:
                    assert np.all(res[b:e] == SENTINEL), (r, b, e)
                else:
                    assert not np.any(res[b:e] == SENTINEL), f"rank {r}: chunk {c} of the residual was not used"
    assert empty_seen, "one of the sizes leaves a rank an empty chunk"


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def _args_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_ef_f32r_sim import GroupedEfF32rOracleOps

        n = 5000
        good = torch.zeros(n, dtype=torch.float32)
        bad16 = torch.zeros(n, dtype=torch.float16)
        bad64 = torch.zeros(n, dtype=torch.float64)
        cases = [(torch.bfloat16, dict(error_feedback=bad16, group_size=128)),
                 (torch.bfloat16, dict(error_feedback=bad64, group_size=128, algorithm="direct")),
                 (torch.float32, dict(error_feedback=torch.zeros(n, dtype=torch.bfloat16), group_size=128)),
                 (torch.bfloat16, dict(error_feedback=torch.zeros(n - 1), group_size=128)),
                 (torch.bfloat16, dict(error_feedback=good)),                                                   # the per-chunk wire
                 (torch.bfloat16, dict(error_feedback=good, group_size=128, algorithm="direct", transport="p2p")),
                 (torch.bfloat16, dict(error_feedback=good, group_size=128, algorithm="direct", error_feedback_requantize=True))]   # the good call last
        seen = []
        for xdt, kwargs in cases:
            x = torch.ones(n, dtype=xdt)
            try:
                D.quantized_all_reduce(x, quant_dtype=torch.uint8, _ops=GroupedEfF32rOracleOps(), **kwargs)
                seen.append(("no error", True))
            except (ValueError, RuntimeError) as exc:
                seen.append((type(exc).__name__ + ": " + str(exc), bool((x == 1).all()) and bool((good == 0).all())))
        return seen
    finally:
        dist.destroy_process_group()


def test_a_bad_residual_raises_on_every_rank_before_anything_moves():
    results = run_ranks(2, _args_worker, (), timeout=240)
    for r in range(2):
        msgs = [m for m, _ in results[r]]
        for i in (0, 1, 2):
            assert msgs[i].startswith("ValueError") and "dtype" in msgs[i], msgs[i]
        assert msgs[3].startswith("ValueError") and "numel" in msgs[3], msgs[3]
        assert msgs[4].startswith("ValueError") and "group_size" in msgs[4], msgs[4]
        assert msgs[5].startswith("ValueError") and "p2p" in msgs[5], msgs[5]
        assert msgs[6] == "no error", msgs[6]
        assert all(ok for _, ok in results[r]), results[r]
