"""CPU: group-wise quantize-dequantize (piquant_hip_quantize_dequantize_grouped / _batch) -- the ABI and the Python surface exist and check their
arguments, and the CPU model the GPU test compares against, dequantize_grouped(quantize_grouped(x)) of tests/grouped_model.py, stays within the
half step that the quantization step allows (tests/test_gpu_grouped_requant.py runs the HIP kernels)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from grouped_edge_cases import edge_tensor, values

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("piquant_hip_quantize_dequantize_grouped", "piquant_hip_quantize_dequantize_grouped_batch")


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r"PIQUANT_EXPORT\s+void\s+" + name + r"\s*\(", header), f"{name} is not declared in piquant_hip.h"
    import piquant
    import piquant.torch as pt
    from piquant._bootstrap import C_LIB, library_path

    for name in NEW_SYMBOLS:
        assert getattr(C_LIB, name).argtypes is not None
    assert len(C_LIB.piquant_hip_quantize_dequantize_grouped.argtypes) == 12 and len(C_LIB.piquant_hip_quantize_dequantize_grouped_batch.argtypes) == 13
    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, f"libpiquant.so does not export {name}"
    assert callable(piquant.Context.quantize_dequantize_grouped_ptr) and callable(piquant.Context.quantize_dequantize_grouped_batch_ptr)
    assert callable(pt.quantize_dequantize_grouped) and callable(pt.quantize_dequantize_grouped_batch)


def test_torch_wrappers_refuse_bad_arguments():
    """Every refusal is a ValueError raised in Python, before a native call could abort (host and meta tensors: nothing here touches a device)."""
    import piquant.torch as pt

    x = torch.zeros(1000)
    m = torch.zeros(1000, device="meta")
    ng = pt.num_groups(1000, 128)
    sc, zp = torch.zeros(ng), torch.zeros(ng, dtype=torch.uint8)
    single, batch = pt.quantize_dequantize_grouped, pt.quantize_dequantize_grouped_batch
    for t in (x, m):
        # dtype of the tensor, quantized dtype
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            single(t.to(torch.float16), quant_dtype=torch.uint8)
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            batch([t, t.to(torch.float64)], quant_dtype=torch.uint8)
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            single(None, quant_dtype=torch.uint8)
        for bad in (torch.float32, torch.int8, None):
            with pytest.raises(ValueError, match="quantized dtype"):
                single(t, quant_dtype=bad)
            with pytest.raises(ValueError, match="quantized dtype"):
                batch([t], quant_dtype=bad)
        # group_size, round_mode, reduce_op
        for bad in (100, 16, 8192, None, 128.0, True):
            with pytest.raises(ValueError, match="group_size"):
                single(t, quant_dtype=torch.uint8, group_size=bad)
            with pytest.raises(ValueError, match="group_size"):
                batch([t], quant_dtype=torch.uint8, group_size=bad)
        with pytest.raises(ValueError, match="round_mode"):
            single(t, quant_dtype=torch.uint8, round_mode="up")
        with pytest.raises(ValueError, match="round_mode"):
            batch([t], quant_dtype=torch.uint8, round_mode="up")
        with pytest.raises(ValueError, match="reduce_op"):
            single(t, quant_dtype=torch.uint8, reduce_op="mul")
        with pytest.raises(ValueError, match="reduce_op"):
            batch([t], quant_dtype=torch.uint8, reduce_op="mul")
        with pytest.raises(ValueError, match="out="):
            single(t, quant_dtype=torch.uint8, reduce_op="add")
        with pytest.raises(ValueError, match="outs="):
            batch([t], quant_dtype=torch.uint8, reduce_op="add")
        # out: contiguity, numel, dtype, device
        with pytest.raises(ValueError, match="contiguous"):
            single(t, quant_dtype=torch.uint8, out=torch.zeros(2000, device=t.device)[::2])
        with pytest.raises(ValueError, match="1000 elements"):
            single(t, quant_dtype=torch.uint8, out=torch.zeros(999, device=t.device))
        with pytest.raises(ValueError, match="torch.float32"):
            single(t, quant_dtype=torch.uint8, out=torch.zeros(1000, dtype=torch.bfloat16, device=t.device))
        with pytest.raises(ValueError, match=r"outs\[1\].*contiguous"):
            batch([t, t], quant_dtype=torch.uint8, outs=[torch.zeros(1000, device=t.device), torch.zeros(2000, device=t.device)[::2]])
        with pytest.raises(ValueError, match=r"outs\[0\].*1000 elements"):
            batch([t], quant_dtype=torch.uint8, outs=[torch.zeros(7, device=t.device)])
        # list lengths
        with pytest.raises(ValueError, match="empty"):
            batch([], quant_dtype=torch.uint8)
        with pytest.raises(ValueError, match="same length"):
            batch([t, t], quant_dtype=torch.uint8, outs=[torch.zeros(1000, device=t.device)])
        with pytest.raises(ValueError, match="same length"):
            batch([t, t], quant_dtype=torch.uint8, scales=[sc], zero_points=[zp, zp])
        with pytest.raises(ValueError, match="one device and one dtype"):
            batch([t, t.to(torch.bfloat16)], quant_dtype=torch.uint8)
        # one of scales / zero_points without the other; their length and dtype
        with pytest.raises(ValueError, match="both"):
            single(t, quant_dtype=torch.uint8, scales=sc)
        with pytest.raises(ValueError, match="both"):
            single(t, quant_dtype=torch.uint8, zero_points=zp)
        with pytest.raises(ValueError, match="both"):
            batch([t], quant_dtype=torch.uint8, scales=[sc])
        with pytest.raises(ValueError, match=f"scales must be .* {ng} elements"):
            single(t, quant_dtype=torch.uint8, scales=torch.zeros(ng + 1), zero_points=zp)
        with pytest.raises(ValueError, match="scales must be .* float32"):
            single(t, quant_dtype=torch.uint8, scales=sc.double(), zero_points=zp)
        with pytest.raises(ValueError, match=f"zero_points must be .* {ng} elements"):
            single(t, quant_dtype=torch.uint8, scales=sc, zero_points=torch.zeros(ng - 1, dtype=torch.uint8))
        with pytest.raises(ValueError, match="zero_points must be .* uint8"):
            single(t, quant_dtype=torch.uint8, scales=sc, zero_points=zp.to(torch.int32))
        with pytest.raises(ValueError, match=f"scales must be .* {ng} elements"):
            batch([t], quant_dtype=torch.uint8, scales=[torch.zeros(3)], zero_points=[zp])
        # device / ROCm: everything else in order, but host or meta tensors
        with pytest.raises(ValueError, match="ROCm"):
            single(t, quant_dtype=torch.uint8)
        with pytest.raises(ValueError, match="ROCm"):
            single(t, quant_dtype=torch.quint4x2, out=t, reduce_op="add", return_params=True)
        with pytest.raises(ValueError, match="ROCm"):
            batch([t, t], quant_dtype=torch.quint2x4)
    with pytest.raises(ValueError, match="on cpu"):          # out on another device than the tensor
        single(x, quant_dtype=torch.uint8, out=m)
    with pytest.raises(ValueError, match="ROCm"):
        single(x, quant_dtype=torch.uint8, scales=sc, zero_points=zp)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
@pytest.mark.parametrize("qd_name", ["UINT8", "UINT4", "UINT2"])
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_model_round_trip_stays_within_half_a_step(oracle_mod, dt_name, qd_name, G):
    """d = dequantize_grouped(quantize_grouped(x)) of the model on edge_tensor, nearest rounding.  For every group that is non-degenerate (its
    parameters are not (1.0, qmax >> 1)), finite (no infinity) and non-constant (max != min), in exact arithmetic

        |x - d| <= scale / 2 + dist(x, [(0 - zp) scale, (qmax - zp) scale])

    The bound comes from the step, not from a measurement: the nearest code of x is at most half a step away, and a code is clamped to
    [0, qmax], which costs what x lies outside the codes' range.  For an element inside that range -- every element of a group whose zero point
    is not clamped, up to the half step that rounding the zero point moves the range by -- this is |x - d| <= scale / 2.  edge_tensor's
    far_pos / far_neg / line_* / unbounded_* groups are one-sided far from zero ON PURPOSE: their zero point clamps to 0 or qmax, every code
    saturates, and |x - d| is about |x|; the plain half-step bound cannot hold for them, the clamped one does.  Evaluated in
    float64 with one ulp of the output type at |d| added (the dequantized value and, for bfloat16, its one rounding).  A group whose scale is so
    small that fl(1 / scale) overflows (all_denormal: scale < 2^-128) quantizes x * inf and is left out: no step bounds that.
    NaNs: the quantizer gives a NaN a code like any other element, so after SET its position holds a code's value of its group (finite, inside
    the codes' range) -- it does not stay NaN; a NaN in an ADD accumulator does.  Both are asserted."""
    from grouped_model import QMAX, dequantize_grouped, quantize_grouped

    O = oracle_mod
    dt, qd = (O.F32 if dt_name == "f32" else O.BF16), getattr(O, qd_name)
    bits, lay = edge_tensor(dt, qd, G, 0)
    x = bits.view(np.float32) if dt == O.F32 else bits
    q, s, z = quantize_grouped(x, dt, qd, G)
    d = dequantize_grouped(q, qd, dt, x.size, G, s, z)
    with np.errstate(invalid="ignore"):
        xv = values(bits).astype(np.float64)
        dv = values(d.view(np.uint32) if dt == O.F32 else d).astype(np.float64)
    ulp = np.spacing(np.abs(dv).astype(np.float32)).astype(np.float64) if dt == O.F32 else np.maximum(np.abs(dv) * 2.0 ** -7, 2.0 ** -133)
    checked = plain = 0
    worst = 0.0
    for g in range(s.size):
        b, e = lay.bounds(g)
        xs, ds, scale, zp = xv[b:e], dv[b:e], float(s[g]), int(z[g])
        nan = np.isnan(xs)
        lo_rep, hi_rep = (0 - zp) * scale, (QMAX[qd] - zp) * scale
        if nan.any() and np.isfinite(scale):   # a NaN gets a code: a finite value inside the codes' range
            assert np.all(np.isfinite(ds[nan])) and np.all((ds[nan] >= lo_rep - ulp[b:e][nan]) & (ds[nan] <= hi_rep + ulp[b:e][nan])), lay.describe(g)
        degenerate = scale == 1.0 and zp == QMAX[qd] >> 1
        if degenerate or np.isinf(xs).any() or nan.all() or xs[~nan].max() == xs[~nan].min():
            continue
        with np.errstate(over="ignore"):
            inv = np.float32(1.0) / np.float32(scale)
        if not np.isfinite(inv):
            assert lay.cls[g] == "all_denormal", lay.describe(g)
            continue
        xs, ds, u = xs[~nan], ds[~nan], ulp[b:e][~nan]
        dist = np.maximum(0.0, np.maximum(lo_rep - xs, xs - hi_rep))
        err = np.abs(xs - ds)
        assert np.all(err <= scale / 2 + dist + u), f"{lay.describe(g)}: |x - d| exceeds scale / 2 by {float((err - scale / 2 - dist).max()):.3g}"
        checked += 1
        if not dist.any():
            plain += 1
            worst = max(worst, float((err / scale).max()))
    print(f"{dt_name} {qd_name} G={G}: {checked} groups checked, {plain} of them wholly inside the codes' range (largest |x - d| / scale = {worst:.6f})")
    assert plain >= 1 and checked > plain   # groups wholly inside their codes' range (ties, ordinary), and clamped ones (far_pos / far_neg)

    acc = x.copy()
    acc[[1, G + 3, x.size - 1]] = np.uint16(0x7FC0) if dt == O.BF16 else np.float32(np.nan)
    added = dequantize_grouped(q, qd, dt, x.size, G, s, z, O.ADD, prev=acc)
    with np.errstate(invalid="ignore"):
        av = values(added.view(np.uint32) if dt == O.F32 else added)
    assert np.all(np.isnan(av[[1, G + 3, x.size - 1]])), "a NaN in the accumulator stays a NaN"
