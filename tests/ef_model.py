"""CPU model of error-feedback group-wise quantization (piquant_hip_quantize_grouped_ef), built from the group model (tests/grouped_model.py)
and the oracle's bf16 conversions.

One step, with T the tensor's type (float32 arrays, or bf16 bit patterns as uint16 arrays):
  1. y = x + r rounded to T (bf16: both widened to float32, added in float32, rounded to nearest even)
  2. (q, scales, zero points) = quantize_grouped(y) with computed parameters
  3. d = dequantize_grouped(q, scales, zero points) in T (SET)
  4. r <- y - d rounded to T
"""
import numpy as np

import oracle as O
from grouped_model import dequantize_grouped, group_params_all, quantize_grouped

EPS = {O.F32: 2.0 ** -23, O.BF16: 2.0 ** -8}


def widen(a, dt):
    """the values of `a` (float32 array or bf16 bit patterns) as float32"""
    return O.bf16_to_f32(a) if dt == O.BF16 else np.ascontiguousarray(a, dtype=np.float32)


def narrow(f32, dt):
    """float32 values rounded to the type (bf16: the oracle's round to nearest even)"""
    return O.f32_to_bf16(np.ascontiguousarray(f32, dtype=np.float32)) if dt == O.BF16 else np.ascontiguousarray(f32, dtype=np.float32)


def add_t(a, b, dt):
    with np.errstate(invalid="ignore", over="ignore"):
        return narrow(widen(a, dt) + widen(b, dt), dt)


def sub_t(a, b, dt):
    with np.errstate(invalid="ignore", over="ignore"):
        return narrow(widen(a, dt) - widen(b, dt), dt)


def ef_step(x, r, dt, qd, G, round_mode=O.NEAREST, threshold=0.0, quantize=None):
    """-> (packed bytes, scales, zero points, new residual, y, d); x and r are not modified.  quantize: (y, scales, zero points) -> packed bytes
    that takes the place of step 2's rounding (tests/per_element_model.py: per-element thresholds); the parameters stay the computed ones."""
    y = add_t(x, r, dt)
    s, z = group_params_all(widen(y, dt), G, qd)
    q = quantize_grouped(y, dt, qd, G, round_mode, threshold, params=(s, z))[0] if quantize is None else quantize(y, s, z)
    d = dequantize_grouped(q, qd, dt, y.size, G, s, z)
    return q, s, z, sub_t(y, d, dt), y, d


def conservation_defect(xs, ds, r_last, ys, dt):
    """(max |S|, bound): S = sum_t d_t + r_K - sum_t x_t in float64; bound = K eps_T M with M the largest |y| or |d| seen."""
    S = np.zeros(r_last.size, dtype=np.float64)
    M = 0.0
    for x, d, y in zip(xs, ds, ys):
        S += widen(d, dt).astype(np.float64) - widen(x, dt).astype(np.float64)
        M = max(M, float(np.abs(widen(y, dt)).max(initial=0.0)), float(np.abs(widen(d, dt)).max(initial=0.0)))
    S += widen(r_last, dt).astype(np.float64)
    return float(np.abs(S).max(initial=0.0)), len(xs) * EPS[dt] * M
