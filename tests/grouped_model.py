"""CPU model of group-wise quantization (piquant_hip_quantize_grouped / _dequantize_grouped), built from the oracle's per-tensor steps.

Group g covers [g G, min((g + 1) G, n)).  Its parameters are the device scan's: min / max with NaNs ignored (np.fmin / np.fmax from the
scan's identities +-FLT_MAX), a group of nothing but NaNs -- max < min -- gets the degenerate (1.0, qmax >> 1), otherwise the reference
epilogue (oracle.quant_params_from_minmax).  Its bytes are oracle.quantize of the slice (the position-independent form), laid end to end.
"""
import numpy as np

import oracle as O

FLT_MAX = np.float32(3.4028234663852886e38)
QMAX = {O.UINT2: 3, O.UINT4: 15, O.UINT8: 255}
PACK = {O.UINT2: 4, O.UINT4: 2, O.UINT8: 1}


def as_f32(x, dt_in):
    return O.bf16_to_f32(x) if dt_in == O.BF16 else np.ascontiguousarray(x, dtype=np.float32)


def group_params(xf32: np.ndarray, qd: int):
    """(scale, zero point) of one group given as float32 values."""
    lo = np.fmin.reduce(xf32, initial=FLT_MAX) if xf32.size else FLT_MAX
    hi = np.fmax.reduce(xf32, initial=-FLT_MAX) if xf32.size else -FLT_MAX
    if not hi > lo:
        return 1.0, QMAX[qd] >> 1
    return O.quant_params_from_minmax(float(lo), float(hi), qd)


def groups(n: int, G: int):
    return [(b, min(b + G, n)) for b in range(0, n, G)]


def quantize_grouped(x, dt_in, qd, G, round_mode=O.NEAREST, threshold=0.0, params=None):
    """-> (packed bytes, scales float32[ng], zero points uint8[ng]); `params` = (scales, zero_points) given instead of computed."""
    xf = as_f32(x, dt_in)
    gs = groups(x.size, G)
    scales = np.empty(len(gs), dtype=np.float32)
    zps = np.empty(len(gs), dtype=np.uint8)
    parts = []
    for g, (b, e) in enumerate(gs):
        if params is None:
            s, z = group_params(xf[b:e], qd)
        else:
            s, z = float(params[0][g]), int(params[1][g])
        scales[g], zps[g] = s, z
        parts.append(O.quantize(x[b:e], dt_in, qd, s, z, round_mode, threshold))
    q = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return q, scales, zps


def dequantize_grouped(q, qd, dt_out, n, G, scales, zps, reduce_op=O.SET, prev=None):
    """Group by group through oracle.dequantize; `prev` is the accumulator for ADD (copied, not modified)."""
    out = np.zeros(n, dtype=np.float32 if dt_out == O.F32 else np.uint16) if prev is None else prev.copy()
    for g, (b, e) in enumerate(groups(n, G)):
        qb, qe = b // PACK[qd], (e + PACK[qd] - 1) // PACK[qd]
        seg = out[b:e].copy()
        O.dequantize(q[qb:qe], qd, dt_out, e - b, float(scales[g]), int(zps[g]), reduce_op, out=seg)
        out[b:e] = seg
    return out


def group_minmax(xf32: np.ndarray, G: int):
    """Vectorised per-group {min, max} with NaNs ignored, from the scan's identities."""
    ng = (xf32.size + G - 1) // G
    pad = np.full(ng * G, np.nan, dtype=np.float32)
    pad[: xf32.size] = xf32
    m = pad.reshape(ng, G)
    return np.fmin.reduce(m, axis=1, initial=FLT_MAX), np.fmax.reduce(m, axis=1, initial=-FLT_MAX)


def group_params_all(xf32: np.ndarray, G: int, qd: int):
    """Every group's (scale, zero point) as float32[ng], uint8[ng] (same rules as group_params)."""
    lo, hi = group_minmax(xf32, G)
    s = np.empty(lo.size, dtype=np.float32)
    z = np.empty(lo.size, dtype=np.uint8)
    for g in range(lo.size):
        s[g], z[g] = (1.0, QMAX[qd] >> 1) if not hi[g] > lo[g] else O.quant_params_from_minmax(float(lo[g]), float(hi[g]), qd)
    return s, z
