"""Stochastic rounding for the MX formats (include/piquant_hip.h, piquant_hip_quantize_mx_sr) in numpy: float64 and integers, no lanes.  The code
tables and the packing are mx_model's and mx_fp6_model's, the thresholds oracle.element_threshold's.  Codes travel unpacked, one uint8 per element."""
import numpy as np

import mx_fp6_model as M6
import mx_model as M4
import oracle

BLOCK = 32
FP4, FP8, E2M3, E3M2 = M4.FP4, M4.FP8, M6.E2M3, M6.E3M2
FORMATS = (FP4, FP8, E2M3, E3M2)
EMAX = {**M4.EMAX, **M6.EMAX}
TOP_MANT = {FP4: 0x400000, E2M3: 0x700000, E3M2: 0x600000, FP8: 0x600000}     # the mantissa field of 6, 7.5, 28, 448
SIGN = {**M4.SIGN, E2M3: M6.SIGN, E3M2: M6.SIGN}
NAN_CODE = {FP4: 0, FP8: 0x7F, E2M3: 0, E3M2: 0}


def magnitudes(fmt):
    """The non-negative finite values of the format in code order (code k has value magnitudes[k]), float64."""
    return M4.code_values(fmt)[: M4.TOP[fmt] + 1] if fmt in M4.EMAX else M6.code_values(fmt)[: M6.TOP + 1]


def thresholds(seed, index_base, n):
    """t = floor(element_threshold(seed, g) * 2^24) for g = index_base .. index_base + n - 1 (modulo 2^64)."""
    return np.array([int(oracle.element_threshold(seed, (index_base + i) & (2 ** 64 - 1)) * 2 ** 24) for i in range(n)], np.int64)


def scale_bytes(x, fmt):
    """The scale byte with headroom of every block of a float32 array."""
    nb = -(-x.size // BLOCK)
    a = np.zeros(nb * BLOCK, np.uint32)
    a[: x.size] = x.view(np.uint32) & 0x7FFFFFFF
    a[a > 0x7F800000] = 0                                             # NaNs do not take part
    amax = a.reshape(nb, BLOCK).max(1).astype(np.int64)
    E, M = amax >> 23, amax & 0x7FFFFF
    bump = (E >= EMAX[fmt]) & (E < 255) & (M > TOP_MANT[fmt])
    return (np.maximum(E - EMAX[fmt], 0) + bump).astype(np.uint8)


def quantize(x, fmt, seed, index_base=0):
    """(codes uint8[numel], scales uint8[nblocks]) of a float32 array (a bfloat16 tensor: widened exactly first)."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    s = scale_bytes(x, fmt)
    with np.errstate(invalid="ignore"):
        xf = x.astype(np.float64)
    v = np.abs(np.ldexp(xf, 127 - np.repeat(s.astype(np.int64), BLOCK)[: x.size]))   # exact: a power-of-two scaling in float64
    mags = magnitudes(fmt)
    top = mags.size - 1
    finite = np.isfinite(v)
    vv = np.where(finite, v, 0.0)
    assert (vv <= mags[top]).all(), "the headroom rule keeps every finite element at or below the top"
    k = np.searchsorted(mags, vv, side="right") - 1                 # lo = mags[k] <= v
    lo, hi = mags[k], mags[np.minimum(k + 1, top)]
    fl = np.where(k < top, np.floor((vv - lo) / np.where(k < top, hi - lo, 1.0) * 2.0 ** 24), 0).astype(np.int64)   # exact in float64
    code = k + (fl + thresholds(seed, index_base, x.size) >= 2 ** 24)
    code = np.where(np.isinf(xf), top, code) | np.where(np.signbit(xf), SIGN[fmt], 0)
    return np.where(np.isnan(xf), NAN_CODE[fmt], code).astype(np.uint8), s


def pack(codes, fmt):
    return M4.pack(codes, fmt) if fmt in M4.EMAX else M6.pack(codes)


def dequantize(codes, scales, fmt):
    return (M4 if fmt in M4.EMAX else M6).dequantize(codes, scales, fmt)
