"""The MX block formats of include/piquant_hip.h (piquant_hip_quantize_mx / piquant_hip_dequantize_mx) in numpy: float64 and integers, no lanes.
Codes travel unpacked (one uint8 per element); pack / unpack give the stored bytes."""
import numpy as np

BLOCK = 32
FP4, FP8 = "fp4_e2m1", "fp8_e4m3"
EMAX = {FP4: 2, FP8: 8}
TOP = {FP4: 7, FP8: 0x7E}          # the largest finite positive code
SIGN = {FP4: 0x8, FP8: 0x80}


def code_values(fmt):
    """float64 value of every code (16 or 256); the E4M3 NaN codes are NaN."""
    if fmt == FP4:
        mag = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6.0])
        return np.concatenate([mag, -mag])
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    v[(c & 0x7F) == 0x7F] = np.nan
    return np.where(c & 0x80, -v, v)


def quantize(x, fmt):
    """(codes uint8[numel], scales uint8[nblocks]) of a float32 array (a bfloat16 tensor: widened exactly first)."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    n, nb = x.size, -(-x.size // BLOCK)
    bits = np.zeros(nb * BLOCK, np.uint32)
    bits[:n] = x.view(np.uint32)
    a = bits & 0x7FFFFFFF
    a[a > 0x7F800000] = 0                                             # NaNs do not take part
    E = np.maximum(a.reshape(nb, BLOCK).max(1) >> 23, 1).astype(np.int64)
    s = np.maximum(E - EMAX[fmt], 0)
    with np.errstate(invalid="ignore"):                             # a signaling NaN among the inputs
        xf = bits.view(np.float32).astype(np.float64)
    av = np.abs(np.ldexp(xf, np.repeat(127 - s, BLOCK)))             # exact: a power-of-two scaling in float64
    mags = code_values(fmt)[: TOP[fmt] + 1]
    mid = (mags[:-1] + mags[1:]) / 2
    k = np.searchsorted(mid, av, side="left")                         # midpoints below |v|; everything above the last one saturates
    tie = mid[np.minimum(k, mid.size - 1)] == av
    code = (k + (tie & (k % 2 == 1))).astype(np.uint8) | np.where(np.signbit(xf), SIGN[fmt], 0).astype(np.uint8)
    code[np.isnan(xf)] = 0 if fmt == FP4 else 0x7F
    return code[:n], s.astype(np.uint8)


def dequantize(codes, scales, fmt):
    """float32[numel]: value(code) * 2^(s - 127) rounded to float32; NaN for s = 0xFF and NaN codes."""
    s = np.repeat(scales.astype(np.int64), BLOCK)[: codes.size]
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.ldexp(code_values(fmt)[codes], s - 127).astype(np.float32)
    d[s == 255] = np.nan
    return d


def bf16_bits(f):
    """RNE_bf16 of a float32 array, as uint16 (NaN: the quiet NaN)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(f)] = 0x7FC0
    return r


def bf16_to_f32(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def store(d, out_before=None, bf16=False):
    """What dequantize leaves in `out`: SET (out_before None) or ADD; float32, or bfloat16 bits (out_before then too) rounded once."""
    with np.errstate(over="ignore", invalid="ignore"):
        if out_before is not None:
            d = (bf16_to_f32(out_before) if bf16 else np.asarray(out_before, np.float32)) + d
    return bf16_bits(d) if bf16 else d


def pack(codes, fmt):
    if fmt == FP8:
        return codes.copy()
    c = np.concatenate([codes, np.zeros(codes.size % 2, np.uint8)])
    return c[0::2] | (c[1::2] << 4)


def unpack(raw, numel, fmt):
    if fmt == FP8:
        return raw[:numel].copy()
    return np.stack([raw & 0xF, raw >> 4], 1).ravel()[:numel]
