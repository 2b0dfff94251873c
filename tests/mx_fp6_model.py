"""The MXFP6 formats of include/piquant_hip.h (E2M3 and E3M2 under piquant_hip_quantize_mx / piquant_hip_dequantize_mx) in numpy: float64 and
integers, no lanes.  Codes travel unpacked (one uint8 per element); pack / unpack give the stored bytes, the dense 6-bit string."""
import numpy as np

from mx_model import bf16_bits, bf16_to_f32, store  # noqa: F401  (the float side is the FP4 / FP8 model's)

BLOCK = 32
E2M3, E3M2 = "fp6_e2m3", "fp6_e3m2"
FORMATS = (E2M3, E3M2)
EMAX = {E2M3: 2, E3M2: 4}
MBITS = {E2M3: 3, E3M2: 2}
BIAS = {E2M3: 1, E3M2: 3}
TOP, SIGN = 0x1F, 0x20               # the largest positive code; neither format has a NaN or an infinity


def code_values(fmt):
    """float64 value of each of the 64 codes."""
    c = np.arange(64)
    mb, one = MBITS[fmt], 1 << MBITS[fmt]
    e, m = (c & 0x1F) >> mb, c & (one - 1)
    v = np.where(e == 0, m * 2.0 ** (1 - BIAS[fmt] - mb), (one + m) * 2.0 ** (e - BIAS[fmt] - mb))
    return np.where(c & SIGN, -v, v)


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
    mags = code_values(fmt)[: TOP + 1]
    mid = (mags[:-1] + mags[1:]) / 2
    k = np.searchsorted(mid, av, side="left")                         # midpoints below |v|; everything above the last one saturates
    tie = mid[np.minimum(k, mid.size - 1)] == av
    code = (k + (tie & (k % 2 == 1))).astype(np.uint8) | np.where(np.signbit(xf), SIGN, 0).astype(np.uint8)
    code[np.isnan(xf)] = 0
    return code[:n], s.astype(np.uint8)


def dequantize(codes, scales, fmt):
    """float32[numel]: value(code) * 2^(s - 127) rounded to float32 (+-inf past the top); NaN for s = 0xFF."""
    s = np.repeat(scales.astype(np.int64), BLOCK)[: codes.size]
    with np.errstate(over="ignore"):
        d = np.ldexp(code_values(fmt)[codes], s - 127).astype(np.float32)
    d[s == 255] = np.nan
    return d


def pack(codes):
    """Element i in bits [6i, 6i + 6) of the little-endian bit string: ceil(6 * numel / 8) bytes, the spare bits of the last one 0."""
    bits = (codes[:, None] >> np.arange(6)) & 1
    return np.packbits(bits.ravel().astype(np.uint8), bitorder="little")


def unpack(raw, numel):
    bits = np.unpackbits(raw, bitorder="little")[: 6 * numel].reshape(numel, 6)
    return (bits << np.arange(6)).sum(1).astype(np.uint8)
