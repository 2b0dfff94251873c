"""CPU model of the four device calls that carry the per-chunk wire (one 16-byte parameter record, then packed bytes), made of the oracle alone:
dequantize_sum, reduce_quantize_dynamic, quantize_dynamic_batch (dequantize_dynamic_batch is dequantize_sum with one term per member).

Plain numpy over the oracle module `O` (O.dequantize, O.compute_quant_params, O.quantize, O.quantize_per_element, O.f32_to_bf16); nothing of the
product is imported.  float32 tensors are numpy float32, bfloat16 tensors numpy uint16 bit patterns, quantized tensors packed uint8.

A term's record is the 16 bytes the device reads: `<ffq` = scale, 1 / scale, zero point.  A rounding mode is one of
    NEAREST                       round to nearest
    per_call(tau)                 stochastic with one threshold for the call
    per_element(seed, base)       stochastic with the threshold of the 64-bit index base + i for element i of the tensor
"""
import struct

import numpy as np

F32, BF16, UINT2, UINT4, UINT8 = 0, 1, 2, 3, 4
SET, ADD = 0, 1
QMAX = {UINT8: 255, UINT4: 15, UINT2: 3}
BITS = {UINT8: 8, UINT4: 4, UINT2: 2}
NP_OF = {F32: np.float32, BF16: np.uint16}
M64 = (1 << 64) - 1

NEAREST = ("nearest",)


def per_call(tau):
    return ("call", float(tau))


def per_element(seed, index_base):
    return ("element", int(seed), int(index_base))


def record(scale, zero_point, inv=None):
    """the 16 bytes of a parameter record; `inv` defaults to the float32 quotient 1 / scale"""
    s = np.float32(scale)
    if inv is None:
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            inv = np.float32(1.0) / s
    return struct.pack("<ffq", float(s), float(np.float32(inv)), int(zero_point))


def read_record(rec):
    """-> (scale, 1 / scale, zero point) of a 16-byte record"""
    return struct.unpack("<ffq", bytes(rec))


def scale_bits(scale):
    """the float32 bit pattern scales are compared by"""
    return int(np.float32(scale).view(np.uint32))


def same_record(a, b):
    """(scale, zero point) pairs equal, the scale by its float32 bit pattern"""
    return scale_bits(a[0]) == scale_bits(b[0]) and int(a[1]) == int(b[1])


def is_nan(y, dt_f):
    return np.isnan(y) if dt_f == F32 else (y & 0x7FFF) > 0x7F80


def pack(codes, dt_q):
    """one code per element -> packed bytes (low bits = lower element index, the bits behind the end zero)"""
    per, bits = 8 // BITS[dt_q], BITS[dt_q]
    c = np.zeros((codes.size + per - 1) // per * per, dtype=np.uint8)
    c[: codes.size] = codes
    out = np.zeros(c.size // per, dtype=np.uint8)
    for j in range(per):
        out |= c[j::per] << np.uint8(j * bits)
    return out


def dequantize_sum(O, terms, records, dt_q, dt_f, n, op, prev):
    """out (op)= sum of the dequantized terms: O.dequantize per term in order, the first with `op`, the others ADD, the running value held in dt_f.
    `prev` (the previous contents of out; None: zeros) is not modified."""
    out = np.zeros(n, dtype=NP_OF[dt_f]) if prev is None else np.array(prev, dtype=NP_OF[dt_f]).reshape(-1).copy()
    assert out.size == n and len(terms) == len(records)
    for i, (q, rec) in enumerate(zip(terms, records)):
        scale, _, zp = read_record(rec)
        out = O.dequantize(q, dt_q, dt_f, n, scale, zp, op if i == 0 else ADD, out=out)
    return out


def sum_params(O, y, dt_f, dt_q):
    """(scale, zero point) from the non-NaN elements of y; the degenerate record (1.0, qmax >> 1) when there is none"""
    keep = y[~is_nan(y, dt_f)]
    if keep.size == 0:
        return 1.0, QMAX[dt_q] >> 1
    return O.compute_quant_params(np.ascontiguousarray(keep), dt_f, dt_q)


def quantize(O, y, dt_f, dt_q, scale, zp, round):
    if round[0] == "nearest":
        return O.quantize(y, dt_f, dt_q, scale, zp)
    if round[0] == "call":
        return O.quantize(y, dt_f, dt_q, scale, zp, O.STOCHASTIC, round[1])
    assert round[0] == "element"
    return O.quantize_per_element(y, dt_f, dt_q, scale, zp, round[1], round[2] & M64)


def quantize_dynamic(O, x, dt_f, dt_q, round):
    """-> (packed bytes, (scale, zero point)) of one tensor with parameters from its own non-NaN elements"""
    scale, zp = sum_params(O, x, dt_f, dt_q)
    return quantize(O, x, dt_f, dt_q, scale, zp, round), (scale, zp)


def reduce_quantize(O, acc, terms, records, dt_q, dt_f, round):
    """quantize(acc + sum of the dequantized terms) with parameters from that sum -> (packed bytes, (scale, zero point), the sum)"""
    y = dequantize_sum(O, terms, records, dt_q, dt_f, acc.size, ADD, acc)
    q, params = quantize_dynamic(O, y, dt_f, dt_q, round)
    return q, params, y


def quantize_batch(O, xs, dt_f, dt_q, round):
    """per member the single-tensor result: [(packed bytes, (scale, zero point))]; with per-element rounding every member counts from the same
    index_base"""
    return [quantize_dynamic(O, x, dt_f, dt_q, round) for x in xs]
