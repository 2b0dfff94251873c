"""Inputs and models for the fused grouped reduce + quantize with error feedback of a bfloat16 accumulator with a FLOAT32 residual
(piquant_hip_reduce_quantize_grouped_ef_mixed); numpy and the oracle only.  tests/test_grouped_reduce_ef_f32r_cpu.py proves that the inputs
discriminate, tests/test_gpu_grouped_reduce_ef_f32r.py runs them on the device.

The definition is tests/grouped_ef_f32r_sim.py: reduce_ef_f32r_step -- every term by grouped dequantize ADD into the bfloat16 acc, in order, one
rounding to bfloat16 per term, then the mixed step.  reduce_ef_f32r_model is that composition with the rounding mode passed on;
float32_sum_variant is the WRONG model a fused kernel could fall into: the terms summed in float32 and rounded to bfloat16 once.

tie_case builds terms by hand (packed codes, scales and zero points written directly) whose values are small multiples of 2^-8 -- half an ulp of
a bfloat16 in [1, 2) -- against accumulators on both kinds of neighbours:
  acc = 1.0        + 2^-8 is a tie that rounds to even, DOWN to 1.0; twice in a row it stays 1.0, where a float32 running sum reaches 1.0078125
  acc = 1.0078125  + 2^-8 is a tie that rounds to even, UP to 1.015625
  acc = 1.0, terms 2^-8 then 2^-7 give 1.0078125; 2^-7 then 2^-8 give 1.015625: the order of the terms shows
Every value is exact in both dequantize forms ((q - zp) * scale for uint8, fma(q, scale, -zp * scale) for uint4 and uint2)."""
import numpy as np

import oracle as O
from ef_f32r_model import ef_f32r_step
from ef_model import widen
from grouped_model import PACK, dequantize_grouped

BF16 = O.BF16
BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
ACC_CYCLE = (1.0, 1.0078125, -1.0, -1.0078125, 1.015625, 0.5, 2.0, 1.0, 1.0078125, 0.0, 255.0)   # 11 values: coprime to every group size


def pack_codes(codes, qd):
    """one code per element -> packed bytes, element i in bits [(i % per) * bits, ...) of byte i // per; the last byte zero-filled"""
    per, bits = PACK[qd], BITS[qd]
    c = np.zeros((codes.size + per - 1) // per * per, dtype=np.uint32)
    c[: codes.size] = codes
    return (c.reshape(-1, per) << (np.arange(per, dtype=np.uint32) * bits)[None, :]).sum(axis=1).astype(np.uint8)


def _term(units, zps, G, qd):
    """the term whose element i dequantizes to units[i] * 2^-8 with group g's zero point zps[g]: code = units + zp, scale 2^-8"""
    codes = units + np.repeat(zps.astype(np.int64), G)[: units.size]
    assert codes.min() >= 0 and codes.max() < (1 << BITS[qd])
    return pack_codes(codes.astype(np.uint32), qd), np.full(zps.size, 2.0 ** -8, dtype=np.float32), zps.astype(np.uint8)


def tie_case(qd, G, n):
    """-> (acc as bf16 bits, float32 residual, {"A", "B", "C", "D"}: terms as (packed bytes, scales, zero points)).
    A and B dequantize to exactly 2^-8 everywhere, C to 2^-7, D to a mix of {-1, 0, 1, 2} * 2^-8."""
    ng = (n + G - 1) // G
    i = np.arange(n)
    acc = O.f32_to_bf16(np.array(ACC_CYCLE, dtype=np.float32)[i % len(ACC_CYCLE)])
    r = np.where((i // G) % 2 == 0, 0.0, (i % 5) * 2.0 ** -12).astype(np.float32)
    zp01 = (np.arange(ng) % 2).astype(np.int64)
    one = np.ones(n, dtype=np.int64)
    terms = {"A": _term(one, zp01, G, qd), "B": _term(one, 1 - zp01, G, qd), "C": _term(2 * one, zp01, G, qd),
             "D": _term((i * 7 // 3) % 4 - 1, np.ones(ng, dtype=np.int64), G, qd)}
    return acc, r, terms


TIE_ORDERS = ("AB", "AC", "CA", "ABD", "DBA", "ABCD")


def add_terms(acc, terms, qd, G):
    """acc <- rn_bf16(widen(acc) + d_i) term by term: grouped dequantize ADD through the oracle"""
    acc = acc.copy()
    for q, s, z in terms:
        acc = dequantize_grouped(q, qd, BF16, acc.size, G, s, z, O.ADD, prev=acc)
    return acc


def reduce_ef_f32r_model(acc, r, terms, qd, G, round_mode=O.NEAREST, threshold=0.0):
    """reduce_ef_f32r_step (tests/grouped_ef_f32r_sim.py) with the rounding mode passed on -> (packed bytes, scales, zero points, new residual)"""
    return ef_f32r_step(add_terms(acc, terms, qd, G), r, qd, G, round_mode, threshold)[:4]


def float32_sum_variant(acc, r, terms, qd, G):
    """NOT the definition: the terms added to the widened acc in float32, one rounding to bfloat16 at the end, then the mixed step"""
    a = widen(acc, BF16)
    for q, s, z in terms:
        with np.errstate(invalid="ignore", over="ignore"):
            a = a + widen(dequantize_grouped(q, qd, BF16, acc.size, G, s, z), BF16)
    return ef_f32r_step(O.f32_to_bf16(a), r, qd, G)[:4]


def differs(a, b):
    """two (bytes, scales, zero points, residual) results differ in at least one output byte or residual word"""
    return bool(np.any(a[0] != b[0])) or bool(np.any(a[3].view(np.uint32) != b[3].view(np.uint32)))

