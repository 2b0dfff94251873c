"""CPU model of error feedback in the rotated domain (include/piquant_hip.h, piquant_hip_quantize_grouped_rotated_ef /
_reduce_quantize_grouped_rotated_ef): compositions of tests/rot_model.py, tests/grouped_rotated_sim.py's rotated_sum, tests/ef_model.py and
tests/per_element_model.py, with no arithmetic of their own.

The residual is a float32 array of ROTATED values whatever the tensor's type:
  quantize   ef_step(rotate(widen(x)), r) in float32
  reduce     ef_step(rotate(widen(acc)) + the terms' float32 dequantizes in order, r) in float32: the residual is added behind the terms
Every function returns ef_model.ef_step's tuple (packed bytes, scales, zero points, new residual, y, d)."""
import oracle as O
import ef_model as EF
import per_element_model as PE
import rot_model as RM


def rotated_sum(acc, dt, terms, qd, G, seed):
    import grouped_rotated_sim as S

    return S.rotated_sum(acc, dt, terms, qd, G, seed)


def quantize_grouped_rotated_ef(x, dt, r, qd, G, seed, round_mode=O.NEAREST, threshold=0.0):
    return EF.ef_step(RM.rotate(RM.widen(x, dt), G, seed), r, O.F32, qd, G, round_mode, threshold)


def reduce_quantize_grouped_rotated_ef(acc, dt, r, terms, qd, G, seed, round_mode=O.NEAREST, threshold=0.0):
    return EF.ef_step(rotated_sum(acc, dt, terms, qd, G, seed), r, O.F32, qd, G, round_mode, threshold)


def reduce_quantize_grouped_rotated_ef_per_element(acc, dt, r, terms, qd, G, seed, elem_seed, index_base):
    """the same in per-element stochastic mode: element i draws the threshold of index index_base + i (no terms: the quantize)"""
    rounding = lambda y, s, z: PE.quantize(y, O.F32, qd, G, elem_seed, index_base, (s, z))[0]   # noqa: E731
    return EF.ef_step(rotated_sum(acc, dt, terms, qd, G, seed), r, O.F32, qd, G, quantize=rounding)
