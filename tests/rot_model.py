"""CPU model of the randomized Hadamard rotation of whole groups and of the three calls built on it (include/piquant_hip.h,
piquant_hip_hadamard_grouped / _quantize_grouped_rotated / _dequantize_grouped_rotated), made only from numpy float32 butterflies,
oracle.element_threshold, the oracle's bfloat16 conversions and the group model (tests/grouped_model.py, tests/per_element_model.py).

The rotation of group size G = 2^k with a 64-bit seed, on float32 values, one FULL group at a time:
  signs        d[j] = -1 if bit (j mod 16) of floor(element_threshold(seed, j div 16) * 2^24) is set, else +1: the same d for every group
  butterflies  fwht(v): for h = 1, 2, 4, .., G / 2 in this order, every pair (i, i + h) with bit h of i clear becomes (v[i] + v[i + h],
               v[i] - v[i + h]), each ONE float32 operation
  constant     c_G = 2^(-k / 2): the exact power of two for even k, float32(sqrt 2) (bits 0x3FB504F3) * 2^(-(k + 1) / 2) for odd k
  forward      y = c_G * fwht(d * x)            inverse      x = d * (c_G * fwht(y))
A ragged last group (a tensor shorter than G is one) is not rotated.
"""
import numpy as np

import oracle as O
import grouped_model as GM
import per_element_model as PE

SQRT2_F32 = np.array([0x3FB504F3], dtype=np.uint32).view(np.float32)[0]


def log2_of(G: int) -> int:
    assert G >= 32 and G <= 4096 and G & (G - 1) == 0
    return G.bit_length() - 1


def scale_const(G: int) -> np.float32:
    k = log2_of(G)
    return np.float32((SQRT2_F32 if k & 1 else np.float32(1.0)) * np.float32(2.0 ** -((k + 1) // 2)))   # a power-of-two factor: exact


def sign_words(G: int, seed: int):
    """the 16-bit sign words of a group: word w covers positions [16 w, 16 w + 16)"""
    return [int(O.element_threshold(seed & PE.M64, w) * 16777216.0) & 0xFFFF for w in range(G // 16)]


def signs(G: int, seed: int) -> np.ndarray:
    d = np.ones(G, dtype=np.float32)
    for w, word in enumerate(sign_words(G, seed)):
        for b in range(16):
            if (word >> b) & 1:
                d[16 * w + b] = -1.0
    return d


def fwht(v: np.ndarray) -> np.ndarray:
    """float32 [ng, G] -> the butterflies of every row, stage by stage in the contract's order"""
    assert v.dtype == np.float32 and v.ndim == 2
    ng, G = v.shape
    with np.errstate(over="ignore", invalid="ignore"):
        h = 1
        while h < G:
            p = v.reshape(ng, G // (2 * h), 2, h)
            a, b = p[:, :, 0, :], p[:, :, 1, :]
            v = np.stack([a + b, a - b], axis=2).reshape(ng, G)   # float32 + float32: one correctly rounded float32 operation each
            h *= 2
    return v


def rotate(x: np.ndarray, G: int, seed: int, inverse: bool = False) -> np.ndarray:
    """float32[n] -> float32[n]: every full group rotated (forward or inverse), the ragged last group unchanged"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    full = x.size // G
    out = x.copy()
    if full == 0:
        return out
    d, c = signs(G, seed), scale_const(G)
    v = x[: full * G].reshape(full, G)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (fwht(v) * c) * d[None, :] if inverse else fwht(v * d[None, :]) * c
    out[: full * G] = y.reshape(-1)
    return out


def widen(x: np.ndarray, dt: int) -> np.ndarray:
    return GM.as_f32(x, dt)


def hadamard_grouped(x: np.ndarray, dt: int, G: int, seed: int, inverse: bool = False) -> np.ndarray:
    """out of the tensor's type: float32 as is; bfloat16 widened, transformed, rounded on store -- a group that is not rotated keeps its bits"""
    y = rotate(widen(x, dt), G, seed, inverse)
    if dt == O.F32:
        return y
    out = x.copy()
    full = x.size // G * G
    out[:full] = O.f32_to_bf16(y[:full])
    return out


def quantize_grouped_rotated(x, dt, qd, G, seed, round_mode=O.NEAREST, threshold=0.0):
    """-> (packed bytes, scales, zero points): quantize_grouped of the float32 forward rotation of the widened tensor"""
    return GM.quantize_grouped(rotate(widen(x, dt), G, seed), O.F32, qd, G, round_mode, threshold)


def quantize_grouped_rotated_per_element(x, dt, qd, G, seed, elem_seed, index_base, start=0):
    """the same in per-element stochastic mode: element i draws the threshold of index index_base + i; x may be the window [start, start + x.size) of
    a longer tensor, start a multiple of G (the rotation depends on the position inside the group only)"""
    return PE.quantize(rotate(widen(x, dt), G, seed), O.F32, qd, G, elem_seed, index_base, start=start)


def dequantize_grouped_rotated(q, qd, dt_out, n, G, scales, zps, seed, reduce_op=O.SET, prev=None):
    """z = the float32 inverse rotation of the float32 grouped dequantize; SET converts z, ADD converts widen(prev) + z (one float32 add)"""
    z = rotate(GM.dequantize_grouped(q, qd, O.F32, n, G, scales, zps), G, seed, inverse=True)
    if reduce_op == O.ADD:
        with np.errstate(over="ignore", invalid="ignore"):
            z = widen(prev, dt_out) + z
    return z if dt_out == O.F32 else O.f32_to_bf16(z)


def hadamard_matrix(G: int) -> np.ndarray:
    """the Sylvester matrix H_G in float64: fwht(v) == H v exactly in exact arithmetic"""
    H = np.ones((1, 1))
    while H.shape[0] < G:
        H = np.block([[H, H], [H, -H]])
    return H


def outlier_data(G: int, ngroups: int, seed: int) -> np.ndarray:
    """N(0, 1) with one element of 50 sigma in every group: the data of the one fixed quality ratio"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(ngroups * G).astype(np.float32)
    x[np.arange(ngroups) * G + rng.integers(0, G, ngroups)] = 50.0 * rng.choice([-1.0, 1.0], ngroups)
    return x
