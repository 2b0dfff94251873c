"""CPU: the randomized Hadamard rotation of whole groups -- the model of tests/rot_model.py against its own definition, the gain it is there for,
and the surface of the three calls (tests/test_gpu_grouped_rotated.py runs the kernels against the model).

The error bounds, for a group of G = 2^k float32 values with u = 2^-24: a transform is k stages of one addition per element, each with a
relative error of at most u, and one multiplication; norm-wise the computed transform differs from the exact one by at most about
(k + 1) u |x|_2, and an element's share of that on random data is of the order sqrt(k) u rms(x).  The bounds below, (k + 2) 2^-23 max|x| per
element for a transform and for the round trip of two, and (k + 2) 2^-23 |x|_2 for a norm, are between 10 and 100 times that."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle as O
import grouped_model as GM
import rot_model as R

ROOT = Path(__file__).resolve().parent.parent
GROUP_SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
SEEDS = (0x1234_5678_9ABC_DEF0, 7)
SYMBOLS = {"piquant_hip_hadamard_grouped": 8, "piquant_hip_quantize_grouped_rotated": 11, "piquant_hip_dequantize_grouped_rotated": 11}


def bound(G):
    return (R.log2_of(G) + 2) * 2.0 ** -23


def random_groups(G, ngroups, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(ngroups * G) * rng.uniform(0.01, 30.0, ngroups * G)).astype(np.float32)


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_inverse_of_forward_is_the_identity(G):
    x = random_groups(G, 8, G)
    y = R.rotate(x, G, SEEDS[0])
    back = R.rotate(y, G, SEEDS[0], inverse=True)
    err = np.abs(back.astype(np.float64) - x).reshape(-1, G).max(axis=1)
    assert np.all(err <= bound(G) * np.abs(x).reshape(-1, G).max(axis=1)), (G, err.max())
    assert not np.array_equal(y, x)


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_model_is_the_signed_hadamard_matrix(G):
    x = random_groups(G, 4, 100 + G)
    d = R.signs(G, SEEDS[1]).astype(np.float64)
    M = R.hadamard_matrix(G) * d[None, :] * 2.0 ** (-R.log2_of(G) / 2)       # c H diag(d) in float64
    exact = x.reshape(-1, G).astype(np.float64) @ M.T
    y = R.rotate(x, G, SEEDS[1]).reshape(-1, G)
    assert np.all(np.abs(y - exact).max(axis=1) <= bound(G) * np.abs(x).reshape(-1, G).max(axis=1))
    # the inverse is the transpose: diag(d) H c
    z = R.rotate(x, G, SEEDS[1], inverse=True).reshape(-1, G)
    assert np.all(np.abs(z - x.reshape(-1, G).astype(np.float64) @ M).max(axis=1) <= bound(G) * np.abs(x).reshape(-1, G).max(axis=1))


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_group_norms_are_preserved(G):
    x = random_groups(G, 8, 200 + G)
    for inverse in (False, True):
        y = R.rotate(x, G, SEEDS[0], inverse)
        nx = np.linalg.norm(x.reshape(-1, G).astype(np.float64), axis=1)
        ny = np.linalg.norm(y.reshape(-1, G).astype(np.float64), axis=1)
        assert np.all(np.abs(ny - nx) <= bound(G) * nx)


def test_constant_is_the_contracts():
    assert R.SQRT2_F32 == np.float32(np.sqrt(2.0))
    for G in GROUP_SIZES:
        k = R.log2_of(G)
        c = R.scale_const(G)
        assert c.dtype == np.float32
        if k % 2 == 0:
            assert c == np.float32(2.0 ** (-k // 2))
        else:
            assert c == np.float32(np.float32(np.sqrt(2.0)) * 2.0 ** (-(k + 1) // 2))
        assert abs(float(c) - 2.0 ** (-k / 2)) <= 2.0 ** -24 * 2.0 ** (-k / 2)


def test_sign_rule():
    """d[j] from bit j mod 16 of floor(element_threshold(seed, j div 16) * 2^24); two seeds give different signs; the signs of a smaller group size
    are the leading ones of a larger (they depend on the position only)."""
    ds = []
    for seed in SEEDS:
        d = R.signs(4096, seed)
        for j in range(4096):
            word = int(np.floor(np.float64(O.element_threshold(seed, j // 16)) * 2.0 ** 24))
            assert d[j] == (-1.0 if (word >> (j % 16)) & 1 else 1.0), (seed, j)
        assert set(np.unique(d)) == {-1.0, 1.0}
        assert 0.4 < np.mean(d < 0) < 0.6
        for G in GROUP_SIZES:
            assert np.array_equal(R.signs(G, seed), d[:G])
        ds.append(d)
    assert not np.array_equal(ds[0][:32], ds[1][:32])
    assert np.array_equal(R.signs(128, SEEDS[0] + (1 << 64)), R.signs(128, SEEDS[0]))   # modulo 2^64


@pytest.mark.parametrize("G", (32, 128, 4096))
def test_ragged_tail_and_short_tensor_are_unchanged(G):
    x = random_groups(G, 3, 300 + G)[: 2 * G + G // 2 + 1]
    for inverse in (False, True):
        y = R.rotate(x, G, SEEDS[0], inverse)
        assert np.array_equal(y[2 * G:].view(np.uint32), x[2 * G:].view(np.uint32))
        assert not np.array_equal(y[: 2 * G], x[: 2 * G])
        short = x[: G - 1]
        assert np.array_equal(R.rotate(short, G, SEEDS[0], inverse).view(np.uint32), short.view(np.uint32))
    xb = O.f32_to_bf16(x)
    yb = R.hadamard_grouped(xb, O.BF16, G, SEEDS[0])
    assert yb.dtype == np.uint16 and np.array_equal(yb[2 * G:], xb[2 * G:]) and not np.array_equal(yb[: 2 * G], xb[: 2 * G])
    assert R.rotate(np.zeros(0, dtype=np.float32), G, 1).size == 0
    # a shard that starts on a group boundary rotates as the whole tensor does
    assert np.array_equal(R.rotate(x[G:], G, SEEDS[0])[:G].view(np.uint32), R.rotate(x, G, SEEDS[0])[G: 2 * G].view(np.uint32))


def test_non_finite_inputs_propagate():
    G = 64
    x = random_groups(G, 3, 5)
    x[G + 3] = np.nan
    x[2 * G + 9] = np.inf
    y = R.rotate(x, G, SEEDS[0])
    assert np.all(np.isfinite(y[:G])) and np.all(np.isnan(y[G: 2 * G])) and not np.any(np.isfinite(y[2 * G:]))


def round_trip_mse(x, qd, G, seed=None):
    n = x.size
    if seed is None:
        q, s, z = GM.quantize_grouped(x, O.F32, qd, G)
        back = GM.dequantize_grouped(q, qd, O.F32, n, G, s, z)
    else:
        q, s, z = R.quantize_grouped_rotated(x, O.F32, qd, G, seed)
        back = R.dequantize_grouped_rotated(q, qd, O.F32, n, G, s, z, seed)
    return float(np.mean((back.astype(np.float64) - x) ** 2))


def test_rotation_gains_on_outliers():
    """The one fixed ratio: G = 128, uint4, N(0, 1) with one 50 sigma element per group, 4 096 groups, the oracle's exact formulas: the rotated
    round trip's MSE is at most 0.25 of the un-rotated one's (a float64 simulation with plain min/max quantization gave 0.064)."""
    x = R.outlier_data(128, 4096, 11)
    plain, rotated = round_trip_mse(x, O.UINT4, 128), round_trip_mse(x, O.UINT4, 128, SEEDS[0])
    print(f"G=128 uint4 outliers: MSE rotated / plain = {rotated:.6g} / {plain:.6g} = {rotated / plain:.4f}")
    assert rotated <= 0.25 * plain, (rotated, plain)


def test_model_round_trip_of_the_three_calls_is_consistent():
    """quantize_grouped_rotated is quantize_grouped of the rotated tensor, for a bfloat16 tensor without rounding it back; dequantize ADD adds once."""
    G, n = 64, 64 * 5 + 17
    xb = O.f32_to_bf16(random_groups(G, 6, 9)[:n])
    y = R.rotate(O.bf16_to_f32(xb), G, 3)
    q, s, z = R.quantize_grouped_rotated(xb, O.BF16, O.UINT4, G, 3)
    q2, s2, z2 = GM.quantize_grouped(y, O.F32, O.UINT4, G)
    assert np.array_equal(q, q2) and np.array_equal(s, s2) and np.array_equal(z, z2)
    assert not np.array_equal(q, GM.quantize_grouped(O.bf16_to_f32(O.f32_to_bf16(y)), O.F32, O.UINT4, G)[0])
    prev = O.f32_to_bf16(random_groups(G, 6, 10)[:n])
    got = R.dequantize_grouped_rotated(q, O.UINT4, O.BF16, n, G, s, z, 3, O.ADD, prev)
    zf = R.dequantize_grouped_rotated(q, O.UINT4, O.F32, n, G, s, z, 3)
    assert np.array_equal(got, O.f32_to_bf16(O.bf16_to_f32(prev) + zf))
    qe, _, _ = R.quantize_grouped_rotated_per_element(xb, O.BF16, O.UINT4, G, 3, 99, 1 << 33)
    assert qe.shape == q.shape and not np.array_equal(qe, q)


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    import piquant
    import piquant.torch as pt
    from piquant._bootstrap import C_LIB, library_path

    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for symbol, nargs in SYMBOLS.items():
        assert re.search(r"PIQUANT_EXPORT\s+void\s+" + symbol + r"\s*\(", header), f"{symbol} is not declared in piquant_hip.h"
        assert len(getattr(C_LIB, symbol).argtypes) == nargs
        assert symbol in exported, f"libpiquant.so does not export {symbol}"
    for name in ("hadamard_grouped", "quantize_grouped_rotated", "dequantize_grouped_rotated"):
        assert callable(getattr(pt, name)) and callable(getattr(piquant.Context, name + "_ptr"))


def test_torch_wrappers_refuse_bad_arguments():
    """Host tensors throughout: nothing here touches a device."""
    import piquant.torch as pt

    x = torch.zeros(1000)
    q = torch.zeros(1000, dtype=torch.uint8)
    s, z = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    for bad in (100, 16, 8192, None, 128.0, True):
        with pytest.raises(ValueError, match="group_size"):
            pt.hadamard_grouped(x, group_size=bad, seed=1)
        with pytest.raises(ValueError, match="group_size"):
            pt.quantize_grouped_rotated(x, dtype=torch.quint4x2, group_size=bad, seed=1)
        with pytest.raises(ValueError, match="group_size"):
            pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=bad, seed=1)
    with pytest.raises(ValueError, match="seed"):
        pt.hadamard_grouped(x)
    with pytest.raises(ValueError, match="seed"):
        pt.quantize_grouped_rotated(x, dtype=torch.quint4x2)
    with pytest.raises(ValueError, match="seed"):
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=128)
    for bad in (1.5, "7", None, True):
        with pytest.raises(ValueError, match="seed"):
            pt.hadamard_grouped(x, seed=bad)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pt.hadamard_grouped(q, seed=1)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pt.hadamard_grouped(torch.zeros(64, dtype=torch.float16), seed=1)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pt.quantize_grouped_rotated(q, dtype=torch.quint4x2, seed=1)
    with pytest.raises(ValueError, match="quantized dtype"):
        pt.quantize_grouped_rotated(x, dtype=torch.float32, seed=1)
    with pytest.raises(ValueError, match="round_mode"):
        pt.quantize_grouped_rotated(x, dtype=torch.quint4x2, seed=1, round_mode="up")
    with pytest.raises(ValueError, match="both out_scales and out_zero_points"):
        pt.quantize_grouped_rotated(x, dtype=torch.quint4x2, seed=1, out_scales=s)
    with pytest.raises(ValueError, match="float dtype"):
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.uint8, group_size=128, seed=1)
    with pytest.raises(ValueError, match="reduce_op"):
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=128, seed=1, reduce_op="mul")
    with pytest.raises(ValueError, match="quantized tensor"):
        pt.dequantize_grouped_rotated(x, s, z, dtype=torch.float32, group_size=128, seed=1)
    with pytest.raises(ValueError, match="scales must be"):
        pt.dequantize_grouped_rotated(q, s[:3], z, dtype=torch.float32, group_size=128, seed=1)
    with pytest.raises(ValueError, match="ROCm"):
        pt.hadamard_grouped(x, seed=1)                       # everything matches, but host tensors
    with pytest.raises(ValueError, match="ROCm"):
        pt.quantize_grouped_rotated(x, dtype=torch.quint4x2, seed=1)
    with pytest.raises(ValueError, match="ROCm"):
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=128, seed=1)
