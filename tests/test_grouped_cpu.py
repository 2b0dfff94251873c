"""Group-wise quantization without a GPU: the CPU group model the GPU tests check against, and the Python argument checks of
piquant.torch.quantize_grouped / dequantize_grouped, which raise ValueError before any device work."""
import numpy as np
import pytest

import oracle as O
from grouped_model import FLT_MAX, dequantize_grouped, group_params, groups, quantize_grouped


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


@pytest.mark.parametrize("qd", [O.UINT8, O.UINT4, O.UINT2])
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_group_params_match_oracle_on_slices(qd, G):
    rng = np.random.default_rng(G + qd)
    x = (rng.standard_normal(10 * G + 7) * rng.uniform(0.1, 10)).astype(np.float32)
    for b, e in groups(x.size, G):
        assert group_params(x[b:e], qd) == O.compute_quant_params(x[b:e], O.F32, qd)


def test_group_params_nan_rules():
    x = np.array([np.nan, 1.0, -2.0, np.nan], dtype=np.float32)
    assert group_params(x, O.UINT4) == O.compute_quant_params(np.array([1.0, -2.0], dtype=np.float32), O.F32, O.UINT4)
    assert group_params(np.full(32, np.nan, dtype=np.float32), O.UINT4) == (1.0, 7)
    assert group_params(np.full(32, np.nan, dtype=np.float32), O.UINT8) == (1.0, 127)
    assert group_params(np.full(32, 3.0, dtype=np.float32), O.UINT2) == (1.0, 1)
    assert group_params(np.array([FLT_MAX], dtype=np.float32), O.UINT8) == (1.0, 127)


@pytest.mark.parametrize("dt_in", [O.F32, O.BF16])
@pytest.mark.parametrize("qd", [O.UINT8, O.UINT4, O.UINT2])
def test_grouped_model_is_per_group_quantize(dt_in, qd):
    G = 32
    rng = np.random.default_rng(qd)
    xf = rng.uniform(-3, 3, 5 * G + 3).astype(np.float32)
    x = O.f32_to_bf16(xf) if dt_in == O.BF16 else xf
    q, s, z = quantize_grouped(x, dt_in, qd, G)
    pack = {O.UINT8: 1, O.UINT4: 2, O.UINT2: 4}[qd]
    assert q.size == O.packed_numel(x.size, qd) and s.size == z.size == 6
    for g, (b, e) in enumerate(groups(x.size, G)):
        assert np.array_equal(q[b // pack:(e + pack - 1) // pack], O.quantize(x[b:e], dt_in, qd, float(s[g]), int(z[g])))
    # given parameters reproduce the computed bytes; dequantize is per group too
    q2, _, _ = quantize_grouped(x, dt_in, qd, G, params=(s, z))
    assert np.array_equal(q, q2)
    for dt_out in (O.F32, O.BF16):
        d = dequantize_grouped(q, qd, dt_out, x.size, G, s, z)
        b, e = 2 * G, 3 * G
        assert np.array_equal(d[b:e], O.dequantize(q[b // pack:e // pack], qd, dt_out, G, float(s[2]), int(z[2])))


def test_grouped_beats_per_tensor_on_outliers():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(128 * 64).astype(np.float32)
    x[rng.choice(x.size, 8, replace=False)] = 200.0
    q, s, z = quantize_grouped(x, O.F32, O.UINT4, 128)
    err_g = np.abs(dequantize_grouped(q, O.UINT4, O.F32, x.size, 128, s, z) - x).mean()
    st, zt = O.compute_quant_params(x, O.F32, O.UINT4)
    err_t = np.abs(O.dequantize(O.quantize(x, O.F32, O.UINT4, st, zt), O.UINT4, O.F32, x.size, st, zt) - x).mean()
    assert err_g * 4 < err_t


# ---- argument checks: ValueError before anything reaches the device -----------------------------------------------------------------
torch = pytest.importorskip("torch")


def _pt():
    import piquant.torch as pt

    return pt


def test_quantize_grouped_rejects_cpu_tensor():
    with pytest.raises(ValueError):
        _pt().quantize_grouped(torch.zeros(256), dtype=torch.quint4x2)


@pytest.mark.parametrize("G", [0, 16, 31, 48, 100, 8192, 128.0, True, None])
def test_bad_group_size(G):
    pt = _pt()
    with pytest.raises(ValueError):
        pt.quantize_grouped(torch.zeros(256), dtype=torch.uint8, group_size=G)
    with pytest.raises(ValueError):
        pt.dequantize_grouped(torch.zeros(256, dtype=torch.uint8), torch.ones(8), torch.zeros(8, dtype=torch.uint8), dtype=torch.float32, group_size=G)


def test_quantized_input_rejected():
    with pytest.raises(ValueError):
        _pt().quantize_grouped(torch.zeros(256, dtype=torch.uint8), dtype=torch.uint8)


def test_one_of_scales_zero_points_rejected():
    pt = _pt()
    with pytest.raises(ValueError):
        pt.quantize_grouped(torch.zeros(256), dtype=torch.uint8, scales=torch.ones(2))
    with pytest.raises(ValueError):
        pt.quantize_grouped(torch.zeros(256), dtype=torch.uint8, zero_points=torch.zeros(2, dtype=torch.uint8))


@pytest.mark.parametrize("scales,zps", [
    (torch.ones(3), torch.zeros(2, dtype=torch.uint8)),                       # wrong length
    (torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.uint8)),  # wrong dtype
    (torch.ones(2), torch.zeros(2, dtype=torch.int32)),                       # wrong dtype
    (torch.ones(2, 1), torch.zeros(2, dtype=torch.uint8)),                    # not 1-D
])
def test_bad_given_params(scales, zps):
    pt = _pt()
    with pytest.raises(ValueError):
        pt.quantize_grouped(torch.zeros(256), dtype=torch.uint8, scales=scales, zero_points=zps)
    with pytest.raises(ValueError):
        pt.dequantize_grouped(torch.zeros(256, dtype=torch.uint8), scales, zps, dtype=torch.float32, group_size=128)


def test_bad_modes_rejected():
    pt = _pt()
    with pytest.raises(ValueError):
        pt.quantize_grouped(torch.zeros(256), dtype=torch.uint8, round_mode="up")
    with pytest.raises(ValueError):
        pt.dequantize_grouped(torch.zeros(256, dtype=torch.uint8), torch.ones(2), torch.zeros(2, dtype=torch.uint8), dtype=torch.float32,
                              group_size=128, reduce_op="mul")
    with pytest.raises(ValueError):
        pt.dequantize_grouped(torch.zeros(256, dtype=torch.uint8), torch.ones(2), torch.zeros(2, dtype=torch.uint8), dtype=torch.uint8, group_size=128)


def test_dequantize_grouped_rejects_cpu_tensor():
    with pytest.raises(ValueError):
        _pt().dequantize_grouped(torch.zeros(256, dtype=torch.uint8), torch.ones(2), torch.zeros(2, dtype=torch.uint8), dtype=torch.float32,
                                 group_size=128)


def test_num_groups():
    pt = _pt()
    assert pt.num_groups(0, 32) == 0 and pt.num_groups(1, 32) == 1 and pt.num_groups(64, 32) == 2 and pt.num_groups(65, 32) == 3
    assert pt.GROUP_SIZES == (32, 64, 128, 256, 512, 1024, 2048, 4096)
