"""Fixed answers of tests/mx_model.py, the numpy form of the MX definition in include/piquant_hip.h, and the argument rules of piquant.torch's MX
calls that hold before anything moves."""
import numpy as np
import pytest

import mx_model as M

torch = pytest.importorskip("torch")


def test_every_code_at_scale_one():
    assert np.array_equal(M.dequantize(np.arange(16, dtype=np.uint8), np.array([127], np.uint8), M.FP4),
                          np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], np.float32))
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    got = M.dequantize(codes, np.full(8, 127, np.uint8), M.FP8)
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 2


def test_hand_computed_block():
    # amax 7.9: exponent field 129, s = 127 for E2M1 -- the scaled domain is the data; 7.0 and -7.9 saturate, 0.25 and 0.75 tie to the even code
    x = np.array([6.0, 7.0, -7.9, 0.25, 0.75, 1.25, -0.0, 5.0] + [0.0] * 24 + [3.0], np.float32)
    codes, scales = M.quantize(x, M.FP4)
    assert scales.tolist() == [127, 126]                          # the ragged second block: amax 3.0, field 128
    assert codes[:8].tolist() == [7, 7, 0xF, 0, 2, 2, 8, 6]       # 1.25 lies between codes 2 and 3, 5.0 between 6 and 7: the even one
    assert codes[32] == 7                                         # 3.0 * 2^(127 - 126) = 6.0
    assert M.pack(codes, M.FP4)[:4].tolist() == [0x77, 0x0F, 0x22, 0x68] and M.pack(codes, M.FP4).size == 17
    # E4M3: the same block has s = 129 - 8 = 121, v = x * 64: 7.0 -> 448 (exact), 7.9 -> 505.6 saturates to 448
    c8, s8 = M.quantize(x[:32], M.FP8)
    assert s8.tolist() == [121] and c8[:3].tolist() == [0x7C, 0x7E, 0xFE]


def test_small_exponents_clamp_the_scale_to_zero():
    for fmt in (M.FP4, M.FP8):
        for field in (0, 1, M.EMAX[fmt]):
            x = np.zeros(32, np.uint32)
            x[5] = (field << 23) | 0x400000
            assert M.quantize(x.view(np.float32), fmt)[1].tolist() == [0]
        x[5] = (M.EMAX[fmt] + 1) << 23
        assert M.quantize(x.view(np.float32), fmt)[1].tolist() == [1]
    x = np.full(32, np.inf, np.float32)
    x[0] = np.nan
    codes, scales = M.quantize(x, M.FP8)
    assert scales.tolist() == [247] and codes[1] == 0x7E and codes[0] == 0x7F


def test_argument_rules_hold_before_anything_moves():
    import piquant.torch as T

    x = torch.zeros(64)
    for call in (lambda: T.quantize_mx(x, format="fp6"), lambda: T.quantize_mx(x.to(torch.float16)), lambda: T.quantize_mx(x),
                 lambda: T.quantize_mx(x, out_scales=torch.zeros(3, dtype=torch.uint8)),
                 lambda: T.dequantize_mx(torch.zeros(32, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8), format="fp4_e2m1", dtype=torch.float32),
                 lambda: T.dequantize_mx(torch.zeros(32, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), format="fp8_e4m3", dtype=torch.float16),
                 lambda: T.dequantize_mx(torch.zeros(32, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), format="fp8_e4m3", dtype=torch.float32)):
        with pytest.raises(ValueError):
            call()
