"""tests/mx_fp6_model.py on hand-written values, and the argument rules of the FP6 formats in the wrappers: no GPU."""
import numpy as np
import pytest

import mx_fp6_model as M

torch = pytest.importorskip("torch")


def block(*head):
    x = np.zeros(32, np.float32)
    x[: len(head)] = head
    return x


def test_code_values():
    e2m3 = [0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875, 2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5,
            5.5, 6, 6.5, 7, 7.5]
    e3m2 = [0, .0625, .125, .1875, .25, .3125, .375, .4375, .5, .625, .75, .875, 1, 1.25, 1.5, 1.75, 2, 2.5, 3, 3.5, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20,
            24, 28]
    for fmt, mags in ((M.E2M3, e2m3), (M.E3M2, e3m2)):
        v = M.code_values(fmt)
        assert v[:32].tolist() == mags and v[32:].tolist() == [-m for m in mags] and np.signbit(v[32])


@pytest.mark.parametrize("fmt,top,inf_scale", [(M.E2M3, 7.5, 253), (M.E3M2, 28.0, 251)])
def test_quantize_by_hand(fmt, top, inf_scale):
    # the maximum 2^emax keeps the scale at 127: top and beyond saturate (the block's scale follows the largest element, so scale it down)
    codes, scales = M.quantize(block(top, -top, top * 1.06, np.nan, -0.0, -1e-6), fmt)
    assert scales.tolist() == [127] and codes[:6].tolist() == [0x1F, 0x3F, 0x1F, 0, 0x20, 0x20]
    # NaN is left out of amax; ties go to the even code: E2M3 1.0625 -> 1.0 (8), 1.1875 -> 1.25 (10); E3M2 1.125 -> 1.0 (12), 1.375 -> 1.5 (14)
    ties = (1.0625, 1.1875, 4.0) if fmt == M.E2M3 else (1.125, 1.375, 16.0)
    codes, scales = M.quantize(np.concatenate([block(np.nan, *ties), block(np.nan), block(np.inf, -np.inf, 3e38, 1.0)]), fmt)
    assert scales.tolist() == [127, 0, inf_scale]
    assert codes[:4].tolist() == ([0, 8, 10, 24] if fmt == M.E2M3 else [0, 12, 14, 28]) and codes[32:64].tolist() == [0] * 32
    # under an infinity: saturated codes, 3e38 * 2^-126 = 3.53 -> 3.5 (22), 3e38 * 2^-124 = 14.1 -> 14 (27)
    assert codes[64:68].tolist() == [0x1F, 0x3F, 22 if fmt == M.E2M3 else 27, 0]
    assert M.dequantize(np.array([0x1F, 0x3F, 1], np.uint8), np.array([128], np.uint8), fmt).tolist() == [2 * top, -2 * top, 2 * M.code_values(fmt)[1]]
    assert np.isnan(M.dequantize(np.array([5], np.uint8), np.array([255], np.uint8), fmt)).all()


def test_pack_by_hand():
    codes = np.array([0x01, 0x3F, 0x20, 0x15, 0x2A], np.uint8)          # 000001 111111 100000 010101 101010, element 0 lowest: 30 bits, 4 bytes
    want = 0x01 | 0x3F << 6 | 0x20 << 12 | 0x15 << 18 | 0x2A << 24
    assert M.pack(codes).tolist() == [want & 0xFF, want >> 8 & 0xFF, want >> 16 & 0xFF, want >> 24 & 0xFF] == [0xC1, 0x0F, 0x56, 0x2A]
    assert M.unpack(M.pack(codes), 5).tolist() == codes.tolist() and M.pack(np.full(32, 0x3F, np.uint8)).tolist() == [0xFF] * 24


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_argument_rules(fmt):
    import piquant.distributed as D
    import piquant.torch as T

    assert T.MX_FORMATS[M.E2M3] == 2 and T.MX_FORMATS[M.E3M2] == 3
    assert [T.mx_nbytes(n, fmt) for n in (1, 2, 3, 4, 5, 32, 33)] == [(1, 1), (2, 1), (3, 1), (3, 1), (4, 1), (24, 1), (25, 2)]
    x, r = torch.zeros(64), torch.zeros(64)
    term = tuple(torch.zeros(k, dtype=torch.uint8) for k in T.mx_nbytes(64, fmt))
    for call in (lambda: T.quantize_mx_batch([x], format=fmt), lambda: T.reduce_quantize_mx(x, [term], format=fmt),
                 lambda: T.dequantize_sum_mx([term], format=fmt, out=x), lambda: T.quantize_mx_ef(x, r, format=fmt),
                 lambda: D.quantized_all_reduce(x, mx_format=fmt), lambda: D.mx_wire_layout(64, fmt), lambda: T.quantize_mx(x, format="fp6")):
        with pytest.raises(ValueError):
            call()
    assert not x.any() and not r.any()
