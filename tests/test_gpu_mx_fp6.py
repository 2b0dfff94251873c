"""The MXFP6 formats through piquant_hip_quantize_mx / piquant_hip_dequantize_mx on the device against tests/mx_fp6_model.py, bit for bit, with guard
bytes around every buffer (the buffers and calls of test_gpu_mx.py).  No tolerance: only NaN floats are compared as "a NaN"."""
import numpy as np
import pytest

import mx_fp6_model as M
from test_gpu_mx import as_input, canon_floats, ctx, device_dequantize, device_quantize  # noqa: F401  (ctx: the fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLOATS = ["float32", "bfloat16"]
TILE = 2048                                                              # kMx6TileElems: 64 blocks, one per lane; four tiles a workgroup
SAT = {M.E2M3: 0x700000, M.E3M2: 0x600000}                               # mantissa of the largest code: 7.5 = 1.875 * 2^2, 28 = 1.75 * 2^4
POW2 = {M.E2M3: 24, M.E3M2: 28}                                          # the code of 2^emax


def check_quantize(ctx, x32, dt, fmt, off=(0, 0, 0)):
    held, wide = as_input(np.ascontiguousarray(x32, np.float32), dt)
    raw, scales = device_quantize(ctx, held, dt, fmt, off)
    want, want_scales = M.quantize(wide, fmt)
    assert np.array_equal(scales, want_scales)
    got = M.unpack(raw, wide.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], wide[bad[:8]], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(raw, M.pack(want))                            # the spare bits of a ragged end are 0
    return raw, scales


def check_dequantize(ctx, raw, scales, n, fmt, dt, before=None, off=(0, 0, 0)):
    got = device_dequantize(ctx, raw, scales, n, fmt, dt, before, off)
    want = M.store(M.dequantize(M.unpack(raw, n), scales, fmt), before, dt == "bfloat16")
    bad = np.flatnonzero(canon_floats(got, dt) != canon_floats(want, dt))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    return got


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_decode_every_code_at_every_slot(ctx, fmt, dt, add):
    sbytes = np.array([0, 1, 2, 3, 64, 126, 127, 128, 200, 250, 251, 252, 253, 254, 255], np.uint8)
    table = ((np.arange(64)[:, None] + np.arange(32)) % 64).astype(np.uint8).ravel()    # block k holds codes (k + i) % 64
    codes, scales = np.tile(table, sbytes.size), np.repeat(sbytes, 64)
    before = None
    if add:   # ordinary values, zeros of both signs, infinities, the largest float, a denormal and bfloat16 ties: 1 and 1 + 2^-7 under terms of 2^-8 (1 + 2^-3)
        pre = np.array([1.0, -2.5, 0.0, -0.0, np.inf, -np.inf, 3.3895e38, 1.0078125, 1e-40, -0.375, 28.0], np.float32)
        before = as_input(np.resize(pre, codes.size), dt)[0]
    check_dequantize(ctx, M.pack(codes), scales, codes.size, fmt, dt, before)


def edge_blocks(fmt, dt):
    """For every exponent class and mantissa of a block's maximum -- denormal, s = 0, middle, the top finite exponent, infinity -- blocks whose other 31
    elements sweep every midpoint between adjacent code magnitudes that the input type holds under that scale and its two neighbours in the input
    type, in both signs, with a NaN, zeros and values that round to the zeros; then the special blocks."""
    step = 1 if dt == "float32" else 0x10000
    emax, sat = M.EMAX[fmt], SAT[fmt]
    mags = M.code_values(fmt)[: M.TOP + 1]
    mids = (mags[:-1] + mags[1:]) / 2
    blocks, place = [], 0
    for field in (0, 1, emax - 1, emax, emax + 1, 127, 200, 254, 255):
        for mant in (0, sat - step, sat + step, 0x7FFFFF & ~(step - 1)):    # around the saturation line; the last: (7.5, 8) / (28, 32)
            top = np.uint32((field << 23) | mant)
            s = max(max(field, 1) - emax, 0)
            with np.errstate(over="ignore"):
                m = np.ldexp(mids, s - 127).astype(np.float32)
            m = m[np.isfinite(m) & (np.ldexp(m.astype(np.float64), 127 - s) == mids) & ((m.view(np.uint32) & (step - 1)) == 0)].view(np.uint32)
            x = np.concatenate([m - step, m, m + step]).view(np.float32)
            tiny = np.float32(np.ldexp(1.0, s - 127 - 12))
            x = np.concatenate([x, -x, np.array([0.0, -0.0, np.nan, tiny, -tiny], np.float32)])
            x = x[((x.view(np.uint32) & 0x7FFFFFFF) <= min(top, np.uint32(0x7F800000))) & np.isfinite(x) | np.isnan(x)]
            for i in range(0, x.size, 31):
                b = np.zeros(32, np.float32)
                chunk = x[i: i + 31]
                pos = (0, 31, 7, 8, 16, 5)[place % 6]
                place += 1
                b[np.delete(np.arange(32), pos)[: chunk.size]] = chunk
                b.view(np.uint32)[pos] = top
                blocks.append(b)
    nan = np.full(32, np.nan, np.float32)
    beside = nan.copy()
    beside[[3, 4]] = [5.0, -1000.0]
    both = np.linspace(-3, 3, 32, dtype=np.float32)
    both[[0, 31]] = [np.inf, -np.inf]
    return np.concatenate(blocks + [np.zeros(32, np.float32), nan, beside, both, -np.zeros(32, np.float32)])


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_encode_edges(ctx, fmt, dt):
    check_quantize(ctx, edge_blocks(fmt, dt), dt, fmt)


def positional(n, fmt):
    """Element i quantizes to a code that depends on i: block b holds exact code values under its own power of two, its maximum 2^emax at slot 7 b % 32."""
    i = np.arange(-(-n // 32) * 32)
    b = i // 32
    code = np.where(i % 32 == (7 * b) % 32, POW2[fmt], (5 * i + b) % (POW2[fmt] + 1)) | np.where((i // 3) % 2, M.SIGN, 0)
    return np.ldexp(M.code_values(fmt)[code], b % 37 - 18).astype(np.float32)[:n]


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_positions_and_sizes(ctx, fmt, dt):
    for n in (1, 31, 32, 33, 46, TILE - 1, TILE, TILE + 1, TILE + 2, 5 * TILE + 37):   # numel % 4 = 1, 2, 3; a ragged tile in a second workgroup
        raw, scales = check_quantize(ctx, positional(n, fmt), dt, fmt)
        check_dequantize(ctx, raw, scales, n, fmt, dt)
    x = np.random.default_rng(5).uniform(-1, 1, (32, TILE)).astype(np.float32)           # tile t: the maximum of its first and last block at slot t
    x[np.arange(32), np.arange(32)] = 3.0
    x[np.arange(32), TILE - 32 + np.arange(32)] = -5.0
    raw, scales = check_quantize(ctx, x.ravel(), dt, fmt)
    check_dequantize(ctx, raw, scales, x.size, fmt, dt)


@pytest.mark.parametrize("off", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_misaligned_buffers_give_the_same_bytes(ctx, fmt, dt, off):
    n = TILE + 33                                                        # the float side one element, codes or scales one byte off 16
    x = positional(n, fmt)
    x[[5, 40, n - 1]] = [np.nan, np.inf, -np.inf]
    raw, scales = check_quantize(ctx, x, dt, fmt)
    raw_off, scales_off = check_quantize(ctx, x, dt, fmt, off)
    assert np.array_equal(raw, raw_off) and np.array_equal(scales, scales_off)
    for before in (None, as_input(positional(n, fmt)[::-1].copy(), dt)[0]):
        assert np.array_equal(check_dequantize(ctx, raw, scales, n, fmt, dt, before), check_dequantize(ctx, raw, scales, n, fmt, dt, before, off))


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_public_path_in_a_captured_graph(ctx, fmt, dt):
    import piquant.torch as T

    tdt, idt = getattr(torch, dt), torch.int16 if dt == "bfloat16" else torch.int32
    n = 3 * TILE + 45

    def on_device(x32):
        held = as_input(x32, dt)[0]
        return torch.from_numpy(held).cuda().view(tdt) if dt == "bfloat16" else torch.from_numpy(held).cuda()

    gx = torch.zeros(n, dtype=tdt, device="cuda")
    gc, gs = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in T.mx_nbytes(n, fmt))
    gb = torch.zeros(n, dtype=tdt, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        T.quantize_mx(gx, format=fmt, out=gc, out_scales=gs)
        T.dequantize_mx(gc, gs, format=fmt, dtype=tdt, out=gb)
    for x32 in (positional(n, fmt), -2 * positional(n, fmt)[::-1].copy(), positional(n, fmt)):
        gx.copy_(on_device(x32))
        graph.replay()
        torch.cuda.synchronize()
        wc, ws = M.quantize(as_input(x32, dt)[1], fmt)
        assert np.array_equal(gc.cpu().numpy(), M.pack(wc)) and np.array_equal(gs.cpu().numpy(), ws)
        want = M.store(M.dequantize(wc, ws, fmt), None, dt == "bfloat16")
        assert np.array_equal(gb.view(idt).cpu().numpy().view(want.dtype), want)
    back = T.dequantize_mx(gc, gs, format=fmt, dtype=tdt)               # no shape: the largest numel that fills the bytes
    assert back.numel() == gc.numel() * 8 // 6 and torch.equal(back[:n].view(idt), gb.view(idt))
