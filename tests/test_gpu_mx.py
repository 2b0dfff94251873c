"""piquant_hip_quantize_mx / piquant_hip_dequantize_mx on the device against tests/mx_model.py, bit for bit, with guard bytes around every buffer.
The only slack is the definition's own: a NaN keeps neither payload nor sign (NaN codes and NaN floats are compared as "a NaN")."""
import numpy as np
import pytest

import mx_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMTS = [M.FP4, M.FP8]
FLOATS = ["float32", "bfloat16"]
GUARD = 64
TILE = {(M.FP4, "float32"): 2048, (M.FP8, "float32"): 1024, (M.FP4, "bfloat16"): 2048, (M.FP8, "bfloat16"): 2048}   # MxQuantTile::TILE_ELEMS
DTILE = {M.FP4: 4096, M.FP8: 2048}                                                                                   # MxDequantTile::TILE_ELEMS


@pytest.fixture(scope="module")
def ctx():
    import piquant

    torch.cuda.set_device(0)
    return piquant.Context.get(0)


class Buf:
    """nbytes of device memory `off` bytes behind a 16-byte boundary, between two runs of guard bytes."""

    def __init__(self, nbytes, off=0, fill=None):
        self.whole = torch.full((GUARD + off + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.whole[GUARD + off: GUARD + off + nbytes]
        assert self.whole.data_ptr() % 16 == 0
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).ravel()))

    def bytes(self):
        w = self.whole.cpu().numpy()
        assert (w[: w.size - GUARD - self.view.numel()] == 0xA5).all() and (w[-GUARD:] == 0xA5).all(), "guard bytes overwritten"
        return w[w.size - GUARD - self.view.numel(): w.size - GUARD]


def as_input(x32, dt):
    """float32 values -> what the device tensor holds (float32, or bfloat16 bits by truncation) and the same widened back to float32."""
    if dt == "float32":
        return x32, x32
    b = (x32.view(np.uint32) >> 16).astype(np.uint16)
    return b, M.bf16_to_f32(b)


def canon_codes(c, fmt):
    return np.where((c & 0x7F) == 0x7F, 0x7F, c) if fmt == M.FP8 else c


def canon_floats(raw, dt):
    if dt == "float32":
        u = raw.view(np.uint32)
        return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC00000, u)
    u = raw.view(np.uint16)
    return np.where((u & 0x7FFF) > 0x7F80, 0x7FC0, u)


def device_quantize(ctx, held, dt, fmt, off=(0, 0, 0)):
    import piquant
    import piquant.torch as T

    n, esize = held.size, held.itemsize
    nc, ns = T.mx_nbytes(n, fmt)
    x, codes, scales = Buf(n * esize, off[0] * esize, held), Buf(nc, off[1]), Buf(ns, off[2])
    ctx.set_stream(0)
    ctx.quantize_mx_ptr(x.view.data_ptr(), piquant.DataType.F32 if dt == "float32" else piquant.DataType.BF16, codes.view.data_ptr(), scales.view.data_ptr(), n,
                        T.MX_FORMATS[fmt], _device_ptrs=True)
    torch.cuda.synchronize()
    x.bytes()
    return codes.bytes(), scales.bytes()


def device_dequantize(ctx, raw, scales, n, fmt, dt, before=None, off=(0, 0, 0)):
    import piquant
    import piquant.torch as T

    esize = 4 if dt == "float32" else 2
    c, s, out = Buf(raw.size, off[1], raw), Buf(scales.size, off[2], scales), Buf(n * esize, off[0] * esize, before)
    ctx.set_stream(0)
    ctx.dequantize_mx_ptr(c.view.data_ptr(), s.view.data_ptr(), out.view.data_ptr(), piquant.DataType.F32 if dt == "float32" else piquant.DataType.BF16, n,
                          T.MX_FORMATS[fmt], piquant.ReduceOp.SET if before is None else piquant.ReduceOp.ADD, _device_ptrs=True)
    torch.cuda.synchronize()
    c.bytes(), s.bytes()
    return out.bytes().view(np.float32 if dt == "float32" else np.uint16)


def windows_of(n):
    """Everything, or for a long tensor three block-aligned windows: both ends and the middle."""
    w = 3 * 4096
    return [(0, n)] if n <= 4 * w else [(0, w), (n // 2 // w * w, n // 2 // w * w + w), (n // w * w - w, n)]


def check_quantize(ctx, x32, dt, fmt, off=(0, 0, 0)):
    held, wide = as_input(np.ascontiguousarray(x32, np.float32), dt)
    raw, scales = device_quantize(ctx, held, dt, fmt, off)
    got = M.unpack(raw, wide.size, fmt)
    for lo, hi in windows_of(wide.size):
        want_codes, want_scales = M.quantize(wide[lo:hi], fmt)
        assert np.array_equal(scales[lo // M.BLOCK: -(-hi // M.BLOCK)], want_scales)
        bad = np.flatnonzero(canon_codes(got[lo:hi], fmt) != canon_codes(want_codes, fmt))
        assert bad.size == 0, (lo, bad[:8], wide[lo:hi][bad[:8]], got[lo:hi][bad[:8]], want_codes[bad[:8]])
    if fmt == M.FP4 and wide.size % 2:
        assert raw[-1] >> 4 == 0
    return raw, scales


def check_dequantize(ctx, raw, scales, n, fmt, dt, before=None, off=(0, 0, 0)):
    got = device_dequantize(ctx, raw, scales, n, fmt, dt, before, off)
    codes = M.unpack(raw, n, fmt)
    for lo, hi in windows_of(n):
        want = M.store(M.dequantize(codes[lo:hi], scales[lo // M.BLOCK: -(-hi // M.BLOCK)], fmt), None if before is None else before[lo:hi], dt == "bfloat16")
        bad = np.flatnonzero(canon_floats(got[lo:hi], dt) != canon_floats(want, dt))
        assert bad.size == 0, (lo, bad[:8], got[lo:hi][bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_every_code_under_every_scale(ctx, fmt, dt, add):
    ncodes = 16 if fmt == M.FP4 else 256
    per = max(ncodes, M.BLOCK)                                          # elements under one scale byte: whole blocks holding every code
    codes = np.tile((np.arange(per) % ncodes).astype(np.uint8), 256)
    scales = np.repeat(np.arange(256, dtype=np.uint8), per // M.BLOCK)
    before = None
    if add:   # ordinary values, zeros of both signs, infinities, the largest float, a denormal and bfloat16 ties: 1 and 1 + 2^-7 under a term of 2^-8
        pre = np.array([1.0, -2.5, 0.0, -0.0, np.inf, -np.inf, 3.3895e38, 1.0078125, 1e-40, -0.375, 448.0], np.float32)
        before = as_input(np.resize(pre, codes.size), dt)[0]
    check_dequantize(ctx, M.pack(codes, fmt), scales, codes.size, fmt, dt, before)


def edge_blocks(fmt, dt):
    """The encode table: for every exponent field and mantissa of a block's maximum, blocks whose other 31 elements sweep every midpoint between
    adjacent codes and its two neighbours in the input type, in both signs, with a NaN, zeros and values that underflow; then the special blocks."""
    step = 1 if dt == "float32" else 0x10000
    emax, sat = M.EMAX[fmt], 0x400000 if fmt == M.FP4 else 0x600000   # 6 = 1.5 * 2^2, 448 = 1.75 * 2^8
    mags = M.code_values(fmt)[: M.TOP[fmt] + 1]
    mids = ((mags[:-1] + mags[1:]) / 2).astype(np.float32).view(np.uint32)
    blocks, place = [], 0
    for field in (0, 1, emax - 1, emax, emax + 1, 127, 200, 254, 255):
        for mant in (0, sat - step, sat + step, 0x7FFFFF & ~(step - 1)):
            top = np.uint32((field << 23) | mant)
            s = max(max(field, 1) - emax, 0)
            t = np.concatenate([mids - step, mids, mids + step]).view(np.float32).astype(np.float64)
            with np.errstate(over="ignore"):
                x = np.ldexp(t, s - 127).astype(np.float32)
            x = x[(np.ldexp(x.astype(np.float64), 127 - s) == t) & ((x.view(np.uint32) & (step - 1)) == 0)]   # what the input type represents exactly
            tiny = np.ldexp(1.0, s - 127 - 12)
            x = np.concatenate([x, -x, np.array([0.0, -0.0, np.nan, tiny, -tiny], np.float32)])
            keep = (x.view(np.uint32) & 0x7FFFFFFF) <= top if (top & 0x7FFFFFFF) <= 0x7F800000 else np.ones(x.size, bool)
            x = x[keep | np.isnan(x)]
            for i in range(0, x.size, 31):
                b = np.zeros(32, np.float32)
                chunk = x[i: i + 31]
                pos = (0, 31, 7, 8, 16, 5)[place % 6]                 # first, last, and around the lane boundaries of both float types
                place += 1
                b[np.delete(np.arange(32), pos)[: chunk.size]] = chunk
                b.view(np.uint32)[pos] = top
                blocks.append(b)
    nan = np.full(32, np.nan, np.float32)
    beside = nan.copy()
    beside[[3, 4]] = [5.0, -1000.0]
    both = np.linspace(-3, 3, 32, dtype=np.float32)
    both[[0, 31]] = [np.inf, -np.inf]
    blocks += [np.zeros(32, np.float32), nan, beside, both, -np.zeros(32, np.float32)]
    return np.concatenate(blocks)


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_encode_edges(ctx, fmt, dt):
    check_quantize(ctx, edge_blocks(fmt, dt), dt, fmt)


def random_blocks(n, seed):
    """Every block its own magnitude, its maximum at a position drawn from a seeded permutation."""
    rng = np.random.default_rng(seed)
    nb = -(-n // M.BLOCK)
    x = rng.uniform(-1, 1, (nb, M.BLOCK)).astype(np.float32)
    x[np.arange(nb), rng.permutation(nb) % M.BLOCK] = rng.choice(np.array([1.0, -1.0, 1.49, 1.51, 1.76, 1.99], np.float32), nb)
    return (x * np.ldexp(1.0, rng.integers(-30, 30, (nb, 1))).astype(np.float32)).ravel()[:n]


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_shapes(ctx, fmt, dt):
    sizes = {0, 1, 31, 32, 33, 63}
    for t in (TILE[fmt, dt], DTILE[fmt]):                               # the wave tiles of both kernels; a block of threads is four of them
        sizes |= {t - 1, t, t + 33, 4 * t + t + 5}
    sizes.add(3 * 256 * 4 * TILE[fmt, dt] - 7)                          # three times one block of threads per CU, less 7: checked in windows
    for n in sorted(sizes):
        if n == 0:
            assert device_quantize(ctx, np.zeros(0, np.float32), "float32", fmt)[0].size == 0
            continue
        raw, scales = check_quantize(ctx, random_blocks(n, n), dt, fmt)
        check_dequantize(ctx, raw, scales, n, fmt, dt)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_misaligned_buffers_give_the_same_bytes(ctx, fmt, dt, which):
    n = TILE[fmt, dt] + 33
    off = tuple(1 if k == which else 0 for k in range(3))              # the float side one element, codes or scales one byte off 16
    x = random_blocks(n, 7)
    x[[5, 40, n - 1]] = [np.nan, np.inf, -np.inf]
    raw, scales = check_quantize(ctx, x, dt, fmt, off)
    before = as_input(random_blocks(n, 8), dt)[0]
    check_dequantize(ctx, raw, scales, n, fmt, dt, None, off)
    check_dequantize(ctx, raw, scales, n, fmt, dt, before, off)


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_public_path(ctx, fmt, dt):
    import piquant.torch as T

    tdt = getattr(torch, dt)
    held, wide = as_input(random_blocks(3 * 2048 + 45, 3).reshape(-1, 3), dt)
    x = torch.from_numpy(held).cuda().view(tdt) if dt == "bfloat16" else torch.from_numpy(held).cuda()
    codes, scales = T.quantize_mx(x, format=fmt)
    back = T.dequantize_mx(codes, scales, format=fmt, dtype=tdt, shape=x.shape)
    wc, ws = M.quantize(wide, fmt)
    assert np.array_equal(codes.cpu().numpy(), M.pack(wc, fmt)) and np.array_equal(scales.cpu().numpy(), ws) and back.shape == x.shape
    want = M.store(M.dequantize(wc, ws, fmt), None, dt == "bfloat16")
    assert np.array_equal(back.view(torch.int16 if dt == "bfloat16" else torch.float32).cpu().numpy().ravel().view(want.dtype), want)
    s32 = scales.view(torch.float8_e8m0fnu).float().repeat_interleave(M.BLOCK)[: x.numel()]
    assert np.array_equal(s32.cpu().numpy(), np.ldexp(1.0, np.repeat(ws.astype(int), M.BLOCK)[: x.numel()] - 127).astype(np.float32))
    if fmt == M.FP8:
        assert np.array_equal((codes.view(torch.float8_e4m3fn).float() * s32).cpu().numpy(), M.dequantize(wc, ws, fmt))
    else:
        assert codes.view(torch.float4_e2m1fn_x2).shape == codes.shape

    # one capture of both calls, replayed on two inputs, against the eager results above and the model
    graph = torch.cuda.CUDAGraph()
    gx, gc, gs, gb = torch.zeros_like(x), torch.zeros_like(codes), torch.zeros_like(scales), torch.zeros_like(back)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        T.quantize_mx(gx, format=fmt, out=gc, out_scales=gs)
        T.dequantize_mx(gc, gs, format=fmt, dtype=tdt, out=gb)
    for src in (x, -2 * x, x):
        gx.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = T.dequantize_mx(*T.quantize_mx(src, format=fmt), format=fmt, dtype=tdt, shape=x.shape)
        assert torch.equal(gb.view(torch.int16 if dt == "bfloat16" else torch.int32), eager.view(torch.int16 if dt == "bfloat16" else torch.int32))
    assert torch.equal(gc, codes) and torch.equal(gs, scales)


def test_large_index(ctx):
    """2^32 + 40 037 bfloat16 elements into FP4: windows at both ends and across 2^32 against the model (element, code-byte and scale indices there)."""
    import piquant.torch as T

    if torch.cuda.get_device_properties(0).total_memory < 80 * 2**30:
        pytest.skip("needs ~30 GB of HBM")
    n, w = 2**32 + 40_037, 3 * 4096
    x = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    x[: 2**32].view(2**16, 2**16).normal_()
    x[: 2**32].view(2**16, 2**16).mul_(torch.pow(2.0, (torch.arange(2**16, device="cuda") % 41 - 20).float()).to(torch.bfloat16)[:, None])
    x[2**32:].normal_()
    codes, scales = T.quantize_mx(x, format=M.FP4)
    back = T.dequantize_mx(codes, scales, format=M.FP4, dtype=torch.bfloat16, shape=(n,))
    torch.cuda.synchronize()
    for lo, hi in ((0, w), (2**32 - w, 2**32 + w), (n - 40_037 - w, n)):
        wide = M.bf16_to_f32(x[lo:hi].view(torch.int16).cpu().numpy().view(np.uint16))
        wc, ws = M.quantize(wide, M.FP4)
        assert np.array_equal(codes[lo // 2: (hi + 1) // 2].cpu().numpy(), M.pack(wc, M.FP4)) and np.array_equal(scales[lo // 32: (hi + 31) // 32].cpu().numpy(), ws)
        assert np.array_equal(back[lo:hi].view(torch.int16).cpu().numpy().view(np.uint16), M.bf16_bits(M.dequantize(wc, ws, M.FP4)))
