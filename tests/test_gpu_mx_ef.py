"""Error feedback on the MX wire on the device -- piquant_hip_quantize_mx_ef, its batch and piquant_hip_reduce_quantize_mx_ef -- bit for bit against
the composition include/piquant_hip.h defines them by, written over tests/mx_model.py: a float32 add, quantize, dequantize, a float32 subtract.
Guard bytes around every buffer; NaN codes and NaN floats are compared as "a NaN" (test_gpu_mx.py's only slack)."""
import numpy as np
import pytest

import mx_model as M
from test_gpu_mx import Buf, as_input, canon_codes, canon_floats
from test_gpu_mx_wire import ctx, fmt_code, make_terms, model_sum, pq_dtype, term_bufs, widen  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMTS = [M.FP4, M.FP8]
FLOATS = ["float32", "bfloat16"]
# a ragged block; a block + a ragged one, an odd count; a wave tile + a ragged one; past a block of threads, ragged for the 1024-element tile too
SIZES = [1, 33, 2048 + 31, 4 * 2048 + 1024 + 37]
RAGGED = SIZES[2]


def model_step(wide, res, fmt):
    """The definition: (codes, scales, the new residual) of float32 values `wide` and the float32 residual `res`."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = wide.astype(np.float32) + res
        codes, scales = M.quantize(y, fmt)
        return codes, scales, y - M.dequantize(codes, scales, fmt)


def special_blocks(fmt):
    """(x, y) of six hand-placed blocks: y = x + R is what the kernel must see (inputs() takes R = y - x from the x the tensor really holds -- a bfloat16
    tensor truncates 2 * 449 -- and every such difference is exact).  Ties on format
    midpoints under scale 2^0; the saturating part of the scaled domain; all zeros; x + R cancelling to +-0; a denormal y, alone and among normal
    values."""
    top, mids, sat = (4.0, [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], [6.5, 7.0, 7.75]) if fmt == M.FP4 else \
        (256.0, [2.0 ** -10, 3 * 2.0 ** -10, 1.0625, 1.1875, 17.0, 19.0, 136.0, 272.0, 464.0], [449.0, 470.0, 511.0])
    y = np.zeros((6, 32), np.float32)
    x = np.zeros((6, 32), np.float32)
    ties = np.array([top] + mids + [-m for m in mids], np.float32)
    y[0, : ties.size], x[0, : ties.size] = ties, ties / 2
    y[1, :7] = [top] + sat + [-s for s in sat]
    x[1] = y[1] * 2                                                     # R = -x / 2
    y[2, 1::2] = -0.0
    x[2] = y[2]
    y[3, :4], x[3, :4] = [1.0, 0.0, -0.0, 0.0], [1.0, 3.0, -0.0, -1.5]  # 3 + -3 -> +0, -0 + -0 -> -0, -1.5 + 1.5 -> +0
    y[4, :3], x[4, :3] = [2.0 ** -140, -3 * 2.0 ** -141, 2.0 ** -127], [2.0 ** -130, 0.0, 2.0 ** -127]
    y[5, :3], x[5, :3] = [1.0, 2.0 ** -135, -0.75], [0.5, 2.0 ** -132, -0.75]
    return x.ravel(), y.ravel()


def inputs(n, dt, fmt, seed, special=True):
    """(what the device tensor holds, the same widened to float32, the residual): blocks under exponents from -12 to 11 with a residual of their
    size, the special blocks in front (as far as n reaches), a NaN and the two infinities behind them."""
    rng = np.random.default_rng(seed)
    nb = -(-n // M.BLOCK)
    e = np.ldexp(1.0, rng.integers(-12, 12, (nb, 1)))
    x = (rng.uniform(-1, 1, (nb, M.BLOCK)) * e).astype(np.float32).ravel()[:n]
    res = (rng.uniform(-0.5, 0.5, (nb, M.BLOCK)) * e).astype(np.float32).ravel()[:n]
    sx, sy = special_blocks(fmt)
    k = min(n, sx.size) if special else 0
    x[:k] = sx[:k]
    if special and n > sx.size + 70:
        x[sx.size + 3], x[sx.size + 40], x[sx.size + 69] = np.nan, np.inf, -np.inf
    held, wide = as_input(x, dt)
    res[:k] = np.where((sy[:k] == 0) & np.signbit(sy[:k]), np.float32(-0.0), sy[:k] - wide[:k])   # -0 + -0: the only sum that is -0
    return held, wide, res


def device_ef(ctx, held, res, dt, fmt, off=(0, 0, 0, 0), terms=None):
    """One call on fresh buffers; off: x / the residual one element, codes / scales one byte off a 16-byte boundary.  terms: the fused reduce."""
    import piquant.torch as T

    n = held.size
    nc, ns = T.mx_nbytes(n, fmt)
    x, r = Buf(held.nbytes, off[0] * held.itemsize, held), Buf(4 * n, 4 * off[1], res)
    codes, scales = Buf(nc, off[2]), Buf(ns, off[3])
    ctx.set_stream(0)
    if terms is None:
        ctx.quantize_mx_ef_ptr(x.view.data_ptr(), pq_dtype(dt), r.view.data_ptr(), codes.view.data_ptr(), scales.view.data_ptr(), n, fmt_code(fmt),
                               _device_ptrs=True)
    else:
        tb = term_bufs(terms, fmt)
        ctx.reduce_quantize_mx_ef_ptr(x.view.data_ptr(), pq_dtype(dt), r.view.data_ptr(), [c.view.data_ptr() for c, _ in tb], [s.view.data_ptr() for _, s in tb],
                                      codes.view.data_ptr(), scales.view.data_ptr(), n, fmt_code(fmt), _device_ptrs=True)
    torch.cuda.synchronize()
    assert np.array_equal(x.bytes(), held.view(np.uint8)), "the input was written"
    return codes.bytes(), scales.bytes(), r.bytes().view(np.float32).copy()


def assert_step(got, want, n, fmt, what=""):
    raw, scales, res = got
    codes, want_scales, want_res = want
    assert np.array_equal(scales, want_scales), what
    bad = np.flatnonzero(canon_codes(M.unpack(raw, n, fmt), fmt) != canon_codes(codes, fmt))
    assert bad.size == 0, (what, bad[:8], M.unpack(raw, n, fmt)[bad[:8]], codes[bad[:8]])
    bad = np.flatnonzero(canon_floats(res, "float32") != canon_floats(want_res, "float32"))
    assert bad.size == 0, (what, bad[:8], res[bad[:8]], want_res[bad[:8]])
    if fmt == M.FP4 and n % 2:
        assert raw[-1] >> 4 == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_four_chained_steps_equal_the_composition(ctx, fmt, dt, n):
    res = None
    for step in range(4):   # the device's residual of step k is the input of step k + 1: its read-modify-write
        held, wide, fresh = inputs(n, dt, fmt, 10 * n + step, special=step == 0)
        res = fresh if res is None else res
        got = device_ef(ctx, held, res, dt, fmt)
        assert_step(got, model_step(wide, res, fmt), n, fmt, f"step {step}")
        res = got[2]


@pytest.mark.parametrize("off", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)], ids=["input", "residual", "codes"])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_misaligned_buffers_give_the_aligned_bytes(ctx, fmt, dt, off):
    held, wide, res = inputs(RAGGED, dt, fmt, 77)
    aligned, guarded = device_ef(ctx, held, res, dt, fmt), device_ef(ctx, held, res, dt, fmt, off)
    assert_step(guarded, model_step(wide, res, fmt), RAGGED, fmt)
    assert np.array_equal(guarded[0], aligned[0]) and np.array_equal(guarded[1], aligned[1])
    assert np.array_equal(canon_floats(guarded[2], "float32"), canon_floats(aligned[2], "float32"))


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_batch_members_equal_their_single_calls(ctx, fmt, dt):
    import piquant.torch as T

    sizes, offs = [SIZES[3], 0, RAGGED, 33], [0, 0, 1, 0]              # two share the launch; one is empty, one has its residual an element off
    data = [inputs(n, dt, fmt, 90 + i) for i, n in enumerate(sizes)]
    bufs = []
    for (held, _, res), o in zip(data, offs):
        nc, ns = T.mx_nbytes(held.size, fmt)
        bufs.append((Buf(held.nbytes, 0, held), Buf(4 * held.size, 4 * o, res), Buf(nc), Buf(ns)))
    ctx.set_stream(0)
    ptrs = [[b[k].view.data_ptr() for b in bufs] for k in range(4)]
    ctx.quantize_mx_ef_batch_ptr(ptrs[0], pq_dtype(dt), ptrs[1], ptrs[2], ptrs[3], sizes, fmt_code(fmt), _device_ptrs=True)
    torch.cuda.synchronize()
    for (held, _, res), o, b in zip(data, offs, bufs):
        if held.size == 0:
            continue
        single = device_ef(ctx, held, res, dt, fmt, (0, o, 0, 0))
        assert np.array_equal(b[2].bytes(), single[0]) and np.array_equal(b[3].bytes(), single[1])
        assert np.array_equal(canon_floats(b[1].bytes().view(np.float32), "float32"), canon_floats(single[2], "float32"))
        assert np.array_equal(b[0].bytes(), held.view(np.uint8))


@pytest.mark.parametrize("off", [(0, 0, 0, 0), (0, 1, 0, 0)], ids=["streaming", "guarded"])
@pytest.mark.parametrize("count", [0, 1, 16])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_adds_the_residual_behind_the_terms(ctx, fmt, dt, count, off):
    held, _, res = inputs(RAGGED, dt, fmt, 300 + count)
    terms = make_terms(RAGGED, fmt, count, 400)
    total = widen(model_sum(held, terms, fmt, dt), dt)                  # the sum as reduce_quantize_mx forms it, rounded to dt after each term
    assert_step(device_ef(ctx, held, res, dt, fmt, off, terms), model_step(total, res, fmt), RAGGED, fmt)


def test_reduce_refuses_17_terms():
    import piquant.torch as T

    acc, res = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    terms = [(torch.zeros(32, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda"))] * 17
    with pytest.raises(ValueError):
        T.reduce_quantize_mx_ef(acc, res, terms, format=M.FP4)
    assert not res.any()


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_captured_graph_replayed_twice_equals_two_eager_steps(fmt, dt):
    import piquant.torch as T

    held, wide, res0 = inputs(SIZES[3], dt, fmt, 55, special=False)
    x = torch.from_numpy(held.view(np.int16)).cuda().view(torch.bfloat16) if dt == "bfloat16" else torch.from_numpy(held).cuda()
    res = torch.from_numpy(res0).cuda()
    out = tuple(torch.empty(k, dtype=torch.uint8, device="cuda") for k in T.mx_nbytes(held.size, fmt))
    T.quantize_mx_ef(x, res.clone(), format=fmt)                       # warm-up outside capture (code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.quantize_mx_ef(x, res, format=fmt, out=out)
    res.copy_(torch.from_numpy(res0))
    eager_res = torch.from_numpy(res0).cuda()
    for step in range(2):
        graph.replay()
        eager = T.quantize_mx_ef(x, eager_res, format=fmt)
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and torch.equal(res.view(torch.int32), eager_res.view(torch.int32)), step
    assert_step((out[0].cpu().numpy(), out[1].cpu().numpy(), res.cpu().numpy()), model_step(wide, model_step(wide, res0, fmt)[2], fmt), held.size, fmt)
