"""The MX wire's four calls on the device -- piquant_hip_reduce_quantize_mx, piquant_hip_dequantize_sum_mx and the two batches -- bit for bit against
tests/mx_model.py composed as include/piquant_hip.h defines them, with guard bytes around every buffer.  The only slack is test_gpu_mx.py's: NaN
codes and NaN floats are compared as "a NaN"."""
import numpy as np
import pytest

import mx_model as M
from test_gpu_mx import Buf, as_input, canon_codes, canon_floats, random_blocks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMTS = [M.FP4, M.FP8]
FLOATS = ["float32", "bfloat16"]
SIZES = [1, 33, 2049, 20_517]   # a ragged block, the first block boundary, the first tile boundary, a block of threads + a tile + a ragged tile


@pytest.fixture(scope="module")
def ctx():
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    c.set_stream(0)
    return c


def pq_dtype(dt):
    import piquant

    return piquant.DataType.F32 if dt == "float32" else piquant.DataType.BF16


def fmt_code(fmt):
    import piquant.torch as T

    return T.MX_FORMATS[fmt]


def make_terms(n, fmt, count, seed):
    """count terms (unpacked codes, scales) of n elements whose blocks span exponents; the first holds zeros of both signs."""
    terms = []
    for i in range(count):
        x = random_blocks(n, seed + i)
        x[:: 7] = -0.0 if i == 0 else x[:: 7]
        terms.append(M.quantize(x, fmt))
    return terms


def model_sum(held, terms, fmt, dt, set_first=False):
    """The composition: dequantize_mx of term 0 with SET or ADD, the others ADD, the sum rounded to dt after each term."""
    cur = None if set_first else held
    for codes, scales in terms:
        cur = M.store(M.dequantize(codes, scales, fmt), cur, dt == "bfloat16")
    return cur


def widen(held, dt):
    return held if dt == "float32" else M.bf16_to_f32(held)


def term_bufs(terms, fmt, off=(0, 0)):
    return [(Buf(M.pack(c, fmt).size, off[0], M.pack(c, fmt)), Buf(s.size, off[1], s)) for c, s in terms]


def device_reduce(ctx, held, terms, fmt, dt, off=(0, 0, 0)):
    """off: acc one element, every code buffer / every scale buffer (terms and result) one byte off 16."""
    import piquant.torch as T

    n = held.size
    nc, ns = T.mx_nbytes(n, fmt)
    acc, tb = Buf(held.nbytes, off[0] * held.itemsize, held), term_bufs(terms, fmt, off[1:])
    codes, scales = Buf(nc, off[1]), Buf(ns, off[2])
    ctx.reduce_quantize_mx_ptr(acc.view.data_ptr(), pq_dtype(dt), [c.view.data_ptr() for c, _ in tb], [s.view.data_ptr() for _, s in tb], codes.view.data_ptr(),
                               scales.view.data_ptr(), n, fmt_code(fmt), _device_ptrs=True)
    torch.cuda.synchronize()
    assert np.array_equal(acc.bytes(), held.view(np.uint8)), "acc was written"
    for c, s in tb:
        c.bytes(), s.bytes()
    return M.unpack(codes.bytes(), n, fmt), scales.bytes()


def check_reduce(ctx, held, terms, fmt, dt, off=(0, 0, 0)):
    got_codes, got_scales = device_reduce(ctx, held, terms, fmt, dt, off)
    want_codes, want_scales = M.quantize(widen(model_sum(held, terms, fmt, dt), dt), fmt)
    assert np.array_equal(got_scales, want_scales)
    bad = np.flatnonzero(canon_codes(got_codes, fmt) != canon_codes(want_codes, fmt))
    assert bad.size == 0, (bad[:8], got_codes[bad[:8]], want_codes[bad[:8]])
    return got_codes


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("count", [0, 1, 2, 16])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_quantize(ctx, fmt, dt, count, n):
    check_reduce(ctx, as_input(random_blocks(n, n + count), dt)[0], make_terms(n, fmt, count, 100 * n), fmt, dt)


def test_reduce_quantize_refuses_17_terms():
    import piquant.torch as T

    acc = torch.zeros(64, device="cuda")
    terms = [(torch.zeros(32, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda"))] * 17
    with pytest.raises(ValueError):
        T.reduce_quantize_mx(acc, terms, format=M.FP4)


CODE = {M.FP4: {"2^-8": (1, 120), "2^127": (4, 253), "-inf": (0xF, 254)}, M.FP8: {"2^-8": (0x38, 119), "2^127": (0x40, 253), "-inf": (0xFE, 254)}}


def special_case(case, fmt, dt):
    """(acc values, terms) of 2049 elements: ordinary blocks with the case's blocks in front."""
    n = 2049
    x = random_blocks(n, 11)
    rng = np.random.default_rng(12)
    if case == "scale_bytes":   # hand-written scale bytes 0 and 0xFF and, for FP8, NaN codes
        codes = rng.integers(0, 16 if fmt == M.FP4 else 256, n).astype(np.uint8)
        if fmt == M.FP8:
            codes[[3, 40, 2048]] = [0x7F, 0xFF, 0x7F]
        scales = np.resize(np.array([0, 0xFF, 127, 1, 254], np.uint8), -(-n // 32))
        x[:64] = 2.0 ** -140                                          # denormal sums under scale byte 0
        return x, [(codes, scales), M.quantize(random_blocks(n, 13), fmt)]
    one = lambda name: (np.full(n, CODE[fmt][name][0], np.uint8), np.full(-(-n // 32), CODE[fmt][name][1], np.uint8))   # noqa: E731
    if case == "bf16_round_every_term":   # the block's maximum keeps the scale; 1.25 (FP4) / 1.3125 (FP8) sits on a code midpoint, even in bfloat16
        x[:32] = 1.25 if fmt == M.FP4 else 1.3125
        x[0] = 4.0 if fmt == M.FP4 else 256.0
        return x, [one("2^-8"), one("2^-8")]
    if case == "overflow":                # 3e38 + 2^127 overflows float32: the code saturates, in both signs
        x[:64] = 3e38
        x[32:64] *= -1
        t = one("2^127")
        t[0][32:64] |= M.SIGN[fmt]
        return x, [t]
    x[:32] = np.inf                       # "inf_minus_inf": +inf meets a term that decodes to -inf
    x[5] = 1.0
    return x, [one("-inf")]


@pytest.mark.parametrize("case", ["scale_bytes", "bf16_round_every_term", "overflow", "inf_minus_inf"])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_quantize_specials(ctx, fmt, dt, case):
    x, terms = special_case(case, fmt, dt)
    held = as_input(x, dt)[0]
    got = check_reduce(ctx, held, terms, fmt, dt)
    if case == "bf16_round_every_term" and dt == "bfloat16":   # rounding once instead (the float32 sum, rounded at the end) gives other codes
        once = M.bf16_bits(model_sum(widen(held, dt), terms, fmt, "float32"))
        assert not np.array_equal(M.quantize(widen(once, dt), fmt)[0][:32], got[:32])
    if case == "overflow":
        assert (got[:32] == M.TOP[fmt]).all() and (got[32:64] == (M.TOP[fmt] | M.SIGN[fmt])).all()
    if case == "inf_minus_inf":
        assert (canon_codes(np.delete(got[:32], 5), fmt) == (0 if fmt == M.FP4 else 0x7F)).all()


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_quantize_misaligned_gives_the_same_bytes(ctx, fmt, dt, which):
    n = 2049 + 33
    x = random_blocks(n, 5)
    x[[5, 40, n - 1]] = [np.nan, np.inf, -np.inf]
    check_reduce(ctx, as_input(x, dt)[0], make_terms(n, fmt, 2, 6), fmt, dt, tuple(1 if k == which else 0 for k in range(3)))


def check_sum(ctx, terms, n, fmt, dt, add, off=0):
    esize = 4 if dt == "float32" else 2
    before = as_input(random_blocks(n, 77), dt)[0] if add else as_input(np.full(n, np.nan, np.float32), dt)[0]   # SET must not read the NaNs
    out, tb = Buf(n * esize, off * esize, before), term_bufs(terms, fmt)
    import piquant

    ctx.dequantize_sum_mx_ptr([c.view.data_ptr() for c, _ in tb], [s.view.data_ptr() for _, s in tb], out.view.data_ptr(), pq_dtype(dt), n, fmt_code(fmt),
                              piquant.ReduceOp.ADD if add else piquant.ReduceOp.SET, _device_ptrs=True)
    torch.cuda.synchronize()
    got = out.bytes().view(np.float32 if dt == "float32" else np.uint16)
    want = model_sum(before, terms, fmt, dt, set_first=not add)
    bad = np.flatnonzero(canon_floats(got, dt) != canon_floats(want, dt))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("count", [1, 2, 16, 17])
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_dequantize_sum(ctx, fmt, dt, add, count, n):
    check_sum(ctx, make_terms(n, fmt, count, 300 * n), n, fmt, dt, add)


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_dequantize_sum_misaligned_out(ctx, fmt, dt, add):
    check_sum(ctx, make_terms(2049 + 33, fmt, 3, 9), 2049 + 33, fmt, dt, add, off=1)


@pytest.mark.parametrize("members", [1, 3, 17])
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_batches_equal_the_single_calls(ctx, fmt, dt, members):
    """Member i of both batches against the single call on the same bytes; with more than one member one is empty and one is misaligned."""
    import piquant
    import piquant.torch as T

    sizes = [SIZES[(i + 2) % 4] for i in range(members)]
    if members > 1:
        sizes[1] = 0
    esize = 4 if dt == "float32" else 2
    xs, cs, ss, outs, single = [], [], [], [], []
    for i, n in enumerate(sizes):
        off = 1 if members > 1 and i == 2 else 0
        nc, ns = T.mx_nbytes(n, fmt)
        xs.append(Buf(n * esize, off * esize, as_input(random_blocks(n, 40 + i), dt)[0]))
        cs.append(Buf(nc))
        ss.append(Buf(ns))
        outs.append(Buf(n * esize, off * esize))
        c1, s1, o1 = Buf(nc), Buf(ns), Buf(n * esize, off * esize)
        ctx.quantize_mx_ptr(xs[i].view.data_ptr(), pq_dtype(dt), c1.view.data_ptr(), s1.view.data_ptr(), n, fmt_code(fmt), _device_ptrs=True)
        ctx.dequantize_mx_ptr(c1.view.data_ptr(), s1.view.data_ptr(), o1.view.data_ptr(), pq_dtype(dt), n, fmt_code(fmt), piquant.ReduceOp.SET, _device_ptrs=True)
        single.append((c1, s1, o1))
    ptrs = lambda bufs: [b.view.data_ptr() for b in bufs]   # noqa: E731
    ctx.quantize_mx_batch_ptr(ptrs(xs), pq_dtype(dt), ptrs(cs), ptrs(ss), sizes, fmt_code(fmt), _device_ptrs=True)
    ctx.dequantize_mx_batch_ptr(ptrs(cs), ptrs(ss), ptrs(outs), pq_dtype(dt), sizes, fmt_code(fmt), piquant.ReduceOp.SET, _device_ptrs=True)
    torch.cuda.synchronize()
    for i, (c1, s1, o1) in enumerate(single):
        assert np.array_equal(cs[i].bytes(), c1.bytes()) and np.array_equal(ss[i].bytes(), s1.bytes()) and np.array_equal(outs[i].bytes(), o1.bytes()), i


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", FMTS)
def test_public_calls_in_one_captured_graph(ctx, fmt, dt):
    """piquant.torch's reduce_quantize_mx and dequantize_sum_mx in ONE capture, replayed twice on new inputs, against the eager calls and the model."""
    import piquant.torch as T

    n, tdt = 20_517, getattr(torch, dt)
    itype = torch.int16 if dt == "bfloat16" else torch.int32
    terms = make_terms(n, fmt, 2, 21)
    dev = [(torch.from_numpy(M.pack(c, fmt)).cuda(), torch.from_numpy(s).cuda()) for c, s in terms]
    helds = [as_input(random_blocks(n, 30 + k), dt)[0] for k in range(2)]
    acc, out = torch.zeros(n, dtype=tdt, device="cuda"), torch.zeros(n, dtype=tdt, device="cuda")
    rec = tuple(torch.zeros(k, dtype=torch.uint8, device="cuda") for k in T.mx_nbytes(n, fmt))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        T.reduce_quantize_mx(acc, dev, format=fmt, out=rec)
        T.dequantize_sum_mx(dev + [rec], format=fmt, out=out, reduce_op="add")
    for held in helds:
        x = torch.from_numpy(held.view(np.int16 if dt == "bfloat16" else np.float32)).cuda().view(tdt)
        acc.copy_(x)
        out.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager = T.reduce_quantize_mx(x, dev, format=fmt)
        assert torch.equal(rec[0], eager[0]) and torch.equal(rec[1], eager[1])
        assert torch.equal(out.view(itype), T.dequantize_sum_mx(dev + [eager], format=fmt, out=x.clone(), reduce_op="add").view(itype))
        want_codes, want_scales = M.quantize(widen(model_sum(held, terms, fmt, dt), dt), fmt)
        assert np.array_equal(canon_codes(M.unpack(rec[0].cpu().numpy(), n, fmt), fmt), canon_codes(want_codes, fmt))
        want = model_sum(held, terms + [(want_codes, want_scales)], fmt, dt)
        assert np.array_equal(canon_floats(out.view(itype).cpu().numpy().view(want.dtype), dt), canon_floats(want, dt))
