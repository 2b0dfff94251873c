"""Group-wise quantize-dequantize on the MI355X (piquant_hip_quantize_dequantize_grouped / _batch and the piquant.torch wrappers): bit for bit the
CPU model dequantize_grouped(quantize_grouped(x)) of tests/grouped_model.py and the device composition quantize_grouped -> dequantize_grouped,
for SET and ADD, computed and given parameters, no parameter arrays, in place, misaligned buffers (the guarded kernel), batches, graph capture,
a side stream and a blocking context; 64 guard bytes of 0xAA behind everything written, the input unchanged unless in place.  NaNs compare by
position."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle as O
from grouped_edge_cases import edge_tensor
from grouped_model import dequantize_grouped, group_params_all, quantize_grouped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
GUARD = 64
ALL_G = [32, 64, 128, 256, 512, 1024, 2048, 4096]


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)


def _dev(a: np.ndarray, front: int = 0):
    """numpy array -> device uint8 buffer with `front` bytes of 0xAA in front of it and GUARD behind; returns (buffer, view of the data)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((front + raw.size + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    if raw.size:
        buf[front: front + raw.size].copy_(torch.from_numpy(raw.copy()))
    return buf, buf[front: front + raw.size]


def _guard_ok(buf, front, n):
    return bool((buf[:front] == 0xAA).all()) and bool((buf[front + n:] == 0xAA).all())


def widen(a, dt):
    return O.bf16_to_f32(a) if dt == O.BF16 else a


def _narrow(xf, dt):
    return O.f32_to_bf16(xf) if dt == O.BF16 else xf


def make_input(n, dt, seed):
    """Normal data with a varying magnitude and a few planted outliers, and a non-zero accumulator of the same magnitude."""
    rng = np.random.default_rng(seed)
    mag = np.repeat(rng.uniform(0.01, 50.0, n // 97 + 1), 97)[:n]
    xf = (rng.standard_normal(n) * mag).astype(np.float32)
    if n > 10:
        xf[rng.choice(n, max(1, n // 5000), replace=False)] *= 100.0
    af = (rng.standard_normal(n) * mag * 0.7 + 0.3).astype(np.float32)
    return _narrow(xf, dt), _narrow(af, dt)


def gpu_requant(ctx, x, dt, qd, G, mode=O.NEAREST, acc=None, given=None, in_place=False, add=False, shift=False, params=True):
    """One call on guarded buffers -> (out, scales, zero points) on the host (scales / zero points None with params=False).  acc: ADD onto this
    accumulator.  given: (scales, zero_points) to quantize with.  in_place: out is in (SET, or ADD with add=True).  shift: in and out start one
    element behind a 16-byte boundary (the guarded kernel).  Guard bytes around everything written are checked, and x must be unchanged unless
    in place."""
    import piquant

    n = x.size
    ng = (n + G - 1) // G
    esize = x.dtype.itemsize
    front = esize if shift else 0
    add = add or acc is not None
    xbuf, xin = _dev(x, front)
    if in_place:
        obuf, out = xbuf, xin
    else:
        obuf, out = _dev(acc if acc is not None else np.full(n * esize, 0xAA, dtype=np.uint8).view(x.dtype), front)
    if shift and n:
        assert xin.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
    sbuf, sv = _dev(given[0] if given else np.zeros(ng, dtype=np.float32))
    zbuf, zv = _dev(given[1] if given else np.zeros(ng, dtype=np.uint8))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_dequantize_grouped_ptr(xin.data_ptr(), piquant.DataType(dt), out.data_ptr(), piquant.DataType(qd), n, G, sv.data_ptr() if params else 0,
                                        zv.data_ptr() if params else 0, given is not None, piquant.RoundMode(mode),
                                        piquant.ReduceOp.ADD if add else piquant.ReduceOp.SET, _device_ptrs=True)
    torch.cuda.synchronize()
    assert _guard_ok(obuf, front, n * esize), "wrote outside out"
    assert _guard_ok(sbuf, 0, 4 * ng), "wrote past the end of scales"
    assert _guard_ok(zbuf, 0, ng), "wrote past the end of zero_points"
    if not in_place:
        assert _guard_ok(xbuf, front, n * esize) and np.array_equal(xin.cpu().numpy(), x.view(np.uint8).reshape(-1)), "the input was written"
    s, z = sv.cpu().numpy().view(np.float32), zv.cpu().numpy()
    if given:
        assert np.array_equal(s.view(np.uint32), given[0].view(np.uint32)) and np.array_equal(z, given[1]), "given parameters were written"
    if not params:
        assert not s.any() and not z.any(), "parameters were written though none were wanted"
        s = z = None
    return out.cpu().numpy().view(x.dtype), s, z


def assert_same(got, want, dt, what=""):
    """bit for bit, NaNs by position"""
    with np.errstate(invalid="ignore"):
        gn, wn = np.isnan(widen(got, dt)), np.isnan(widen(want, dt))
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8]}"
    gb, wb = (got, want) if dt == O.BF16 else (got.view(np.uint32), want.view(np.uint32))
    bad = np.flatnonzero((gb != wb) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:8]}: got {got[bad[:4]]} want {want[bad[:4]]}"


def assert_params(s, z, ws, wz, what=""):
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), f"{what}: scales differ at groups {np.flatnonzero(s.view(np.uint32) != ws.view(np.uint32))[:8]}"
    assert np.array_equal(z, wz), f"{what}: zero points differ at groups {np.flatnonzero(z != wz)[:8]}"


class Model:
    """dequantize_grouped(quantize_grouped(x)) for several rounding modes and both ops; the computed parameters once."""

    def __init__(self, x, dt, qd, G, params=None):
        self.x, self.dt, self.qd, self.G = x, dt, qd, G
        self.s, self.z = params if params is not None else group_params_all(widen(x, dt), G, qd)

    def out(self, mode=O.NEAREST, tau=0.0, acc=None):
        """-> (SET result, ADD result onto acc or None)"""
        q, _, _ = quantize_grouped(self.x, self.dt, self.qd, self.G, mode, tau, params=(self.s, self.z))
        d = dequantize_grouped(q, self.qd, self.dt, self.x.size, self.G, self.s, self.z)
        a = None if acc is None else dequantize_grouped(q, self.qd, self.dt, self.x.size, self.G, self.s, self.z, O.ADD, prev=acc)
        return d, a


# ---- 1. parity with the CPU model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_parity_with_the_model(ctx, dt, qd, G):
    for i, n in enumerate([1, 31, G - 1, G, G + 1, 10 * G + 7, 1_000_003]):
        x, acc = make_input(n, dt, seed=3000 * G + 10 * i + qd)
        if n == 10 * G + 7:   # NaNs in the input and in the accumulator, compared by position
            x, acc = x.copy(), acc.copy()
            x[[3, G + 1, n - 1]] = np.uint16(0x7FC0) if dt == O.BF16 else np.float32(np.nan)
            acc[[5, n - 2]] = np.uint16(0x7FC0) if dt == O.BF16 else np.float32(np.nan)
        model = Model(x, dt, qd, G)
        for mode, tau in [(O.NEAREST, 0.0), (O.STOCHASTIC, 0.0), (O.STOCHASTIC, 0.37), (O.STOCHASTIC, 0.999)]:
            ctx.set_stochastic_threshold(tau if mode == O.STOCHASTIC else None)
            what = f"n={n} G={G} mode={mode} tau={tau}"
            want_set, want_add = model.out(mode, tau, acc)
            d, s, z = gpu_requant(ctx, x, dt, qd, G, mode)
            assert_params(s, z, model.s, model.z, what)
            assert_same(d, want_set, dt, what + " SET")
            d, s, z = gpu_requant(ctx, x, dt, qd, G, mode, acc=acc)
            assert_params(s, z, model.s, model.z, what)
            assert_same(d, want_add, dt, what + " ADD")
    ctx.set_stochastic_threshold(None)


# ---- 2. the device composition ----------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _device_tensor(n, fdt, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g) * torch.linspace(0.05, 20.0, n, device="cuda")).to(fdt)


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_equals_the_two_public_calls_on_the_device(ctx, dt, qd):
    import piquant.torch as pt

    G = 128
    for n in (10 * G + 7, 1_000_003):
        x = _device_tensor(n, FDT[dt], 5 + qd)
        x0 = x.clone()
        acc = _device_tensor(n, FDT[dt], 50 + qd)
        q, ws, wz = pt.quantize_grouped(x, dtype=QDT[qd], group_size=G)
        want_set = pt.dequantize_grouped(q, ws, wz, dtype=FDT[dt], group_size=G)
        want_add = pt.dequantize_grouped(q, ws, wz, dtype=FDT[dt], group_size=G, reduce_op="add", out=acc.clone())
        d, s, z = pt.quantize_dequantize_grouped(x, quant_dtype=QDT[qd], group_size=G, return_params=True)
        a, s2, z2 = pt.quantize_dequantize_grouped(x, quant_dtype=QDT[qd], group_size=G, reduce_op="add", out=acc, return_params=True)
        torch.cuda.synchronize()
        assert a is acc and torch.equal(_bits(x), _bits(x0))
        assert torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz) and torch.equal(s2.view(torch.int32), ws.view(torch.int32)) and torch.equal(z2, wz)
        assert torch.equal(_bits(d), _bits(want_set)), n
        assert torch.equal(_bits(a), _bits(want_add)), n


# ---- 3. given parameters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,qd", PAIRS)
def test_given_parameters(ctx, dt, qd):
    """The parameters a computed call returned give the same out; deliberately wrong ones (scales doubled) match the model with them."""
    G, n = 128, 20 * 128 * 16 + 77
    x, acc = make_input(n, dt, seed=77 + qd)
    d, s, z = gpu_requant(ctx, x, dt, qd, G)
    dg, _, _ = gpu_requant(ctx, x, dt, qd, G, given=(s, z))
    assert_same(dg, d, dt, "given == computed")
    wrong = ((s * np.float32(2.0)).astype(np.float32), z)
    model = Model(x, dt, qd, G, params=wrong)
    want_set, want_add = model.out(acc=acc)
    dw, _, _ = gpu_requant(ctx, x, dt, qd, G, given=wrong)
    assert_same(dw, want_set, dt, "scales doubled, SET")
    aw, _, _ = gpu_requant(ctx, x, dt, qd, G, given=wrong, acc=acc)
    assert_same(aw, want_add, dt, "scales doubled, ADD")
    sw, _, _ = gpu_requant(ctx, x, dt, qd, G, given=wrong, shift=True)
    assert_same(sw, want_set, dt, "scales doubled, guarded kernel")


# ---- 4. all eight group sizes on the rounding edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", ALL_G)
def test_rounding_edges_on_three_paths(ctx, dt, qd, G):
    """edge_tensor (ties, the 1e9 line, NaNs of both kinds, denormals, +-0, infinities, constant groups) through the streaming kernel, the
    call with given parameters and the guarded kernel (in and out one element off a 16-byte boundary): each against the model, and so against
    one another."""
    bits, lay = edge_tensor(dt, qd, G, 0)
    x = bits.view(np.float32) if dt == O.F32 else bits
    model = Model(x, dt, qd, G)
    want, _ = model.out()
    d, s, z = gpu_requant(ctx, x, dt, qd, G)
    assert_params(s, z, model.s, model.z, "streaming")
    dg, _, _ = gpu_requant(ctx, x, dt, qd, G, given=(model.s, model.z))
    ds, ss, zs = gpu_requant(ctx, x, dt, qd, G, shift=True)
    assert_params(ss, zs, model.s, model.z, "guarded")
    for name, got in (("streaming", d), ("given", dg), ("guarded", ds)):
        with np.errstate(invalid="ignore"):
            gn, wn = np.isnan(widen(got, dt)), np.isnan(widen(want, dt))
        assert np.array_equal(gn, wn), f"{name}: NaN positions differ, first at {lay.describe_element(int(np.flatnonzero(gn != wn)[0]))}"
        bad = np.flatnonzero((got != want) & ~wn) if dt == O.BF16 else np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~wn)
        assert bad.size == 0, f"{name}: {bad.size} elements differ from the model, first at {lay.describe_element(int(bad[0]))}"
    assert_same(dg, d, dt, "given vs streaming")
    assert_same(ds, d, dt, "guarded vs streaming")


# ---- 5. in place, 6. no parameter arrays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("shift", [False, True])
def test_in_place_equals_out_of_place(ctx, dt, qd, shift):
    G, n = 128, 70_003
    x, _ = make_input(n, dt, seed=500 + qd)
    for mode, tau in ((O.NEAREST, 0.0), (O.STOCHASTIC, 0.37)):
        ctx.set_stochastic_threshold(tau if mode == O.STOCHASTIC else None)
        want, ws, wz = gpu_requant(ctx, x, dt, qd, G, mode, shift=shift)
        got, s, z = gpu_requant(ctx, x, dt, qd, G, mode, in_place=True, shift=shift)
        assert_params(s, z, ws, wz)
        assert_same(got, want, dt, f"in place SET mode={mode}")
    ctx.set_stochastic_threshold(None)
    want, ws, wz = gpu_requant(ctx, x, dt, qd, G, acc=x, shift=shift)          # x += d(q(x)), out of place onto a copy of x
    got, s, z = gpu_requant(ctx, x, dt, qd, G, in_place=True, add=True, shift=shift)
    assert_params(s, z, ws, wz)
    assert_same(got, want, dt, "in place ADD")


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_no_parameter_arrays(ctx, dt, qd):
    import piquant.torch as pt

    G, n = 64, 50_021
    x, acc = make_input(n, dt, seed=600 + qd)
    for shift in (False, True):
        want, _, _ = gpu_requant(ctx, x, dt, qd, G, shift=shift)
        got, s, z = gpu_requant(ctx, x, dt, qd, G, shift=shift, params=False)
        assert s is None and z is None
        assert_same(got, want, dt, f"no parameter arrays, shift={shift}")
        wa, _, _ = gpu_requant(ctx, x, dt, qd, G, acc=acc, shift=shift)
        ga, _, _ = gpu_requant(ctx, x, dt, qd, G, acc=acc, shift=shift, params=False)
        assert_same(ga, wa, dt, f"no parameter arrays, ADD, shift={shift}")
    xt = _device_tensor(n, FDT[dt], 9)
    a = pt.quantize_dequantize_grouped(xt, quant_dtype=QDT[qd], group_size=G)
    b, _, _ = pt.quantize_dequantize_grouped(xt, quant_dtype=QDT[qd], group_size=G, return_params=True)
    assert isinstance(a, torch.Tensor) and torch.equal(_bits(a), _bits(b))


# ---- 7. batch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdt,qdt,op", [(torch.float32, torch.quint4x2, "set"), (torch.bfloat16, torch.uint8, "add"), (torch.float32, torch.quint2x4, "add")])
def test_batch_equals_the_single_calls(ctx, fdt, qdt, op):
    """19 tensors -- more than one launch's 16; an empty one, one of a single element, a misaligned one and one of 1 000 003 among them -- with
    stochastic rounding and a pinned threshold: member by member the bytes and parameters of the single call.  A batch of one too."""
    import piquant.torch as pt

    G = 128
    sizes = [3_000 + 1237 * i for i in range(19)]
    sizes[4], sizes[9], sizes[17] = 0, 1, 1_000_003
    whole = [_device_tensor(n + 1, fdt, 40 + i) for i, n in enumerate(sizes)]
    xs = [w[1:] if i == 7 else w[:n].clone() for i, (w, n) in enumerate(zip(whole, sizes))]   # tensor 7: misaligned input
    accs = [_device_tensor(n, fdt, 140 + i) + 0.5 for i, n in enumerate(sizes)]
    assert xs[7].data_ptr() % 16 != 0
    ctx.set_stochastic_threshold(0.37)
    try:
        singles = []
        for x, a in zip(xs, accs):
            o, s, z = pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G, round_mode="stochastic", reduce_op=op,
                                                     out=a.clone() if op == "add" else None, return_params=True)
            singles.append((o, s, z))
        outs = [a.clone() for a in accs] if op == "add" else None
        got, ss, zs = pt.quantize_dequantize_grouped_batch(xs, quant_dtype=qdt, group_size=G, round_mode="stochastic", reduce_op=op, outs=outs,
                                                           return_params=True)
        bare = pt.quantize_dequantize_grouped_batch(xs, quant_dtype=qdt, group_size=G, round_mode="stochastic", reduce_op=op,
                                                    outs=[a.clone() for a in accs] if op == "add" else None)
        one = pt.quantize_dequantize_grouped_batch([xs[17]], quant_dtype=qdt, group_size=G, round_mode="stochastic", reduce_op=op,
                                                   outs=[accs[17].clone()] if op == "add" else None)
        given = pt.quantize_dequantize_grouped_batch(xs, quant_dtype=qdt, group_size=G, round_mode="stochastic", reduce_op=op, scales=ss, zero_points=zs,
                                                     outs=[a.clone() for a in accs] if op == "add" else None)
        torch.cuda.synchronize()
    finally:
        ctx.set_stochastic_threshold(None)
    for i, (wo, ws, wz) in enumerate(singles):
        assert got[i].shape == xs[i].shape and torch.equal(_bits(got[i]), _bits(wo)), i
        assert torch.equal(ss[i].view(torch.int32), ws.view(torch.int32)) and torch.equal(zs[i], wz), i
        assert torch.equal(_bits(bare[i]), _bits(wo)), i
        assert torch.equal(_bits(given[i]), _bits(wo)), i
    assert len(one) == 1 and torch.equal(_bits(one[0]), _bits(singles[17][0]))
    assert torch.equal(_bits(whole[7][:1]), _bits(_device_tensor(sizes[7] + 1, fdt, 47)[:1])), "wrote in front of the misaligned member"


# ---- 8. graph capture, a side stream, a blocking context ---------------------------------------------------------------------------------
def test_graph_capture_side_stream_and_blocking_context(ctx):
    import piquant
    import piquant.torch as pt

    n, G, qdt = 1_000_003, 128, torch.quint4x2
    x = torch.empty(n, device="cuda")
    acc = torch.zeros(n, device="cuda")
    out = torch.empty(n, device="cuda")
    inputs = [_device_tensor(n, torch.float32, 70 + i) for i in range(2)]
    x.copy_(inputs[0])
    pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G, out=out)   # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G, out=out)
        pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G, reduce_op="add", out=acc)
    want_acc = torch.zeros(n, device="cuda")
    for fresh in inputs:
        x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        want = pt.quantize_dequantize_grouped(fresh, quant_dtype=qdt, group_size=G)
        pt.quantize_dequantize_grouped(fresh, quant_dtype=qdt, group_size=G, reduce_op="add", out=want_acc)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(acc), _bits(want_acc))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y = torch.empty(1 << 22, device="cuda")
        y.normal_()
        y.mul_(3.0).add_(1.0)   # still in flight when the call is enqueued behind it on the same stream
        got = pt.quantize_dequantize_grouped(y, quant_dtype=torch.uint8, group_size=G)
    side.synchronize()
    q, s, z = pt.quantize_grouped(y, dtype=torch.uint8, group_size=G)
    want = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=G)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))

    blocking = piquant.Context(1)   # blocking, on its own stream: the result is complete when the call returns
    res = torch.full((1 << 22,), -1.0, device="cuda")
    torch.cuda.synchronize()
    blocking.quantize_dequantize_grouped_ptr(y.data_ptr(), piquant.DataType.F32, res.data_ptr(), piquant.DataType.UINT8, y.numel(), G, 0, 0, False,
                                             piquant.RoundMode.NEAREST, piquant.ReduceOp.SET)
    assert torch.equal(_bits(res), _bits(want))
    blocking.quantize_dequantize_grouped_batch_ptr([y.data_ptr(), x.data_ptr()], piquant.DataType.F32, [res.data_ptr(), out.data_ptr()], piquant.DataType.UINT8,
                                                   [y.numel(), 0], G, None, None, False, piquant.RoundMode.NEAREST, piquant.ReduceOp.ADD)
    torch.cuda.synchronize()
    assert torch.equal(_bits(res), _bits(want + want))


# ---- 9. contract violations --------------------------------------------------------------------------------------------------------------
SINGLE, BATCH = "piquant_hip_quantize_dequantize_grouped", "piquant_hip_quantize_dequantize_grouped_batch"


@pytest.mark.parametrize("snippet,needles", [
    ("C.piquant_hip_quantize_dequantize_grouped(ctx, p, 0, p, 4, 64, 48, s, z, 0, 0, 0)", (SINGLE + ":", "group size 48")),
    ("C.piquant_hip_quantize_dequantize_grouped(ctx, p, 0, p, 1, 64, 32, s, z, 0, 0, 0)", (SINGLE + ":", "must be a quantized type")),
    ("C.piquant_hip_quantize_dequantize_grouped(ctx, p, 3, p, 4, 64, 32, s, z, 0, 0, 0)", (SINGLE + ":", "must be a dequantized type")),
    ("C.piquant_hip_quantize_dequantize_grouped(ctx, p, 0, p, 4, 64, 32, s, None, 0, 0, 0)", (SINGLE + ":", "NULL")),
    ("C.piquant_hip_quantize_dequantize_grouped(ctx, p, 0, p, 4, 64, 32, None, None, 1, 0, 0)", (SINGLE + ":", "NULL")),
    ("C.piquant_hip_quantize_dequantize_grouped(ctx, h, 0, p, 4, 64, 32, s, z, 0, 0, 0)", (SINGLE + ":", "device (or pinned) buffers")),
    ("C.piquant_hip_quantize_dequantize_grouped_batch(ctx, arr(p), 0, arr(p), 4, n64, 8192, arr(s), arr(z), 1, 0, 0, 0)", (BATCH + ":", "group size 8192")),
    ("C.piquant_hip_quantize_dequantize_grouped_batch(ctx, arr(p), 0, arr(h), 4, n64, 32, arr(s), arr(z), 1, 0, 0, 0)",
     (BATCH + ":", "device (or pinned) buffers", "list index 0")),
])
def test_contract_violations_abort_with_a_message_naming_the_entry(snippet, needles):
    code = textwrap.dedent(f"""
        import sys; sys.path.insert(0, {str(os.path.join(os.path.dirname(__file__), '..', 'pi-quant_amd'))!r})
        import ctypes
        import numpy, torch, piquant
        from piquant._bootstrap import C_LIB as C
        t = torch.zeros(64, device='cuda'); p = t.data_ptr()
        s = torch.zeros(2, device='cuda').data_ptr(); z = torch.zeros(2, dtype=torch.uint8, device='cuda').data_ptr()
        host = numpy.zeros(64, dtype=numpy.float32); h = host.ctypes.data
        arr = lambda v: (ctypes.c_void_p * 1)(v)
        n64 = (ctypes.c_size_t * 1)(64)
        ctx = C.piquant_context_create(1)
        {snippet}
        print('survived')
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == -6, (r.returncode, r.stderr[-500:])   # SIGABRT
    assert all(n in r.stderr for n in needles) and "survived" not in r.stdout, r.stderr[-500:]
