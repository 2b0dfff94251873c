"""Error-feedback group-wise quantization on the MI355X (piquant_hip_quantize_grouped_ef / _batch and the piquant.torch wrappers): bit-exact
against the CPU model (tests/ef_model.py) and against the device composition torch.add -> quantize_grouped -> dequantize_grouped -> torch.sub,
guard bytes behind every buffer that is written, misaligned buffers, batches, graph capture, a side stream, and the conservation identity."""
import numpy as np
import pytest

import oracle as O
from ef_model import EPS, add_t, sub_t, widen
from grouped_model import dequantize_grouped, group_params_all, quantize_grouped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
GUARD = 64


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)


def _dev(a: np.ndarray):
    """numpy array -> device uint8 buffer with GUARD bytes of 0xAA behind it; returns (buffer, view of the data)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((raw.size + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    if raw.size:
        buf[: raw.size].copy_(torch.from_numpy(raw.copy()))
    return buf, buf[: raw.size]


def _guard_ok(buf, n):
    return bool((buf[n:] == 0xAA).all())


def _narrow(xf, dt):
    return O.f32_to_bf16(xf) if dt == O.BF16 else xf


def make_input(n, dt, seed):
    """Normal data with a varying magnitude and a few planted outliers, and a residual of about a percent of it (non-zero on entry)."""
    rng = np.random.default_rng(seed)
    mag = np.repeat(rng.uniform(0.01, 50.0, n // 97 + 1), 97)[:n]
    xf = (rng.standard_normal(n) * mag).astype(np.float32)
    if n > 10:
        xf[rng.choice(n, max(1, n // 5000), replace=False)] *= 100.0
    rf = (rng.standard_normal(n) * mag * 0.01).astype(np.float32)
    return _narrow(xf, dt), _narrow(rf, dt)


def gpu_ef(ctx, x, r, dt, qd, G, mode=O.NEAREST):
    """One error-feedback call on guarded buffers; -> (packed bytes, scales, zero points, new residual) on the host.  Guard bytes behind out,
    scales, zero points and the residual are checked, and x must be unchanged."""
    import piquant

    n = x.size
    ng = (n + G - 1) // G
    nbytes = O.packed_numel(n, qd)
    esize = x.dtype.itemsize
    xbuf, xin = _dev(x)
    rbuf, rin = _dev(r)
    obuf, _ = _dev(np.full(nbytes, 0xAA, dtype=np.uint8))
    sbuf, _ = _dev(np.zeros(ng, dtype=np.float32))
    zbuf, _ = _dev(np.zeros(ng, dtype=np.uint8))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_ef_ptr(xin.data_ptr(), piquant.DataType(dt), rin.data_ptr(), obuf.data_ptr(), piquant.DataType(qd), n, G, sbuf.data_ptr(),
                                zbuf.data_ptr(), piquant.RoundMode(mode), _device_ptrs=True)
    torch.cuda.synchronize()
    assert _guard_ok(obuf, nbytes), "wrote past the end of out"
    assert _guard_ok(sbuf, 4 * ng), "wrote past the end of scales"
    assert _guard_ok(zbuf, ng), "wrote past the end of zero_points"
    assert _guard_ok(rbuf, n * esize), "wrote past the end of the residual"
    assert _guard_ok(xbuf, n * esize) and np.array_equal(xbuf[: n * esize].cpu().numpy(), x.view(np.uint8).reshape(-1)), "the input was written"
    return (obuf[:nbytes].cpu().numpy(), sbuf[: 4 * ng].cpu().numpy().view(np.float32), zbuf[:ng].cpu().numpy(),
            rbuf[: n * esize].cpu().numpy().view(x.dtype))


def assert_residual_equal(got, want, dt, what=""):
    """bit for bit, NaNs by position"""
    gn, wn = np.isnan(widen(got, dt)), np.isnan(widen(want, dt))
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8]}"
    bad = np.flatnonzero((got != want) & ~wn) if dt == O.BF16 else np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} residual elements differ, first at {bad[:8]}: got {got[bad[:4]]} want {want[bad[:4]]}"


class Model:
    """The model of one call for several rounding modes: y and the parameters are computed once."""

    def __init__(self, x, r, dt, qd, G):
        self.dt, self.qd, self.G = dt, qd, G
        self.y = add_t(x, r, dt)
        self.s, self.z = group_params_all(widen(self.y, dt), G, qd)

    def step(self, mode=O.NEAREST, tau=0.0):
        q, _, _ = quantize_grouped(self.y, self.dt, self.qd, self.G, mode, tau, params=(self.s, self.z))
        d = dequantize_grouped(q, self.qd, self.dt, self.y.size, self.G, self.s, self.z)
        return q, sub_t(self.y, d, self.dt)


def check_against_model(ctx, x, r, dt, qd, G, model, mode=O.NEAREST, tau=0.0):
    q, s, z, rn = gpu_ef(ctx, x, r, dt, qd, G, mode)
    what = f"n={x.size} G={G} mode={mode} tau={tau}"
    assert np.array_equal(s.view(np.uint32), model.s.view(np.uint32)), f"{what}: scales differ at groups {np.flatnonzero(s.view(np.uint32) != model.s.view(np.uint32))[:8]}"
    assert np.array_equal(z, model.z), f"{what}: zero points differ at groups {np.flatnonzero(z != model.z)[:8]}"
    wq, wr = model.step(mode, tau)
    bad = np.flatnonzero(q != wq)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at byte {bad[:8]}"
    assert_residual_equal(rn, wr, dt, what)


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_parity_nearest_and_stochastic(ctx, dt, qd, G):
    for i, n in enumerate([1, 31, G - 1, G, G + 1, 10 * G + 7, 1_000_003]):
        x, r = make_input(n, dt, seed=2000 * G + 10 * i + qd)
        if n == 10 * G + 7:   # NaNs in the input: they stay NaNs in the residual, and they are compared by position
            x = x.copy()
            x[[3, G + 1, n - 1]] = np.uint16(0x7FC0) if dt == O.BF16 else np.float32(np.nan)
        model = Model(x, r, dt, qd, G)
        ctx.set_stochastic_threshold(None)
        check_against_model(ctx, x, r, dt, qd, G, model, O.NEAREST)
        for tau in (0.0, 0.37, 0.999):
            ctx.set_stochastic_threshold(tau)
            check_against_model(ctx, x, r, dt, qd, G, model, O.STOCHASTIC, tau)
    ctx.set_stochastic_threshold(None)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _device_pair(n, fdt, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = (torch.randn(n, device="cuda", generator=g) * torch.linspace(0.05, 20.0, n, device="cuda")).to(fdt)
    r = (torch.randn(n, device="cuda", generator=g) * 0.05).to(fdt)
    return x, r


def _composition(x, r, qdt, G, mode="nearest"):
    """the four launches the fused call replaces -> (packed bytes, scales, zero points, new residual)"""
    import piquant.torch as pt

    y = torch.add(x, r)
    q, s, z = pt.quantize_grouped(y, dtype=qdt, group_size=G, round_mode=mode)
    d = pt.dequantize_grouped(q, s, z, dtype=x.dtype, group_size=G)
    return pt.packed_bytes(q), s, z, torch.sub(y, d)


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4)])
def test_equals_the_device_composition_at_the_flagship_size(ctx, dt, qd):
    import piquant.torch as pt

    n, G = 27_264_000, 128
    x, r = _device_pair(n, FDT[dt], 5)
    x0 = x.clone()
    wq, ws, wz, wr = _composition(x, r, QDT[qd], G)
    q, s, z = pt.quantize_grouped_ef(x, r, dtype=QDT[qd], group_size=G)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(x0))
    assert torch.equal(pt.packed_bytes(q), wq) and torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz)
    assert torch.equal(_bits(r), _bits(wr))


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4), (O.F32, O.UINT2)])
@pytest.mark.parametrize("which", ["x", "residual", "out"])
def test_misaligned_buffers_take_the_guarded_path(ctx, dt, qd, which):
    """x or the residual shifted by one element, out by one byte: the same bytes as the composition, nothing written outside."""
    import piquant.torch as pt

    n, G = 100_003, 128
    fdt = FDT[dt]
    x, r = _device_pair(n + 1, fdt, 6)
    x, r = (x[1:], r[:n].clone()) if which == "x" else (x[:n].clone(), r[1:]) if which == "residual" else (x[:n].clone(), r[:n].clone())
    whole_r = r._base if r._base is not None else None
    first = whole_r[0].clone() if whole_r is not None else None
    nbytes = O.packed_numel(n, qd)
    obuf = torch.full((nbytes + 1 + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    off = 1 if which == "out" else 0
    out = obuf[off: off + nbytes]
    assert {"x": x, "residual": r, "out": out}[which].data_ptr() % 16 != 0
    wq, ws, wz, wr = _composition(x, r, QDT[qd], G)
    s = torch.empty((n + G - 1) // G, dtype=torch.float32, device="cuda")
    z = torch.empty((n + G - 1) // G, dtype=torch.uint8, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    import piquant

    ctx.quantize_grouped_ef_ptr(x.data_ptr(), piquant.DataType(dt), r.data_ptr(), out.data_ptr(), piquant.DataType(qd), n, G, s.data_ptr(), z.data_ptr(),
                                piquant.RoundMode.NEAREST, _device_ptrs=True)
    torch.cuda.synchronize()
    assert torch.equal(out, wq) and torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz)
    assert torch.equal(_bits(r), _bits(wr))
    assert bool((obuf[:off] == 0xAA).all()) and bool((obuf[off + nbytes:] == 0xAA).all()), "wrote outside out"
    if first is not None:
        assert torch.equal(_bits(whole_r[:1]), _bits(first.reshape(1))), "wrote in front of the residual"


def test_batch_equals_the_single_calls(ctx):
    """17 pairs -- an empty one and a misaligned one among them --: tensor by tensor the bytes, parameters and residuals of the single call."""
    import piquant.torch as pt

    G = 128
    sizes = [40_000 + 1237 * i for i in range(17)]
    sizes[4] = 0
    sizes[9] = 5
    for fdt, qdt in ((torch.float32, torch.quint4x2), (torch.bfloat16, torch.uint8)):
        pairs = [_device_pair(n + 1, fdt, 40 + i) for i, n in enumerate(sizes)]
        xs = [p[0][1:] if i == 7 else p[0][:n].clone() for i, (p, n) in enumerate(zip(pairs, sizes))]   # tensor 7: misaligned input
        rs = [p[1][:n].clone() for p, n in zip(pairs, sizes)]
        assert xs[7].data_ptr() % 16 != 0
        singles = []
        for x, r in zip(xs, rs):
            rr = r.clone()
            q, s, z = pt.quantize_grouped_ef(x, rr, dtype=qdt, group_size=G)
            singles.append((pt.packed_bytes(q), s, z, rr))
        outs, ss, zs = pt.quantize_grouped_ef_batch(xs, rs, dtype=qdt, group_size=G)
        torch.cuda.synchronize()
        for i, (wq, ws, wz, wr) in enumerate(singles):
            assert torch.equal(pt.packed_bytes(outs[i]), wq) and torch.equal(ss[i].view(torch.int32), ws.view(torch.int32)) and torch.equal(zs[i], wz), i
            assert torch.equal(_bits(rs[i]), _bits(wr)), i
        wq, ws, wz, wr = _composition(xs[3], pairs[3][1][:sizes[3]].clone(), qdt, G)
        assert torch.equal(pt.packed_bytes(outs[3]), wq) and torch.equal(_bits(rs[3]), _bits(wr))


def test_graph_capture_replay_and_side_stream(ctx):
    """A 3-step chain (nearest) captured once and replayed twice gives the bytes and the residual of 6 eager steps; a side stream works."""
    import piquant.torch as pt

    n, G, qdt = 1_000_003, 128, torch.quint4x2
    xs = [_device_pair(n, torch.float32, 70 + i)[0] for i in range(3)]
    res = torch.zeros(n, device="cuda")
    eager = []
    for t in range(6):
        q, s, z = pt.quantize_grouped_ef(xs[t % 3], res, dtype=qdt, group_size=G)
        eager.append((pt.packed_bytes(q).clone(), s.clone(), z.clone()))
    torch.cuda.synchronize()
    want_res = res.clone()
    assert bool((want_res != 0).any())

    res.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = [pt.quantize_grouped_ef(xs[t], res, dtype=qdt, group_size=G) for t in range(3)]
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for t in range(3):
        q, s, z = captured[t]
        wq, ws, wz = eager[3 + t]
        assert torch.equal(pt.packed_bytes(q), wq) and torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz), t
    assert torch.equal(res.view(torch.int32), want_res.view(torch.int32))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.empty(1 << 22, device="cuda")
        x.normal_()
        x.mul_(3.0).add_(1.0)   # still in flight when the call is enqueued behind it on the same stream
        r = torch.zeros_like(x)
        r.add_(0.01)
        q, s, z = pt.quantize_grouped_ef(x, r, dtype=torch.uint8, group_size=G)
    side.synchronize()
    wq, ws, wz, wr = _composition(x, torch.full_like(x, 0.01), torch.uint8, G)
    torch.cuda.synchronize()
    assert torch.equal(pt.packed_bytes(q), wq) and torch.equal(s, ws) and torch.equal(z, wz) and torch.equal(r.view(torch.int32), wr.view(torch.int32))


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_conservation_on_the_device(ctx, dt, qd):
    """K = 16 chained steps on the device: S = sum_t d_t + r_K - sum_t x_t in float64 on the host stays within K eps_T M (two roundings to T per
    step, each at most half an ulp; M the largest |y| or |d| seen).  d_t comes from dequantize_grouped of the step's bytes; finite inputs."""
    import piquant.torch as pt

    n, G, K = 200_003, 128, 16
    fdt = FDT[dt]
    fixed = _device_pair(n, fdt, 90)[0]
    fixed[G: 2 * G] = 7.25                                           # one constant group, far from zero
    res = torch.zeros(n, dtype=fdt, device="cuda")
    S = np.zeros(n, dtype=np.float64)
    M = 0.0
    for t in range(K):
        x = fixed if t % 2 == 0 else _device_pair(n, fdt, 100 + t)[0]
        y = torch.add(x, res)
        q, s, z = pt.quantize_grouped_ef(x, res, dtype=QDT[qd], group_size=G)
        d = pt.dequantize_grouped(q, s, z, dtype=fdt, group_size=G)
        S += d.double().cpu().numpy() - x.double().cpu().numpy()
        M = max(M, float(y.float().abs().max()), float(d.float().abs().max()))
    S += res.double().cpu().numpy()
    defect, bound = float(np.abs(S).max()), K * EPS[dt] * M
    print(f"dt={dt} qd={qd}: max|S| = {defect:.3g}, bound = {bound:.3g}")
    assert np.isfinite(S).all() and defect <= bound, (defect, bound)
