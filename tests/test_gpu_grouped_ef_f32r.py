"""Error-feedback group-wise quantization of a bfloat16 tensor with a FLOAT32 residual on the MI355X (piquant_hip_quantize_grouped_ef_mixed,
its batch and the reduce entry): bit-exact against the CPU model (tests/ef_f32r_model.py) and against the device composition
quantize_grouped_ef(x.float(), residual) that defines it, canaries around every buffer, misaligned buffers, batches, the reduce entry, graph
capture, and the conservation identity at float32 precision."""
import numpy as np
import pytest

import oracle as O
from ef_model import EPS, widen
from grouped_model import dequantize_grouped, group_params_all, quantize_grouped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QDS = [O.UINT8, O.UINT4, O.UINT2]
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
GROUP_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
GUARD = 64


def chunk_elems(qd, G):
    """NG * G of the float32 tile (csrc/grouped_kernels.hpp, GroupedQuantTile<DT_F32, BITS, G>): what one wave quantizes"""
    ob = 4 * BITS[qd] // 8
    v = G // 4
    rpg = 1 if v < 64 else v // 64
    nv_want = max(16 // ob, 4)
    return max(rpg, min(v, nv_want)) * 64 * 4


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


def _dev(a: np.ndarray):
    """numpy array -> device uint8 buffer with GUARD bytes of 0xAA in front of and behind the data; -> (buffer, view of the data)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((raw.size + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    if raw.size:
        buf[GUARD: GUARD + raw.size].copy_(torch.from_numpy(raw.copy()))
    return buf, buf[GUARD: GUARD + raw.size]


def _guard_ok(buf, n):
    return bool((buf[:GUARD] == 0xAA).all()) and bool((buf[GUARD + n:] == 0xAA).all())


def make_input(n, seed):
    """bfloat16 data (as bits) with a varying magnitude and a few planted outliers, and a float32 residual of about a percent of it"""
    rng = np.random.default_rng(seed)
    mag = np.repeat(rng.uniform(0.01, 50.0, n // 97 + 1), 97)[:n]
    xf = (rng.standard_normal(n) * mag).astype(np.float32)
    if n > 10:
        xf[rng.choice(n, max(1, n // 5000), replace=False)] *= 100.0
    rf = (rng.standard_normal(n) * mag * 0.01).astype(np.float32)
    return O.f32_to_bf16(xf), rf


def gpu_mixed(ctx, x, r, qd, G, mode=O.NEAREST):
    """One mixed call on guarded buffers, and the composition quantize_grouped_ef(x.float(), r.clone()) beside it on the device (same pinned
    threshold).  -> ((packed bytes, scales, zero points, new residual) on the host, the composition's four as device tensors)"""
    import piquant
    import piquant.torch as pt

    n = x.size
    ng = (n + G - 1) // G
    nbytes = O.packed_numel(n, qd)
    xbuf, xin = _dev(x)
    rbuf, rin = _dev(r)
    obuf, oin = _dev(np.full(nbytes, 0xAA, dtype=np.uint8))
    sbuf, sin = _dev(np.zeros(ng, dtype=np.float32))
    zbuf, zin = _dev(np.zeros(ng, dtype=np.uint8))
    assert xin.data_ptr() % 16 == 0 and rin.data_ptr() % 16 == 0 and oin.data_ptr() % 16 == 0
    xt = xin.view(torch.bfloat16)
    cr = rin.view(torch.float32).clone()
    cq, cs, cz = pt.quantize_grouped_ef(xt.float(), cr, dtype=QDT[qd], group_size=G, round_mode="nearest" if mode == O.NEAREST else "stochastic")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_ef_ptr(xin.data_ptr(), piquant.DataType.BF16, rin.data_ptr(), oin.data_ptr(), piquant.DataType(qd), n, G, sin.data_ptr(),
                                zin.data_ptr(), piquant.RoundMode(mode), _device_ptrs=True, residual_dtype=piquant.DataType.F32)
    torch.cuda.synchronize()
    assert _guard_ok(obuf, nbytes), "wrote outside out"
    assert _guard_ok(sbuf, 4 * ng), "wrote outside scales"
    assert _guard_ok(zbuf, ng), "wrote outside zero_points"
    assert _guard_ok(rbuf, 4 * n), "wrote outside the residual"
    assert _guard_ok(xbuf, 2 * n) and np.array_equal(xin.cpu().numpy(), x.view(np.uint8).reshape(-1)), "the input was written"
    got = (oin.cpu().numpy(), sin.cpu().numpy().view(np.float32), zin.cpu().numpy(), rin.cpu().numpy().view(np.float32))
    return got, (pt.packed_bytes(cq).cpu().numpy(), cs.cpu().numpy(), cz.cpu().numpy(), cr.cpu().numpy())


def assert_residual_equal(got, want, what=""):
    """bit for bit, NaNs by position"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8]}"
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} residual elements differ, first at {bad[:8]}: got {got[bad[:4]]} want {want[bad[:4]]}"


class Model:
    """tests/ef_f32r_model.py for several rounding modes: y = rn_f32(widen(x) + r) and the parameters are computed once"""

    def __init__(self, x, r, qd, G):
        self.qd, self.G = qd, G
        with np.errstate(invalid="ignore", over="ignore"):
            self.y = widen(x, O.BF16) + r
        self.s, self.z = group_params_all(self.y, G, qd)

    def step(self, mode=O.NEAREST, tau=0.0):
        q, _, _ = quantize_grouped(self.y, O.F32, self.qd, self.G, mode, tau, params=(self.s, self.z))
        d = dequantize_grouped(q, self.qd, O.F32, self.y.size, self.G, self.s, self.z)
        with np.errstate(invalid="ignore", over="ignore"):
            return q, self.y - d


def check(ctx, x, r, qd, G, model, mode=O.NEAREST, tau=0.0):
    (q, s, z, rn), (cq, cs, cz, cr) = gpu_mixed(ctx, x, r, qd, G, mode)
    what = f"n={x.size} G={G} qd={qd} mode={mode} tau={tau}"
    wq, wr = model.step(mode, tau)
    for name, wq_, ws_, wz_, wr_ in (("model", wq, model.s, model.z, wr), ("composition", cq, cs, cz, cr)):
        assert np.array_equal(s.view(np.uint32), ws_.view(np.uint32)), f"{what} vs {name}: scales differ at groups {np.flatnonzero(s.view(np.uint32) != ws_.view(np.uint32))[:8]}"
        assert np.array_equal(z, wz_), f"{what} vs {name}: zero points differ at groups {np.flatnonzero(z != wz_)[:8]}"
        bad = np.flatnonzero(q != wq_)
        assert bad.size == 0, f"{what} vs {name}: {bad.size} bytes differ, first at byte {bad[:8]}"
        assert_residual_equal(rn, wr_, f"{what} vs {name}")


def _model_is_the_committed_one(x, r, qd, G, model):
    """the in-test Model (split so that y and the parameters are shared between modes) is ef_f32r_step"""
    from ef_f32r_model import ef_f32r_step

    q, s, z, rn, _, _ = ef_f32r_step(x, r, qd, G)
    wq, wr = model.step()
    assert np.array_equal(q, wq) and np.array_equal(s, model.s) and np.array_equal(z, model.z)
    assert_residual_equal(rn, wr, "Model vs ef_f32r_step")


@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_parity_nearest_and_stochastic(ctx, qd, G):
    chunk = chunk_elems(qd, G)
    for i, n in enumerate([1, 31, G - 1, G, G + 1, 10 * G + 7, chunk - 1, chunk + 1, 200_003]):
        x, r = make_input(n, seed=3000 * G + 10 * i + qd)
        if n == 10 * G + 7:   # NaNs in x and in r: they stay NaNs in the residual, and they are compared by position
            x, r = x.copy(), r.copy()
            x[[3, G + 1, n - 1]] = np.uint16(0x7FC0)
            r[[5, 2 * G + 2, n - 2]] = np.float32(np.nan)
        model = Model(x, r, qd, G)
        if n == G + 1:
            _model_is_the_committed_one(x, r, qd, G, model)
        ctx.set_stochastic_threshold(None)
        check(ctx, x, r, qd, G, model, O.NEAREST)
        for tau in (0.0, 0.37, 0.999):
            ctx.set_stochastic_threshold(tau)
            check(ctx, x, r, qd, G, model, O.STOCHASTIC, tau)
    ctx.set_stochastic_threshold(None)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _device_pair(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = (torch.randn(n, device="cuda", generator=g) * torch.linspace(0.05, 20.0, n, device="cuda")).to(torch.bfloat16)
    r = torch.randn(n, device="cuda", generator=g) * 0.05
    return x, r


def _composition(x, r, qdt, G, mode="nearest"):
    """the definition: the float32 call on the widened tensor -> (packed bytes, scales, zero points, new residual); r is not modified"""
    import piquant.torch as pt

    rr = r.clone()
    q, s, z = pt.quantize_grouped_ef(x.float(), rr, dtype=qdt, group_size=G, round_mode=mode)
    return pt.packed_bytes(q), s, z, rr


@pytest.mark.parametrize("qd", QDS)
def test_per_element_stochastic_mode_indexes_the_global_element(ctx, qd):
    """per-element thresholds: the mixed call and the composition draw the same threshold for the same element, streaming and guarded"""
    import piquant.torch as pt

    G = 128
    try:
        for n, shift in ((200_003, 0), (10 * G + 7, 1)):
            x, r = _device_pair(n + 1, 11 + qd)
            x, r = x[shift: shift + n], r[:n].clone()
            ctx.set_stochastic_per_element(True, seed=0x1234_5678_9ABC, index_base=77)
            wq, ws, wz, wr = _composition(x, r, QDT[qd], G, "stochastic")
            ctx.set_stochastic_per_element(True, seed=0x1234_5678_9ABC, index_base=77)
            q, s, z = pt.quantize_grouped_ef(x, r, dtype=QDT[qd], group_size=G, round_mode="stochastic")
            torch.cuda.synchronize()
            assert torch.equal(pt.packed_bytes(q), wq) and torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz), (n, shift)
            assert torch.equal(_bits(r), _bits(wr)), (n, shift)
    finally:
        ctx.set_stochastic_per_element(False)


def _shifted_call(ctx, qd, sx, sr, so):
    """One mixed call with x, the residual and out shifted by sx, sr and so bytes off a 16-byte boundary: the bytes of the composition, canaries
    around every buffer intact, x not written."""
    import piquant

    n, G = 100_003, 128
    x, r = _device_pair(n, 6)
    wq, ws, wz, wr = _composition(x, r, QDT[qd], G)
    ng = (n + G - 1) // G
    nbytes = O.packed_numel(n, qd)
    xbuf = torch.full((2 * n + sx + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((4 * n + sr + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    obuf = torch.full((nbytes + so + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    xin, rin, out = xbuf[GUARD + sx: GUARD + sx + 2 * n], rbuf[GUARD + sr: GUARD + sr + 4 * n], obuf[GUARD + so: GUARD + so + nbytes]
    xin.copy_(x.view(torch.uint8))
    rin.copy_(r.view(torch.uint8))
    assert (xin.data_ptr() % 16, rin.data_ptr() % 16, out.data_ptr() % 16) == (sx, sr, so)
    s = torch.empty(ng, dtype=torch.float32, device="cuda")
    z = torch.empty(ng, dtype=torch.uint8, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_ef_ptr(xin.data_ptr(), piquant.DataType.BF16, rin.data_ptr(), out.data_ptr(), piquant.DataType(qd), n, G, s.data_ptr(), z.data_ptr(),
                                piquant.RoundMode.NEAREST, _device_ptrs=True, residual_dtype=piquant.DataType.F32)
    torch.cuda.synchronize()
    assert torch.equal(out, wq) and torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz)
    assert torch.equal(rin, wr.view(torch.uint8)), "residual"
    assert torch.equal(xin, x.view(torch.uint8)), "the input was written"
    for buf, lo, size in ((xbuf, GUARD + sx, 2 * n), (rbuf, GUARD + sr, 4 * n), (obuf, GUARD + so, nbytes)):
        assert bool((buf[:lo] == 0xAA).all()) and bool((buf[lo + size:] == 0xAA).all()), "a canary was overwritten"


@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("which", ["x", "residual", "out"])
def test_misaligned_buffers_take_the_guarded_path(ctx, qd, which):
    """x shifted by one bfloat16 element, the residual by one float, out by one byte: the bytes of the composition, canaries intact."""
    _shifted_call(ctx, qd, 2 if which == "x" else 0, 4 if which == "residual" else 0, 1 if which == "out" else 0)


@pytest.mark.parametrize("qd", QDS)
def test_x_aligned_to_8_bytes_but_not_16_streams(ctx, qd):
    """x shifted by four bfloat16 elements sits at address % 16 == 8: still the streaming kernel, whose rows of x are 8-byte loads -- the one
    alignment this kernel family adds.  Single call with canaries, and the same pair among aligned ones in a batch (the batch kernel)."""
    import piquant.torch as pt

    _shifted_call(ctx, qd, 8, 0, 0)
    G, sizes = 128, [30_011, 20_005, 9]
    pairs = [_device_pair(n + 4, 50 + i) for i, n in enumerate(sizes)]
    xs = [p[0][4:] if i == 1 else p[0][:n].clone() for i, (p, n) in enumerate(zip(pairs, sizes))]
    rs = [p[1][:n].clone() for p, n in zip(pairs, sizes)]
    assert xs[1].data_ptr() % 16 == 8
    want = [_composition(x, r, QDT[qd], G) for x, r in zip(xs, rs)]
    outs, ss, zs = pt.quantize_grouped_ef_batch(xs, rs, dtype=QDT[qd], group_size=G)
    torch.cuda.synchronize()
    for i, (wq, ws, wz, wr) in enumerate(want):
        assert torch.equal(pt.packed_bytes(outs[i]), wq) and torch.equal(ss[i].view(torch.int32), ws.view(torch.int32)) and torch.equal(zs[i], wz), i
        assert torch.equal(_bits(rs[i]), _bits(wr)), i


def test_batch_equals_the_single_calls(ctx):
    """17 pairs -- an empty one and a misaligned one among them --: pair by pair the bytes, parameters and residuals of the single call."""
    import piquant.torch as pt

    G = 128
    sizes = [20_000 + 1237 * i for i in range(17)]
    sizes[4] = 0
    sizes[9] = 5
    for qdt in (torch.quint4x2, torch.uint8, torch.quint2x4):
        pairs = [_device_pair(n + 1, 40 + i) for i, n in enumerate(sizes)]
        xs = [p[0][1:] if i == 7 else p[0][:n].clone() for i, (p, n) in enumerate(zip(pairs, sizes))]   # pair 7: misaligned input
        rs = [p[1][:n].clone() for p, n in zip(pairs, sizes)]
        assert xs[7].data_ptr() % 8 != 0
        singles = []
        for x, r in zip(xs, rs):
            rr = r.clone()
            q, s, z = pt.quantize_grouped_ef(x, rr, dtype=qdt, group_size=G)
            singles.append((pt.packed_bytes(q), s, z, rr))
        outs, ss, zs = pt.quantize_grouped_ef_batch(xs, rs, dtype=qdt, group_size=G)
        torch.cuda.synchronize()
        for i, (wq, ws, wz, wr) in enumerate(singles):
            assert torch.equal(pt.packed_bytes(outs[i]), wq) and torch.equal(ss[i].view(torch.int32), ws.view(torch.int32)) and torch.equal(zs[i], wz), i
            assert rs[i].dtype == torch.float32 and torch.equal(_bits(rs[i]), _bits(wr)), i
        wq, ws, wz, wr = _composition(xs[3], pairs[3][1][:sizes[3]].clone(), qdt, G)
        assert torch.equal(pt.packed_bytes(outs[3]), wq) and torch.equal(_bits(rs[3]), _bits(wr))


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("qd", QDS)
def test_reduce_equals_the_add_calls_followed_by_the_mixed_call(ctx, qd, k):
    import piquant.torch as pt

    n, G, qdt = 50_007, 128, QDT[qd]
    acc, r = _device_pair(n, 20 + k)
    terms = [pt.quantize_grouped(_device_pair(n, 30 + i)[0], dtype=qdt, group_size=G) for i in range(k)]
    want_acc, want_r = acc.clone(), r.clone()
    for q, s, z in terms:
        pt.dequantize_grouped(q, s, z, dtype=torch.bfloat16, group_size=G, reduce_op="add", out=want_acc)
    wq, ws, wz = pt.quantize_grouped_ef(want_acc, want_r, dtype=qdt, group_size=G)
    q, s, z = pt.reduce_quantize_grouped_ef(acc, r, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=qdt, group_size=G)
    torch.cuda.synchronize()
    assert torch.equal(pt.packed_bytes(q), pt.packed_bytes(wq)) and torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(z, wz)
    assert r.dtype == torch.float32 and torch.equal(_bits(r), _bits(want_r))
    cq, cs, cz, cr = _composition(want_acc, _device_pair(n, 20 + k)[1], qdt, G)
    assert torch.equal(pt.packed_bytes(q), cq) and torch.equal(_bits(r), _bits(cr))


def test_graph_capture_and_replay(ctx):
    """A 3-step chain (nearest) captured once and replayed twice gives the bytes and the residual of 6 eager steps."""
    import piquant.torch as pt

    n, G, qdt = 200_003, 128, torch.quint4x2
    xs = [_device_pair(n, 70 + i)[0] for i in range(3)]
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


@pytest.mark.parametrize("qd", QDS)
def test_conservation_on_the_device(ctx, qd):
    """K = 16 chained steps on the device, finite inputs: S = sum_t d_t + r_K - sum_t widen(x_t) in float64 on the host, with
    d_t = dequantize_grouped(q_t, dtype=float32), stays within K 2^-23 M: two float32 roundings per step (y = rn(x + r), r = rn(y - d)) of at most
    half an ulp each, M the largest |y| or |d| seen -- the bound tests/ef_model.py uses for float32.  The same chain with the existing bfloat16
    residual is run beside it and its defect printed (DESIGN.md 4c records it); nothing is asserted about that one."""
    import piquant.torch as pt

    n, G, K = 200_003, 128, 16
    fixed = _device_pair(n, 90)[0]
    fixed[G: 2 * G] = 7.25                                           # one constant group, far from zero
    res = torch.zeros(n, dtype=torch.float32, device="cuda")
    res16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    S, S16 = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    M = M16 = 0.0
    for t in range(K):
        x = fixed if t % 2 == 0 else _device_pair(n, 100 + t)[0]
        xd = x.double().cpu().numpy()
        y = torch.add(x.float(), res)
        q, s, z = pt.quantize_grouped_ef(x, res, dtype=QDT[qd], group_size=G)
        d = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=G)
        S += d.double().cpu().numpy() - xd
        M = max(M, float(y.abs().max()), float(d.abs().max()))
        y16 = torch.add(x, res16)
        q, s, z = pt.quantize_grouped_ef(x, res16, dtype=QDT[qd], group_size=G)
        d16 = pt.dequantize_grouped(q, s, z, dtype=torch.bfloat16, group_size=G)
        S16 += d16.double().cpu().numpy() - xd
        M16 = max(M16, float(y16.float().abs().max()), float(d16.float().abs().max()))
    S += res.double().cpu().numpy()
    S16 += res16.double().cpu().numpy()
    defect, bound = float(np.abs(S).max()), K * EPS[O.F32] * M
    defect16, bound16 = float(np.abs(S16).max()), K * EPS[O.BF16] * M16
    print(f"qd={qd}: float32 residual max|S| = {defect:.3g} (bound {bound:.3g}); bfloat16 residual max|S| = {defect16:.3g} (its bound {bound16:.3g})")
    assert np.isfinite(S).all() and defect <= bound, (defect, bound)
