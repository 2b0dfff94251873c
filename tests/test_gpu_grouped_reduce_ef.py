"""The fused grouped reduce + quantize with error feedback (piquant_hip_reduce_quantize_grouped_ef / piquant.torch.reduce_quantize_grouped_ef) on
the MI355X.

The call is specified as a composition of two calls that other files pin against the CPU models: grouped dequantize ADD of every term into acc,
in order, then quantize_grouped_ef(acc, residual).  Packed bytes, scales, zero points and the residual are compared bit for bit (NaN equals NaN
in the residual) with that composition run on the device in the same process and, for a subset, with the CPU model
(tests/grouped_reduce_ef_sim.py: reduce_ef_step), which shares no code with the device composition.  Every written buffer has guard bytes in front
of it and behind it."""
import numpy as np
import pytest

import oracle as O
from grouped_reduce_ef_sim import reduce_ef_step

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
# 70 001: several blocks even for the largest chunk (8 192 elements), a ragged last chunk and a partial last group; 65 536 ends on a chunk
NUMELS = [1, 31, 129, 65_536, 70_001]


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


def _rand(n, fdt, seed, scale=1.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(n, device="cuda", generator=g) * scale
    if n > 16:   # per-group magnitudes that differ, and an outlier or two
        x *= torch.linspace(0.01, 30.0, n, device="cuda")[torch.randperm(n, device="cuda", generator=g)]
        x[torch.randint(0, n, (max(1, n // 4000),), device="cuda", generator=g)] *= 200.0
    return x.to(fdt)


def _terms(n, fdt, qdtype, G, k, seed, special_scales=False):
    """k packed terms of n elements (raw uint8 bytes) with their per-group parameters, made by quantize_grouped of random tensors."""
    import piquant.torch as pt

    out = []
    for i in range(k):
        q, s, z = pt.quantize_grouped(_rand(n, fdt, seed + i), dtype=qdtype, group_size=G)
        raw = (pt.packed_bytes(q) if q.dtype != torch.uint8 else q.view(-1)).clone()
        if special_scales and s.numel() >= 4:
            s[0], s[1], s[2], s[3] = 0.0, -s[1], float("inf"), float("nan")
            s[-1] = -0.0
        out.append((raw, s, z))
    return out


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _guarded(nbytes, shift=0):
    """(whole buffer, view of nbytes bytes that starts GUARD + shift bytes in); everything is 0xAA"""
    buf = torch.full((GUARD + shift + nbytes + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + shift: GUARD + shift + nbytes]


def _guards_ok(buf, nbytes, shift=0):
    return bool((buf[: GUARD + shift] == 0xAA).all()) and bool((buf[GUARD + shift + nbytes:] == 0xAA).all())


def fused(acc, res, terms, qdtype, G, mode="nearest", stream_ctx=None, shift_out=0, shift_res=0):
    """reduce_quantize_grouped_ef into guarded buffers (acc and the residual are copied first; shift_*: bytes by which out / the residual are
    moved off their 16-byte alignment); -> (bytes, scales, zero points, new residual) on the device, guards in front and behind checked."""
    import piquant.torch as pt

    n, es = acc.numel(), acc.element_size()
    qdt = pt.torch_to_piquant_dtype(qdtype)
    nb, ng = qdt.packed_nbytes(n), -(-n // G)
    obuf, out = _guarded(nb, shift_out)
    sbuf, sc = _guarded(4 * ng)
    zbuf, zp = _guarded(ng)
    rbuf, rraw = _guarded(n * es, shift_res)
    r = rraw.view(acc.dtype)
    r.copy_(res)
    saved = [t[0].clone() for t in terms]
    pt.reduce_quantize_grouped_ef(acc.clone() if acc.data_ptr() % 16 == 0 else acc, r, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms],
                                  dtype=qdtype, group_size=G, round_mode=mode, out=out, out_scales=sc.view(torch.float32), out_zero_points=zp, ctx=stream_ctx)
    torch.cuda.synchronize()
    assert _guards_ok(obuf, nb, shift_out), "wrote outside out"
    assert _guards_ok(sbuf, 4 * ng), "wrote outside scales"
    assert _guards_ok(zbuf, ng), "wrote outside zero_points"
    assert _guards_ok(rbuf, n * es, shift_res), "wrote outside the residual"
    assert all(torch.equal(a, t[0]) for a, t in zip(saved, terms)), "a term was modified"
    return out.clone(), sc.view(torch.float32).clone(), zp.clone(), r.clone()


def composition(acc, res, terms, qdtype, G, mode="nearest"):
    """The specification: grouped dequantize ADD of every term into acc, in order, then quantize_grouped_ef(acc, residual)."""
    import piquant.torch as pt

    a, r = acc.clone(), res.clone()
    n = a.numel()
    for raw, s, z in terms:
        pt.dequantize_grouped(raw, s, z, dtype=a.dtype, group_size=G, reduce_op="add", out=a, quant_dtype=qdtype, shape=(n,))
    q, s, z = pt.quantize_grouped_ef(a, r, dtype=qdtype, group_size=G, round_mode=mode)
    torch.cuda.synchronize()
    return (pt.packed_bytes(q) if q.dtype != torch.uint8 else q.view(-1)), s, z, r


def _same(got, want, what=""):
    (q, s, z, r), (wq, ws, wz, wr) = got, want
    assert torch.equal(s.view(torch.int32), ws.view(torch.int32)), f"{what}: scales differ at groups {torch.nonzero(s.view(torch.int32) != ws.view(torch.int32)).flatten()[:8].tolist()}"
    assert torch.equal(z, wz), f"{what}: zero points differ at groups {torch.nonzero(z != wz).flatten()[:8].tolist()}"
    bad = torch.nonzero(q != wq).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} bytes differ, first at {bad[:8].tolist()}"
    gn, wn = torch.isnan(r), torch.isnan(wr)
    assert torch.equal(gn, wn), f"{what}: NaN positions of the residual differ at {torch.nonzero(gn != wn).flatten()[:8].tolist()}"
    bad = torch.nonzero((_bits(r) != _bits(wr)) & ~wn).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} residual elements differ, first at {bad[:8].tolist()}: got {r[bad[:4]].tolist()} want {wr[bad[:4]].tolist()}"


def _pair(n, fdt, seed):
    return _rand(n, fdt, seed), _rand(n, fdt, seed + 500, scale=0.02)


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_fused_equals_the_two_call_composition(ctx, dt, qd, G):
    ctx.set_stochastic_threshold(None)
    for k in (0, 1, 3):
        for i, n in enumerate(NUMELS):
            seed = 1000 * k + 10 * i + G + qd
            acc, res = _pair(n, FDT[dt], seed)
            terms = _terms(n, FDT[dt], QDT[qd], G, k, seed + 1)
            _same(fused(acc, res, terms, QDT[qd], G), composition(acc, res, terms, QDT[qd], G), f"k={k} n={n}")


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4)])
def test_stochastic_pinned_threshold_and_per_element(ctx, dt, qd):
    """ONE threshold per call (pinned, so that both forms draw the same), and the per-element mode, which indexes the global element."""
    try:
        for G, k, n in ((32, 1, 70_001), (128, 3, 70_001), (4096, 1, 65_536), (128, 0, 129)):
            acc, res = _pair(n, FDT[dt], 3 + k + G)
            terms = _terms(n, FDT[dt], QDT[qd], G, k, 90 + k)
            for tau in (0.0, 0.37, 0.999):
                ctx.set_stochastic_threshold(tau)
                _same(fused(acc, res, terms, QDT[qd], G, "stochastic"), composition(acc, res, terms, QDT[qd], G, "stochastic"), f"tau={tau} G={G} k={k}")
            ctx.set_stochastic_threshold(None)
            ctx.set_stochastic_per_element(True, seed=0x1234_5678_9ABC, index_base=7)
            got = fused(acc, res, terms, QDT[qd], G, "stochastic")
            _same(got, composition(acc, res, terms, QDT[qd], G, "stochastic"), f"per element G={G} k={k}")
            if n > 1000:
                nearest = fused(acc, res, terms, QDT[qd], G, "nearest")
                assert not torch.equal(got[0], nearest[0]), "per-element stochastic rounding changed nothing"
            ctx.set_stochastic_per_element(False)
    finally:
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(False)


def test_term_limits(ctx):
    """16 terms are one launch; with 17 the first goes into acc by a grouped dequantize ADD launch and the last 16 are fused."""
    ctx.set_stochastic_threshold(None)
    n, G = 70_001, 128
    for k in (16, 17):
        acc, res = _pair(n, torch.float32, 40 + k)
        terms = _terms(n, torch.float32, torch.quint4x2, G, k, 300 + k)
        _same(fused(acc, res, terms, torch.quint4x2, G), composition(acc, res, terms, torch.quint4x2, G), f"k={k}")


def _host(t, dt):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if dt == O.BF16 else t.cpu().numpy()


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4)])
def test_fused_equals_the_cpu_model(ctx, dt, qd):
    """Against tests/grouped_reduce_ef_sim.py directly: the second, independent reference."""
    G = 128
    ctx.set_stochastic_threshold(None)
    for k, n in ((0, 129), (1, 10 * G + 7), (3, 70_001)):
        acc, res = _pair(n, FDT[dt], 77 + k)
        terms = _terms(n, FDT[dt], QDT[qd], G, k, 500 + k)
        host_terms = [(raw.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()) for raw, s, z in terms]
        wq, ws, wz, wr, _, _ = reduce_ef_step(_host(acc, dt), _host(res, dt), host_terms, dt, qd, G)
        q, s, z, r = fused(acc, res, terms, QDT[qd], G)
        assert np.array_equal(s.cpu().numpy().view(np.uint32), ws.view(np.uint32)) and np.array_equal(z.cpu().numpy(), wz), f"k={k} n={n}: parameters"
        assert np.array_equal(q.cpu().numpy(), wq), f"k={k} n={n}: bytes"
        view = np.uint16 if dt == O.BF16 else np.uint32
        assert np.array_equal(_host(r, dt).view(view), wr.view(view)), f"k={k} n={n}: residual"


def _plant_specials(t, G, n):
    """NaNs of both kinds, +-inf, a constant group, a group of nothing but NaNs, denormals"""
    bf = t.dtype == torch.bfloat16
    iv = t.view(torch.int16) if bf else t.view(torch.int32)
    t[3] = float("nan")
    iv[7] = 0x7FA0 if bf else 0x7FA00000                             # a signaling NaN
    iv[9] = -96 if bf else -6291456                                   # 0xFFA0 / 0xFFA00000: a negative signaling NaN
    t[G + 1] = float("inf")
    t[2 * G + 2] = float("-inf")
    t[3 * G: 4 * G] = 7.25
    t[5 * G: 6 * G] = float("nan")
    iv[6 * G + 1] = 1                                                 # the smallest denormal
    iv[6 * G + 2] = 0x7F if bf else 0x7FFFFF                          # the largest
    iv[6 * G + 3] = -32767 if bf else -2147483647                     # -denormal
    t[n - 2] = float("nan")


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4)])
def test_special_values(ctx, dt, qd):
    """Special values in acc, in the residual (at other places: both meet ordinary values and each other), and terms whose scales are 0,
    negative, -0, inf or NaN."""
    ctx.set_stochastic_threshold(None)
    for G in (32, 128):
        n = 64 * G + 5
        acc, res = _pair(n, FDT[dt], 9 + G)
        _plant_specials(acc, G, n)
        shifted = res[G:].clone()
        _plant_specials(shifted, G, n - G)
        res[G:] = shifted
        res[3] = float("inf")                                         # NaN + inf, inf + -inf further on
        res[G + 1] = float("-inf")
        for k in (0, 1, 3):
            terms = _terms(n, FDT[dt], QDT[qd], G, k, 40 + G + k, special_scales=True)
            _same(fused(acc, res, terms, QDT[qd], G), composition(acc, res, terms, QDT[qd], G), f"G={G} k={k}")


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4)])
@pytest.mark.parametrize("which", ["acc", "residual", "out", "term"])
def test_misaligned_buffers_take_the_two_step_form(ctx, dt, qd, which):
    """acc, the residual, out or one term moved off its 16-byte alignment by one element (one byte for the packed buffers): the same bytes through
    the composition, and nothing written in front of or behind any written buffer."""
    G, n, k = 128, 70_001, 3
    ctx.set_stochastic_threshold(None)
    fdt = FDT[dt]
    base, res = _pair(n + 8, fdt, 5)
    acc = base[1: 1 + n] if which == "acc" else base[:n].clone()
    res = res[:n].clone()
    terms = _terms(n, fdt, QDT[qd], G, k, 6)
    if which == "term":
        raw = torch.empty(terms[1][0].numel() + 1, dtype=torch.uint8, device="cuda")[1:]
        raw.copy_(terms[1][0])
        terms[1] = (raw, terms[1][1], terms[1][2])
    want = composition(acc, res, terms, QDT[qd], G)
    if which == "acc":
        assert acc.data_ptr() % 16 != 0
        before = base.clone()
    got = fused(acc, res, terms, QDT[qd], G, shift_out=1 if which == "out" else 0, shift_res=acc.element_size() if which == "residual" else 0)
    _same(got, want, which)
    if which == "acc":   # acc itself is unspecified afterwards; its neighbours are not
        assert torch.equal(_bits(base[:1]), _bits(before[:1])) and torch.equal(_bits(base[1 + n:]), _bits(before[1 + n:])), "wrote outside acc"


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT2), (O.BF16, O.UINT8)])
def test_no_terms_is_quantize_grouped_ef(ctx, dt, qd):
    import piquant.torch as pt

    ctx.set_stochastic_threshold(None)
    for G, n in ((32, 70_001), (4096, 65_536), (128, 1)):
        acc, res = _pair(n, FDT[dt], 60 + G)
        r = res.clone()
        q, s, z = pt.quantize_grouped_ef(acc, r, dtype=QDT[qd], group_size=G)
        torch.cuda.synchronize()
        _same(fused(acc, res, [], QDT[qd], G), ((pt.packed_bytes(q) if q.dtype != torch.uint8 else q.view(-1)), s, z, r), f"G={G} n={n}")


def test_non_default_stream(ctx):
    import piquant

    G, n = 128, 70_001
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        acc = torch.empty(n, device="cuda")
        acc.normal_()
        acc.mul_(3.0).add_(1.0)   # still in flight when the fused call is enqueued behind it on the same stream
        res = torch.zeros(n, device="cuda")
        res.add_(0.01)
        terms = _terms(n, torch.float32, torch.uint8, G, 3, 11)
        got = fused(acc, res, terms, torch.uint8, G, stream_ctx=piquant.Context.get(0))
        want = composition(acc, res, terms, torch.uint8, G)
    side.synchronize()
    _same(got, want)


def test_graph_capture_and_three_replays(ctx):
    """One step captured once -- a copy that restores acc (it is unspecified after a call), then the fused call -- and replayed three times with the
    residual carried from replay to replay: the bytes, parameters and the residual of three eager steps."""
    import piquant.torch as pt

    G, n, qdt = 128, 70_001, torch.quint4x2
    ctx.set_stochastic_threshold(None)
    acc0, _ = _pair(n, torch.float32, 21)
    terms = _terms(n, torch.float32, qdt, G, 3, 22)
    args = ([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms])
    res = torch.zeros(n, device="cuda")
    eager = []
    for _ in range(3):
        q, s, z = pt.reduce_quantize_grouped_ef(acc0.clone(), res, *args, dtype=qdt, group_size=G)
        eager.append((pt.packed_bytes(q).clone(), s.clone(), z.clone(), res.clone()))
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0]), "the residual changed nothing from step to step"

    res.zero_()
    acc = torch.empty_like(acc0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.copy_(acc0)
        gq, gs, gz = pt.reduce_quantize_grouped_ef(acc, res, *args, dtype=qdt, group_size=G)
    res.zero_()
    for t in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _same((pt.packed_bytes(gq), gs, gz, res), eager[t], f"replay {t}")
