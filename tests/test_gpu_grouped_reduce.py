"""The fused grouped reduce + quantize (piquant_hip_reduce_quantize_grouped / piquant.torch.reduce_quantize_grouped) and the batched grouped
quantize / dequantize on the MI355X.

The fused call is specified as a composition of calls that tests/test_gpu_grouped.py pins against the CPU group model: grouped dequantize ADD
of every term into acc, in order, then quantize_grouped(acc).  Its bytes, scales and zero points are compared bit for bit with that two-step
form run on the device in the same process, and with the CPU model itself on smaller inputs.  The batches are compared with single calls."""
import numpy as np
import pytest

import oracle as O
from grouped_model import dequantize_grouped, group_params_all, quantize_grouped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)


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


def _bytes(q):
    import piquant.torch as pt

    return (pt.packed_bytes(q) if q.dtype != torch.uint8 else q.view(-1)).cpu().numpy()


def fused(acc, terms, qdtype, G, mode="nearest", stream_ctx=None):
    """reduce_quantize_grouped into guarded buffers; -> (bytes, scales, zero points) on the host, guards checked."""
    import piquant
    import piquant.torch as pt

    n = acc.numel()
    qdt = piquant.torch.torch_to_piquant_dtype(qdtype)
    nb, ng = qdt.packed_nbytes(n), -(-n // G)
    out = torch.full((nb + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    sc = torch.full((4 * ng + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    zp = torch.full((ng + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    saved = [t[0].clone() for t in terms]
    pt.reduce_quantize_grouped(acc.clone(), [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=qdtype, group_size=G,
                               round_mode=mode, out=out[:nb], out_scales=sc[: 4 * ng].view(torch.float32), out_zero_points=zp[:ng], ctx=stream_ctx)
    torch.cuda.synchronize()
    assert bool((out[nb:] == 0xAA).all()), "wrote past the end of out"
    assert bool((sc[4 * ng:] == 0xAA).all()), "wrote past the end of scales"
    assert bool((zp[ng:] == 0xAA).all()), "wrote past the end of zero_points"
    assert all(torch.equal(a, t[0]) for a, t in zip(saved, terms)), "a term was modified"
    return out[:nb].cpu().numpy(), sc[: 4 * ng].cpu().numpy().view(np.float32), zp[:ng].cpu().numpy()


def two_step(acc, terms, qdtype, G, mode="nearest"):
    """The specification: grouped dequantize ADD of every term into acc, in order, then quantize_grouped(acc)."""
    import piquant.torch as pt

    a = acc.clone()
    n = a.numel()
    for raw, s, z in terms:
        pt.dequantize_grouped(raw, s, z, dtype=a.dtype, group_size=G, reduce_op="add", out=a, quant_dtype=qdtype, shape=(n,))
    q, s, z = pt.quantize_grouped(a, dtype=qdtype, group_size=G, round_mode=mode)
    torch.cuda.synchronize()
    return _bytes(q), s.cpu().numpy(), z.cpu().numpy()


def _same(got, want, what=""):
    (q, s, z), (wq, ws, wz) = got, want
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), f"{what}: scales differ at groups {np.flatnonzero(s.view(np.uint32) != ws.view(np.uint32))[:8]}"
    assert np.array_equal(z, wz), f"{what}: zero points differ at groups {np.flatnonzero(z != wz)[:8]}"
    bad = np.flatnonzero(q != wq)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:8]}"


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_fused_equals_two_step(ctx, dt, qd, G):
    ctx.set_stochastic_threshold(None)
    for k in (0, 1, 7, 16, 17):
        for i, n in enumerate([1, G - 1, G + 1, 10 * G + 7, 200_003]):
            seed = 1000 * k + 10 * i + G + qd
            acc = _rand(n, FDT[dt], seed)
            terms = _terms(n, FDT[dt], QDT[qd], G, k, seed + 1)
            _same(fused(acc, terms, QDT[qd], G), two_step(acc, terms, QDT[qd], G), f"k={k} n={n}")


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_fused_equals_the_cpu_group_model(ctx, dt, qd):
    """Against tests/grouped_model.py directly: the terms' dequantize ADD group by group through the oracle, then the model's parameters and bytes."""
    G = 128
    ctx.set_stochastic_threshold(None)
    for k in (1, 7):
        n = 10 * G + 7
        acc = _rand(n, FDT[dt], 77 + k)
        terms = _terms(n, FDT[dt], QDT[qd], G, k, 500 + k)
        host = acc.view(torch.int16).cpu().numpy().view(np.uint16) if dt == O.BF16 else acc.cpu().numpy()
        a = host.copy()
        for raw, s, z in terms:
            a = dequantize_grouped(raw.cpu().numpy(), qd, dt, n, G, s.cpu().numpy(), z.cpu().numpy(), O.ADD, prev=a)
        af = O.bf16_to_f32(a) if dt == O.BF16 else a
        ws, wz = group_params_all(af, G, qd)
        wq, _, _ = quantize_grouped(a, dt, qd, G, params=(ws, wz))
        _same(fused(acc, terms, QDT[qd], G), (wq, ws, wz), f"k={k}")


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_special_values(ctx, dt, qd):
    """NaN / +-inf in acc (a group of nothing but NaNs among them), and terms whose given scales are 0, negative, -0, inf or NaN."""
    ctx.set_stochastic_threshold(None)
    for G in (32, 128):
        n = 64 * G + 5
        acc = _rand(n, torch.float32, 9 + G)
        acc[3] = float("nan")
        acc[G + 1] = float("inf")
        acc[2 * G + 2] = float("-inf")
        acc[5 * G: 6 * G] = float("nan")
        acc[n - 2] = float("nan")
        acc = acc.to(FDT[dt])
        for k in (1, 3):
            terms = _terms(n, FDT[dt], QDT[qd], G, k, 40 + G + k, special_scales=True)
            _same(fused(acc, terms, QDT[qd], G), two_step(acc, terms, QDT[qd], G), f"G={G} k={k}")


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_stochastic_with_a_pinned_threshold(ctx, dt, qd):
    for tau in (0.0, 0.37, 0.999):
        ctx.set_stochastic_threshold(tau)
        for G, k in ((32, 1), (128, 7), (4096, 2)):
            n = 30 * G + 3
            acc = _rand(n, FDT[dt], 3 + k)
            terms = _terms(n, FDT[dt], QDT[qd], G, k, 90 + k)
            _same(fused(acc, terms, QDT[qd], G, "stochastic"), two_step(acc, terms, QDT[qd], G, "stochastic"), f"tau={tau} G={G} k={k}")
    ctx.set_stochastic_threshold(None)


def test_misaligned_buffers_take_the_two_step_form(ctx):
    """acc or a term that is not 16-byte aligned: the same bytes through the composition (acc of a slice that starts one element in)."""
    G, n = 128, 50_001
    ctx.set_stochastic_threshold(None)
    for dt, qd in ((O.F32, O.UINT8), (O.BF16, O.UINT4)):
        base = _rand(n + 8, FDT[dt], 5)
        acc = base[1: 1 + n]
        assert acc.data_ptr() % 16 != 0
        terms = _terms(n, FDT[dt], QDT[qd], G, 3, 6)
        raw = torch.empty(terms[1][0].numel() + 1, dtype=torch.uint8, device="cuda")[1:]
        raw.copy_(terms[1][0])
        terms[1] = (raw, terms[1][1], terms[1][2])
        _same(fused(acc, terms, QDT[qd], G), two_step(acc, terms, QDT[qd], G))


def test_non_default_stream(ctx):
    import piquant

    G, n = 128, 1 << 22
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        acc = torch.empty(n, device="cuda")
        acc.normal_()
        acc.mul_(3.0).add_(1.0)   # still in flight when the fused call is enqueued behind it on the same stream
        terms = _terms(n, torch.float32, torch.uint8, G, 7, 11)
        got = fused(acc, terms, torch.uint8, G, stream_ctx=piquant.Context.get(0))
        want = two_step(acc, terms, torch.uint8, G)
    side.synchronize()
    _same(got, want)


def test_graph_capture_replay(ctx):
    import piquant.torch as pt

    G, n = 128, 1_000_003
    acc0 = torch.randn(n, device="cuda")
    terms = _terms(n, torch.float32, torch.quint4x2, G, 3, 21)
    xs = [torch.randn(m, device="cuda") for m in (1000, 0, 70_001, 4096)]
    want = two_step(acc0, terms, torch.quint4x2, G)
    acc = acc0.clone()
    out, s, z = pt.reduce_quantize_grouped(acc, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=torch.quint4x2, group_size=G)
    bq, bs, bz = pt.quantize_grouped_batch(xs, dtype=torch.quint4x2, group_size=G)
    bo = pt.dequantize_grouped_batch(bq, bs, bz, dtype=torch.float32, group_size=G)
    torch.cuda.synchronize()
    want_b = [o.clone() for o in bo]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout, gs, gz = pt.reduce_quantize_grouped(acc, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=torch.quint4x2,
                                                  group_size=G)
        gbq, gbs, gbz = pt.quantize_grouped_batch(xs, dtype=torch.quint4x2, group_size=G)
        gbo = pt.dequantize_grouped_batch(gbq, gbs, gbz, dtype=torch.float32, group_size=G)
    for _ in range(3):
        acc.copy_(acc0)
        gs.zero_()
        for o in gbo:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same((_bytes(gout), gs.cpu().numpy(), gz.cpu().numpy()), want)
        assert all(torch.equal(a, b) for a, b in zip(gbo, want_b))


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
def _batch_inputs(count, fdt, seed):
    sizes = [0, 1, 127, 128, 129, 4096, 10_007, 250_001, 33, 8191, 65_536, 3, 0, 99_999, 4095, 1_000_003, 17]
    xs = [_rand(sizes[(i + seed) % len(sizes)], fdt, seed + i) for i in range(count)]
    if count > 3:   # one tensor whose buffer is not 16-byte aligned (the single call's guarded path inside the batch)
        base = _rand(xs[3].numel() + 4, fdt, seed + 99)
        xs[3] = base[1: 1 + xs[3].numel()]
    return xs


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_quantize_batch_equals_single_calls(ctx, dt, qd, G):
    import piquant.torch as pt

    for count in (1, 2, 5, 16, 17):
        xs = _batch_inputs(count, FDT[dt], 7 * count + G)
        for mode, tau in (("nearest", None), ("stochastic", 0.42)):
            ctx.set_stochastic_threshold(tau)
            outs, ss, zs = pt.quantize_grouped_batch(xs, dtype=QDT[qd], group_size=G, round_mode=mode)
            for i, x in enumerate(xs):
                q1, s1, z1 = pt.quantize_grouped(x, dtype=QDT[qd], group_size=G, round_mode=mode)
                _same((_bytes(outs[i]), ss[i].cpu().numpy(), zs[i].cpu().numpy()), (_bytes(q1), s1.cpu().numpy(), z1.cpu().numpy()), f"{count} {mode} #{i}")
            # given parameters: the batch's own, on other data
            ys = [x.flip(0).contiguous() for x in xs]
            gouts, gss, gzs = pt.quantize_grouped_batch(ys, dtype=QDT[qd], group_size=G, round_mode=mode, scales=ss, zero_points=zs)
            assert all(a is b for a, b in zip(gss, ss))
            for i, y in enumerate(ys):
                q1, _, _ = pt.quantize_grouped(y, dtype=QDT[qd], group_size=G, round_mode=mode, scales=ss[i], zero_points=zs[i])
                assert np.array_equal(_bytes(gouts[i]), _bytes(q1)), (count, mode, i)
    ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_dequantize_batch_equals_single_calls(ctx, dt, qd, G):
    import piquant.torch as pt

    for count in (1, 3, 16, 17):
        xs = _batch_inputs(count, FDT[dt], 11 * count + G)
        qs, ss, zs = pt.quantize_grouped_batch(xs, dtype=QDT[qd], group_size=G)
        outs = pt.dequantize_grouped_batch(qs, ss, zs, dtype=FDT[dt], group_size=G)
        for i in range(count):
            one = pt.dequantize_grouped(qs[i], ss[i], zs[i], dtype=FDT[dt], group_size=G)
            assert torch.equal(outs[i].view(-1).view(torch.int16 if dt == O.BF16 else torch.int32),
                               one.view(-1).view(torch.int16 if dt == O.BF16 else torch.int32)), (count, i)
        accs = [_rand(x.numel(), FDT[dt], 5 + i) for i, x in enumerate(xs)]
        want = [a.clone() for a in accs]
        for i in range(count):
            pt.dequantize_grouped(qs[i], ss[i], zs[i], dtype=FDT[dt], group_size=G, reduce_op="add", out=want[i])
        raw = [_bytes(q) for q in qs]
        raw_dev = [torch.from_numpy(r).cuda() for r in raw]
        pt.dequantize_grouped_batch(raw_dev, ss, zs, dtype=FDT[dt], group_size=G, reduce_op="add", outs=accs, quant_dtype=QDT[qd],
                                    shapes=[(x.numel(),) for x in xs])
        for i in range(count):
            assert torch.equal(accs[i].view(torch.int16 if dt == O.BF16 else torch.int32), want[i].view(torch.int16 if dt == O.BF16 else torch.int32)), (count, i)
