"""Group-wise quantization on the MI355X (piquant_hip_quantize_grouped / _dequantize_grouped and the piquant.torch wrappers): bit-exact
against the CPU group model (tests/grouped_model.py), against the per-tensor device calls on the same slices, guard bytes, streams and
graph capture."""
import numpy as np
import pytest

import oracle as O
from grouped_model import PACK, dequantize_grouped, group_params_all, groups, quantize_grouped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
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


def make_input(n, dt_in, seed, outliers=True):
    """Normal data with a per-group-ish varying magnitude and a few planted outliers; -> (x in the input dtype, x as float32)."""
    rng = np.random.default_rng(seed)
    xf = (rng.standard_normal(n) * np.repeat(rng.uniform(0.01, 50.0, n // 97 + 1), 97)[:n]).astype(np.float32)
    if outliers and n > 10:
        xf[rng.choice(n, max(1, n // 5000), replace=False)] *= 100.0
    if dt_in == O.BF16:
        xb = O.f32_to_bf16(xf)
        return xb, O.bf16_to_f32(xb)
    return xf, xf


def gpu_quantize_grouped(ctx, x, dt_in, qd, G, mode=O.NEAREST, given=None):
    """-> (packed bytes, scales, zero points) from the device, guard bytes behind out / scales / zero_points checked."""
    import piquant

    n = x.size
    ng = (n + G - 1) // G
    nbytes = O.packed_numel(n, qd)
    xbuf, xin = _dev(x)
    obuf, _ = _dev(np.full(nbytes, 0xAA, dtype=np.uint8))
    if given is None:
        sbuf, _ = _dev(np.zeros(ng, dtype=np.float32))
        zbuf, _ = _dev(np.zeros(ng, dtype=np.uint8))
    else:
        sbuf, _ = _dev(np.asarray(given[0], dtype=np.float32))
        zbuf, _ = _dev(np.asarray(given[1], dtype=np.uint8))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_ptr(xin.data_ptr() if n else 0, piquant.DataType(dt_in), obuf.data_ptr(), piquant.DataType(qd), n, G, sbuf.data_ptr(),
                             zbuf.data_ptr(), given is not None, piquant.RoundMode(mode), _device_ptrs=True)
    torch.cuda.synchronize()
    assert _guard_ok(obuf, nbytes), "wrote past the end of out"
    assert _guard_ok(sbuf, 4 * ng), "wrote past the end of scales"
    assert _guard_ok(zbuf, ng), "wrote past the end of zero_points"
    return obuf[:nbytes].cpu().numpy(), sbuf[: 4 * ng].cpu().numpy().view(np.float32), zbuf[:ng].cpu().numpy()


def gpu_dequantize_grouped(ctx, q, qd, dt_out, n, G, scales, zps, op=O.SET, prev=None):
    import piquant

    odt = np.float32 if dt_out == O.F32 else np.uint16
    prev = np.zeros(n, dtype=odt) if prev is None else prev
    qbuf, qin = _dev(q)
    obuf, _ = _dev(prev)
    sbuf, sin = _dev(np.asarray(scales, dtype=np.float32))
    zbuf, zin = _dev(np.asarray(zps, dtype=np.uint8))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.dequantize_grouped_ptr(qin.data_ptr(), piquant.DataType(qd), obuf.data_ptr(), piquant.DataType(dt_out), n, G, sin.data_ptr(), zin.data_ptr(),
                               piquant.ReduceOp(op), _device_ptrs=True)
    torch.cuda.synchronize()
    nb = n * np.dtype(odt).itemsize
    assert _guard_ok(obuf, nb), "wrote past the end of out"
    return obuf[:nb].cpu().numpy().view(odt)


def check_against_model(ctx, x, dt_in, qd, G, mode=O.NEAREST, tau=0.0):
    q, s, z = gpu_quantize_grouped(ctx, x, dt_in, qd, G, mode)
    xf = O.bf16_to_f32(x) if dt_in == O.BF16 else x
    ws, wz = group_params_all(xf, G, qd)
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), f"scales differ at groups {np.flatnonzero(s.view(np.uint32) != ws.view(np.uint32))[:8]}"
    assert np.array_equal(z, wz), f"zero points differ at groups {np.flatnonzero(z != wz)[:8]}"
    want, _, _ = quantize_grouped(x, dt_in, qd, G, mode, tau, params=(ws, wz))
    bad = np.flatnonzero(q != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at byte {bad[:8]} (n={x.size} G={G})"
    return q, s, z


@pytest.mark.parametrize("dt_in,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_parity_nearest_and_stochastic(ctx, dt_in, qd, G):
    for i, n in enumerate([1, 31, G - 1, G, G + 1, 10 * G + 7, 1_000_003]):
        x, _ = make_input(n, dt_in, seed=1000 * G + 10 * i + qd)
        ctx.set_stochastic_threshold(None)
        check_against_model(ctx, x, dt_in, qd, G, O.NEAREST)
        for tau in (0.0, 0.37, 0.999):
            ctx.set_stochastic_threshold(tau)
            check_against_model(ctx, x, dt_in, qd, G, O.STOCHASTIC, tau)
    ctx.set_stochastic_threshold(None)


def _special_f32_bits(G):
    """Groups of special values as uint32 bit patterns (fp32)."""
    rng = np.random.default_rng(5)
    base = rng.uniform(-2, 2, 12 * G).astype(np.float32).view(np.uint32).copy()
    g = lambda k: slice(k * G, (k + 1) * G)  # noqa: E731
    base[g(0)][::3] = 0x7FC00000                                  # quiet NaNs among numbers
    base[g(1)][::5] = 0x7F800001                                  # signaling NaNs
    base[g(1)][7] = 0xFF812345                                    # negative signaling NaN, payload
    base[g(2)][3] = 0x7F800000                                    # +inf
    base[g(3)][4] = 0xFF800000                                    # -inf
    base[g(4)][:] = np.where(np.arange(G) % 2 == 0, 0x00000000, 0x80000000)   # +-0 only
    base[g(5)][:] = np.arange(1, G + 1, dtype=np.uint32)          # positive denormals
    base[g(6)][::2] = 0x80000007                                  # negative denormals among numbers
    base[g(7)][:] = np.float32(3.25).view(np.uint32)              # constant
    base[g(8)][:] = 0x7FC00000                                    # nothing but NaNs
    base[g(9)][:] = np.where(np.arange(G) % 2 == 0, 0x7FA00000, 0xFFC00001)  # nothing but NaNs, signaling and quiet
    base[g(10)][0] = 0x7F800001                                   # a signaling NaN in front of the group's extremes
    base[g(10)][1] = np.float32(-1e30).view(np.uint32)
    base[g(10)][2] = np.float32(1e30).view(np.uint32)
    return base


@pytest.mark.parametrize("dt_in,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 128])
def test_special_inputs_match_per_tensor_device_calls(ctx, dt_in, qd, G):
    """Groups of NaNs (quiet, signaling), +-inf, +-0, denormals, a constant and nothing but NaNs: parameters and bytes equal
    compute_quant_params_device + quantize_uniform on each slice (the promise of the grouped call)."""
    import piquant
    import piquant.torch as pt

    bits = _special_f32_bits(G)
    if dt_in == O.F32:
        x = bits.view(np.float32)
        xt = torch.from_numpy(bits.view(np.int32).copy()).cuda().view(torch.float32)
    else:
        hb = (bits >> 16).astype(np.uint16)   # bf16 patterns by truncation keep the NaN kinds (0x7F80 0001 -> 0x7F80 would be inf: fix below)
        hb[(bits & 0x7FFFFFFF) > 0x7F800000] |= 0x0001   # every NaN stays a NaN (signaling ones stay signaling)
        x = hb
        xt = torch.from_numpy(hb.view(np.int16).copy()).cuda().view(torch.bfloat16)
    q, s, z = gpu_quantize_grouped(ctx, x, dt_in, qd, G)
    tq = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}[qd]
    for g, (b, e) in enumerate(groups(x.size, G)):
        rec = pt.compute_quant_params_device(xt[b:e], dtype=tq)
        ws, wz = pt.params_to_host(rec)
        assert (np.float32(ws).view(np.uint32), wz) == (s[g].view(np.uint32), int(z[g])), f"group {g}"
        out = torch.empty(O.packed_numel(e - b, qd), dtype=torch.uint8, device="cuda")
        ctx.quantize_ptr(xt[b:e].data_ptr(), piquant.DataType(dt_in), out.data_ptr(), piquant.DataType(qd), e - b, ws, wz, piquant.RoundMode.NEAREST,
                         _device_ptrs=True, uniform=True)
        torch.cuda.synchronize()
        assert np.array_equal(q[b // PACK[qd]: e // PACK[qd]], out.cpu().numpy()), f"bytes of group {g}"
    # the documented NaN rule
    assert (float(s[8]), int(z[8])) == (1.0, {O.UINT8: 127, O.UINT4: 7, O.UINT2: 1}[qd])


@pytest.mark.parametrize("dt_in,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4)])
def test_full_size_every_group(ctx, dt_in, qd):
    n, G = 27_264_000, 128
    x, _ = make_input(n, dt_in, seed=27)
    q, s, z = check_against_model(ctx, x, dt_in, qd, G)
    assert s.size == 213_000


@pytest.mark.parametrize("dt_in,qd", PAIRS)
def test_cross_check_per_tensor_device_calls(ctx, dt_in, qd):
    import piquant
    import piquant.torch as pt

    G, n = 128, 1_000_003
    x, _ = make_input(n, dt_in, seed=77 + qd)
    q, s, z = gpu_quantize_grouped(ctx, x, dt_in, qd, G)
    xt = torch.from_numpy(x.view(np.int32 if dt_in == O.F32 else np.int16).copy()).cuda()
    xt = xt.view(torch.float32 if dt_in == O.F32 else torch.bfloat16)
    tq = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}[qd]
    rng = np.random.default_rng(qd)
    ng = s.size
    for g in sorted(set(rng.choice(ng, 300, replace=False).tolist()) | {ng - 1}):
        b, e = g * G, min((g + 1) * G, n)
        ws, wz = pt.params_to_host(pt.compute_quant_params_device(xt[b:e], dtype=tq))
        assert (np.float32(ws).view(np.uint32), wz) == (s[g].view(np.uint32), int(z[g])), f"group {g}"
        out = torch.empty(O.packed_numel(e - b, qd), dtype=torch.uint8, device="cuda")
        ctx.quantize_ptr(xt[b:e].data_ptr(), piquant.DataType(dt_in), out.data_ptr(), piquant.DataType(qd), e - b, ws, wz, piquant.RoundMode.NEAREST,
                         _device_ptrs=True, uniform=True)
        torch.cuda.synchronize()
        assert np.array_equal(q[b // PACK[qd]: (e + PACK[qd] - 1) // PACK[qd]], out.cpu().numpy()), f"bytes of group {g}"


@pytest.mark.parametrize("dt_in,qd", PAIRS)
@pytest.mark.parametrize("G", [32, 4096])
def test_given_parameters(ctx, dt_in, qd, G):
    n = 10 * G + 7
    x, _ = make_input(n, dt_in, seed=3 + qd)
    ng = (n + G - 1) // G
    rng = np.random.default_rng(G)
    scales = rng.uniform(0.001, 2.0, ng).astype(np.float32)
    zps = rng.integers(0, {O.UINT8: 256, O.UINT4: 16, O.UINT2: 4}[qd], ng).astype(np.uint8)
    for mode, tau in ((O.NEAREST, 0.0), (O.STOCHASTIC, 0.37)):
        ctx.set_stochastic_threshold(tau if mode == O.STOCHASTIC else None)
        q, s, z = gpu_quantize_grouped(ctx, x, dt_in, qd, G, mode, given=(scales, zps))
        assert np.array_equal(s, scales) and np.array_equal(z, zps), "given parameters must not be written"
        want, _, _ = quantize_grouped(x, dt_in, qd, G, mode, tau, params=(scales, zps))
        assert np.array_equal(q, want)
    ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("dt_out", [O.F32, O.BF16])
@pytest.mark.parametrize("qd", [O.UINT8, O.UINT4, O.UINT2])
@pytest.mark.parametrize("op", [O.SET, O.ADD])
def test_dequantize(ctx, qd, dt_out, op):
    rng = np.random.default_rng(qd * 10 + dt_out)
    for G in (32, 128, 4096):
        for n in (1, G - 1, 10 * G + 7, 300_001):
            q = rng.integers(0, 256, O.packed_numel(n, qd)).astype(np.uint8)
            if n % PACK[qd]:   # bits past the tensor's end are zero, as every quantize call leaves them
                q[-1] &= (1 << ((n % PACK[qd]) * {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}[qd])) - 1
            ng = (n + G - 1) // G
            scales = rng.uniform(0.001, 3.0, ng).astype(np.float32)
            zps = rng.integers(0, {O.UINT8: 256, O.UINT4: 16, O.UINT2: 4}[qd], ng).astype(np.uint8)
            prev = None
            if op == O.ADD:
                pf = rng.uniform(-5, 5, n).astype(np.float32)
                prev = pf if dt_out == O.F32 else O.f32_to_bf16(pf)
            got = gpu_dequantize_grouped(ctx, q, qd, dt_out, n, G, scales, zps, op, prev)
            want = dequantize_grouped(q, qd, dt_out, n, G, scales, zps, op, prev)
            bad = np.flatnonzero(got.view(np.uint32 if dt_out == O.F32 else np.uint16) != want.view(np.uint32 if dt_out == O.F32 else np.uint16))
            assert bad.size == 0, f"G={G} n={n}: {bad.size} elements differ, first {bad[:8]}"


@pytest.mark.parametrize("dt_in,qd", PAIRS)
def test_round_trip_bound(ctx, dt_in, qd):
    G, n = 128, 100_003
    x, xf = make_input(n, dt_in, seed=11)
    q, s, z = gpu_quantize_grouped(ctx, x, dt_in, qd, G)
    back = gpu_dequantize_grouped(ctx, q, qd, O.F32, n, G, s, z)
    for g, (b, e) in enumerate(groups(n, G)):
        seg = xf[b:e]
        if seg.min() == seg.max():
            continue   # constant groups take the reference's degenerate (1.0, qmax >> 1): DESIGN.md
        err = np.abs(back[b:e].astype(np.float64) - seg.astype(np.float64))
        tol = 0.5 * float(s[g]) * (1 + 1e-5) + 4 * np.spacing(np.abs(seg).max().astype(np.float32))
        assert err.max() <= tol, f"group {g}: {err.max()} > {tol}"


def test_outlier_accuracy_beats_per_tensor(ctx):
    import piquant.torch as pt

    rng = np.random.default_rng(2024)
    n = 1 << 20
    x = rng.standard_normal(n).astype(np.float32)
    x[rng.choice(n, 64, replace=False)] = rng.choice([-1, 1], 64) * 300.0
    xt = torch.from_numpy(x).cuda()
    q, s, z = pt.quantize_grouped(xt, dtype=torch.quint4x2, group_size=128)
    back = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=128)
    err_g = (back - xt).abs().mean().item()
    st, zt = pt.compute_quant_params(xt, dtype=torch.quint4x2)
    qt = pt.quantize(xt, scale=st, zero_point=zt, dtype=torch.quint4x2, uniform=True)
    err_t = (pt.dequantize(qt, scale=st, zero_point=zt, dtype=torch.float32) - xt).abs().mean().item()
    assert err_g * 4 <= err_t, (err_g, err_t)


def test_torch_api_shapes_and_given(ctx):
    import piquant.torch as pt

    x = torch.randn(3, 1000, device="cuda", dtype=torch.bfloat16)
    q, s, z = pt.quantize_grouped(x, dtype=torch.quint4x2, group_size=256)
    assert q.shape == x.shape and q.dtype == torch.quint4x2
    assert s.shape == (12,) and s.dtype == torch.float32 and z.dtype == torch.uint8 and s.device == x.device
    q2, s2, z2 = pt.quantize_grouped(x, dtype=torch.quint4x2, group_size=256, scales=s, zero_points=z)
    assert s2 is s and z2 is z
    assert torch.equal(pt.packed_bytes(q), pt.packed_bytes(q2))
    y = pt.dequantize_grouped(q, s, z, dtype=torch.bfloat16, group_size=256)
    assert y.shape == x.shape and y.dtype == torch.bfloat16
    acc = torch.ones_like(y)
    pt.dequantize_grouped(q, s, z, dtype=torch.bfloat16, group_size=256, reduce_op="add", out=acc)
    assert torch.allclose(acc.float(), y.float() + 1, rtol=1e-2, atol=1e-2)
    e = torch.empty(0, device="cuda")
    qe, se, ze = pt.quantize_grouped(e, dtype=torch.uint8)
    assert qe.numel() == 0 and se.numel() == 0 and ze.numel() == 0
    with pytest.raises(ValueError):
        pt.quantize_grouped(x, dtype=torch.uint8, scales=s.cpu(), zero_points=z.cpu())
    with pytest.raises(ValueError):
        pt.quantize_grouped(x, dtype=torch.uint8, out=torch.empty(5, dtype=torch.uint8, device="cuda"))


def test_non_default_stream_ordering(ctx):
    import piquant.torch as pt

    n = 1 << 24
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.empty(n, device="cuda")
        x.normal_()
        x.mul_(3.0).add_(1.0)   # still in flight when the grouped calls are enqueued behind it on the same stream
        q, s, z = pt.quantize_grouped(x, dtype=torch.uint8, group_size=128)
        y = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=128)
    side.synchronize()
    xs = x.cpu().numpy()
    ws, wz = group_params_all(xs, 128, O.UINT8)
    assert np.array_equal(s.cpu().numpy(), ws) and np.array_equal(z.cpu().numpy(), wz)
    assert torch.equal(y, pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=128))


def test_graph_capture_replay(ctx):
    import piquant.torch as pt

    n = 1_000_003
    x = torch.randn(n, device="cuda")
    q, s, z = pt.quantize_grouped(x, dtype=torch.quint4x2, group_size=128)   # eager warm-up (context, code objects)
    y = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=128)
    torch.cuda.synchronize()
    want_q, want_s, want_z, want_y = pt.packed_bytes(q).clone(), s.clone(), z.clone(), y.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # one stream: quantize -> dequantize, the parameters flowing through device memory only
        gq, gs, gz = pt.quantize_grouped(x, dtype=torch.quint4x2, group_size=128)
        gy = pt.dequantize_grouped(gq, gs, gz, dtype=torch.float32, group_size=128)
    for _ in range(3):
        gy.zero_()
        gs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pt.packed_bytes(gq), want_q) and torch.equal(gs, want_s) and torch.equal(gz, want_z) and torch.equal(gy, want_y)
