"""The randomized Hadamard rotation of whole groups on the MI355X: piquant.torch.hadamard_grouped / quantize_grouped_rotated /
dequantize_grouped_rotated against the CPU model (tests/rot_model.py), bit for bit -- NaN positions are compared, NaN payloads are not -- and
against the compositions of public calls that define the two fused ones, run on the device in the same process.

Shapes, for every group size G: an empty tensor; G - 1 (only a ragged group: the identity); G (exactly one group); 32 768 (whole groups only);
40 037 (several chunks, a partial chunk and a ragged group)."""
import functools

import numpy as np
import pytest

import oracle as O
import rot_model as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GROUP_SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
PAIR_IDS = ["f32-u8", "f32-u4", "f32-u2", "bf16-u8", "bf16-u4", "bf16-u2"]
SEED, SEED_B = 0x9E37_79B9_7F4A_7C15, -3            # the rotation's; any Python int, taken modulo 2^64
ELEM_SEED, INDEX_BASE = 0x0123_4567_89AB_CDEF, (1 << 32) - 1000   # per-element stochastic mode: the base makes the index cross 2^32
THRESHOLD = 0.37
PAD, CANARY = 64, 0xA5


def sizes(G):
    return (0, G - 1, G, 32768, 40037)


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


@functools.lru_cache(maxsize=None)
def data(n, dt, G, seed=1):
    """heavy-tailed values of the tensor's type (float32, or bfloat16 bits); where there is room, group 1 is one large element among zeros and
    group 2 is constant"""
    rng = np.random.default_rng(seed * 1_000_003 + n)
    x = (rng.standard_normal(n) * rng.uniform(0.01, 30.0, n)).astype(np.float32)
    if n >= 3 * G:
        x[G: 2 * G] = 0.0
        x[G + G // 3] = 1000.0
        x[2 * G: 3 * G] = 3.25
    x = x if dt == O.F32 else O.f32_to_bf16(x)
    x.setflags(write=False)
    return x


def dev(a, dt):
    if dt == O.F32:
        return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()
    return torch.from_numpy(np.array(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def host(t):
    """the tensor's bits: float32 as float32, bfloat16 as uint16"""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def same(got, want, what):
    """bit for bit; NaN positions, not NaN payloads"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.uint16:
        gn, wn = np.isnan(O.bf16_to_f32(got)), np.isnan(O.bf16_to_f32(want))
        g, w = got.copy(), want.copy()
    elif got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    else:
        assert np.array_equal(got, want), f"{what}: first difference at {np.flatnonzero(got != want)[:8].tolist()}"
        return
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8].tolist()}"
    g[gn], w[wn] = 0, 0
    assert np.array_equal(g, w), f"{what}: {np.count_nonzero(g != w)} elements differ, first at {np.flatnonzero(g != w)[:8].tolist()}"


def carve(numel, tdtype, off=0):
    """a tensor of `numel` elements inside a byte buffer full of canaries, `off` elements behind a 16-byte boundary -> (buffer, tensor, first byte)"""
    es = torch.empty(0, dtype=tdtype).element_size()
    buf = torch.full(((numel + off) * es + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    first = PAD + off * es
    return buf, buf[first: first + numel * es].view(tdtype), first


def canaries_intact(buf, first, nbytes, what):
    assert bool((buf[:first] == CANARY).all()), f"{what}: wrote in front of the buffer"
    assert bool((buf[first + nbytes:] == CANARY).all()), f"{what}: wrote past the end of the buffer"


def packed_nbytes(n, qd):
    return (n * {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}[qd] + 7) // 8


def quantize_rotated(x, qd, G, seed, mode, off=0):
    """quantize_grouped_rotated into carved buffers -> (bytes, scales, zero points) on the host, canaries checked"""
    import piquant.torch as pt

    n, ng, nb = x.numel(), (x.numel() + G - 1) // G, packed_nbytes(x.numel(), qd)
    qb, q, q0 = carve(nb, torch.uint8, off)
    sb, s, s0 = carve(ng, torch.float32, off)
    zb, z, z0 = carve(ng, torch.uint8, off)
    got = pt.quantize_grouped_rotated(x, dtype=QDT[qd], group_size=G, seed=seed, round_mode=mode, out=q, out_scales=s, out_zero_points=z)
    torch.cuda.synchronize()
    assert got[0] is q and got[1] is s and got[2] is z
    canaries_intact(qb, q0, nb, "packed bytes")
    canaries_intact(sb, s0, ng * 4, "scales")
    canaries_intact(zb, z0, ng, "zero points")
    return q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()


def triple_same(got, want, what):
    same(got[0], np.asarray(want[0], dtype=np.uint8), what + ": packed bytes")
    same(got[1], np.asarray(want[1], dtype=np.float32), what + ": scales")
    same(got[2], np.asarray(want[2], dtype=np.uint8), what + ": zero points")


# ---- hadamard_grouped

@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "inverse"))
@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_hadamard_grouped(ctx, G, dt, inverse):
    import piquant.torch as pt

    for n in sizes(G):
        x = data(n, dt, G)
        want = R.hadamard_grouped(x, dt, G, SEED, inverse)
        xd = dev(x, dt)
        buf, out, first = carve(n, FDT[dt])
        assert pt.hadamard_grouped(xd, group_size=G, seed=SEED, inverse=inverse, out=out) is out
        torch.cuda.synchronize()
        canaries_intact(buf, first, n * out.element_size(), f"n={n}")
        same(host(out), want, f"out of place, n={n}")
        same(host(xd), x, f"the input, n={n}")
        assert pt.hadamard_grouped(xd, group_size=G, seed=SEED, inverse=inverse, out=xd) is xd
        same(host(xd), want, f"in place, n={n}")
        if n == G - 1:
            assert np.array_equal(want, x)


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_forward_then_inverse_and_seeds(ctx, G):
    """fp32: inverse(forward(x)) is x within (k + 2) 2^-23 max|x| per group (tests/test_grouped_rotated_cpu.py has the reasoning); two seeds give
    different bytes; a seed is taken modulo 2^64."""
    import piquant.torch as pt

    n = 32768 + G // 2
    x = data(n, O.F32, G, seed=2)
    xd = dev(x, O.F32)
    y = pt.hadamard_grouped(xd, group_size=G, seed=SEED)
    back = host(pt.hadamard_grouped(y, group_size=G, seed=SEED, inverse=True))
    full = n // G * G
    err = np.abs(back[:full].astype(np.float64) - x[:full]).reshape(-1, G).max(axis=1)
    assert np.all(err <= (R.log2_of(G) + 2) * 2.0 ** -23 * np.abs(x[:full]).reshape(-1, G).max(axis=1)), err.max()
    assert np.array_equal(back[full:].view(np.uint32), x[full:].view(np.uint32))
    other = host(pt.hadamard_grouped(xd, group_size=G, seed=SEED_B))
    assert not np.array_equal(other[:full], host(y)[:full])
    same(other, R.hadamard_grouped(x, O.F32, G, SEED_B), "a negative seed")
    same(host(pt.hadamard_grouped(xd, group_size=G, seed=SEED_B + (1 << 64))), other, "modulo 2^64")


@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_hadamard_non_finite(ctx, G, dt):
    import piquant.torch as pt

    n = 4 * G + 5
    x = np.array(data(n, O.F32, G, seed=3))
    x[G + 7] = np.nan
    x[2 * G + G - 1] = np.inf
    x[3 * G] = np.inf
    x[3 * G + 17] = -np.inf
    x = x if dt == O.F32 else O.f32_to_bf16(x)
    for inverse in (False, True):
        want = R.hadamard_grouped(x, dt, G, SEED, inverse)
        wf = R.widen(want, dt)
        assert np.all(np.isfinite(wf[:G])) and np.all(np.isnan(wf[G: 2 * G])) and not np.any(np.isfinite(wf[2 * G: 4 * G]))
        same(host(pt.hadamard_grouped(dev(x, dt), group_size=G, seed=SEED, inverse=inverse)), want, f"inverse={inverse}")


# ---- quantize_grouped_rotated

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_quantize_grouped_rotated(ctx, G, pair):
    import piquant.torch as pt

    dt, qd = pair
    for n in sizes(G):
        x = data(n, dt, G)
        xd = dev(x, dt)
        rotated = pt.hadamard_grouped(xd.float(), group_size=G, seed=SEED)

        def composition(mode):
            q, s, z = pt.quantize_grouped(rotated, dtype=QDT[qd], group_size=G, round_mode=mode)
            return pt.packed_bytes(q).cpu().numpy() if n else np.zeros(0, dtype=np.uint8), s.cpu().numpy(), z.cpu().numpy()

        ctx.set_stochastic_per_element(False)
        ctx.set_stochastic_threshold(THRESHOLD)
        got = quantize_rotated(xd, qd, G, SEED, "nearest")
        triple_same(got, R.quantize_grouped_rotated(x, dt, qd, G, SEED), f"nearest, n={n}: model")
        triple_same(got, composition("nearest"), f"nearest, n={n}: composition")
        got = quantize_rotated(xd, qd, G, SEED, "stochastic")
        triple_same(got, R.quantize_grouped_rotated(x, dt, qd, G, SEED, O.STOCHASTIC, THRESHOLD), f"stochastic, n={n}: model")
        triple_same(got, composition("stochastic"), f"stochastic, n={n}: composition")
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(True, seed=ELEM_SEED, index_base=INDEX_BASE)
        got = quantize_rotated(xd, qd, G, SEED, "stochastic")
        triple_same(got, R.quantize_grouped_rotated_per_element(x, dt, qd, G, SEED, ELEM_SEED, INDEX_BASE), f"per element, n={n}: model")
        triple_same(got, composition("stochastic"), f"per element, n={n}: composition")
        ctx.set_stochastic_per_element(False)
        same(host(xd), x, f"the input, n={n}")


# ---- dequantize_grouped_rotated

@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_dequantize_grouped_rotated(ctx, G, pair, op):
    import piquant.torch as pt

    dt, qd = pair
    ctx.set_stochastic_per_element(False)
    for n in sizes(G):
        q, s, z = R.quantize_grouped_rotated(data(n, O.F32, G), O.F32, qd, G, SEED)
        qd_, sd, zd = torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(z).cuda()
        prev = data(n, dt, G, seed=5) if op == "add" else None
        want = R.dequantize_grouped_rotated(q, qd, dt, n, G, s, z, SEED, O.ADD if op == "add" else O.SET, prev)
        buf, out, first = carve(n, FDT[dt])
        if op == "add":
            out.copy_(dev(prev, dt))
        kw = dict(dtype=FDT[dt], group_size=G, quant_dtype=QDT[qd], shape=(n,))
        assert pt.dequantize_grouped_rotated(qd_, sd, zd, seed=SEED, reduce_op=op, out=out, **kw) is out
        torch.cuda.synchronize()
        canaries_intact(buf, first, n * out.element_size(), f"n={n}")
        same(host(out), want, f"n={n}: model")
        zf = pt.hadamard_grouped(pt.dequantize_grouped(qd_, sd, zd, dtype=torch.float32, group_size=G, quant_dtype=QDT[qd], shape=(n,)),
                                 group_size=G, seed=SEED, inverse=True)
        comp = zf.to(FDT[dt]) if op == "set" else (dev(prev, dt).float() + zf).to(FDT[dt])
        same(host(out), host(comp), f"n={n}: composition")
        if op == "set" and n:
            assert pt.dequantize_grouped_rotated(qd_, sd, zd, seed=SEED, **kw).shape == (n,)


# ---- buffers one element off a 16-byte boundary: the guarded kernels, the same bytes

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_misaligned_buffers_give_the_same_bytes(ctx, pair):
    import piquant.torch as pt

    dt, qd = pair
    ctx.set_stochastic_per_element(False)
    for G, n in ((128, 128 * 9 + 77), (4096, 4096 * 2 + 1), (32, 31)):
        x = data(n, dt, G, seed=7)
        nb, ng = packed_nbytes(n, qd), (n + G - 1) // G
        xb, xm, x0 = carve(n, FDT[dt], off=1)
        xm.copy_(dev(x, dt))
        assert xm.data_ptr() % 16 != 0
        for inverse in (False, True):
            ob, om, o0 = carve(n, FDT[dt], off=1)
            pt.hadamard_grouped(xm, group_size=G, seed=SEED, inverse=inverse, out=om)
            torch.cuda.synchronize()
            canaries_intact(ob, o0, n * om.element_size(), "hadamard_grouped out")
            same(host(om), R.hadamard_grouped(x, dt, G, SEED, inverse), f"hadamard_grouped, G={G}, inverse={inverse}")
        inplace = xm.clone()   # a clone is aligned; rotate the misaligned tensor in place and compare
        pt.hadamard_grouped(xm, group_size=G, seed=SEED, out=xm)
        same(host(xm), host(pt.hadamard_grouped(inplace, group_size=G, seed=SEED)), f"in place, G={G}")
        canaries_intact(xb, x0, n * xm.element_size(), "hadamard_grouped in place")
        xm.copy_(dev(x, dt))
        for mode, threshold in (("nearest", None), ("stochastic", THRESHOLD)):
            ctx.set_stochastic_threshold(threshold)
            got = quantize_rotated(xm, qd, G, SEED, mode, off=1)
            triple_same(got, quantize_rotated(dev(x, dt), qd, G, SEED, mode), f"quantize_grouped_rotated {mode}, G={G}")
            triple_same(got, R.quantize_grouped_rotated(x, dt, qd, G, SEED, O.STOCHASTIC if threshold else O.NEAREST, threshold or 0.0),
                        f"quantize_grouped_rotated {mode}, G={G}: model")
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(True, seed=ELEM_SEED, index_base=INDEX_BASE)
        triple_same(quantize_rotated(xm, qd, G, SEED, "stochastic", off=1),
                    R.quantize_grouped_rotated_per_element(x, dt, qd, G, SEED, ELEM_SEED, INDEX_BASE), f"per element, G={G}")
        ctx.set_stochastic_per_element(False)
        canaries_intact(xb, x0, n * xm.element_size(), "the input of quantize_grouped_rotated")
        q, s, z = got
        qb, qm, _ = carve(nb, torch.uint8, off=1)
        sb, sm, _ = carve(ng, torch.float32, off=1)
        zb, zm, _ = carve(ng, torch.uint8, off=1)
        qm.copy_(torch.from_numpy(q))
        sm.copy_(torch.from_numpy(s))
        zm.copy_(torch.from_numpy(z))
        prev = data(n, dt, G, seed=8)
        for op in ("set", "add"):
            ob, om, o0 = carve(n, FDT[dt], off=1)
            om.copy_(dev(prev, dt))
            pt.dequantize_grouped_rotated(qm, sm, zm, dtype=FDT[dt], group_size=G, seed=SEED, reduce_op=op, out=om, quant_dtype=QDT[qd], shape=(n,))
            torch.cuda.synchronize()
            canaries_intact(ob, o0, n * om.element_size(), "dequantize_grouped_rotated out")
            same(host(om), R.dequantize_grouped_rotated(q, qd, dt, n, G, s, z, SEED, O.ADD if op == "add" else O.SET, prev),
                 f"dequantize_grouped_rotated {op}, G={G}")


# ---- hipGraph capture

def test_graph_capture_and_replay(ctx):
    import piquant.torch as pt

    G, n, qd = 128, 40037, O.UINT4
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    x = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    acc = torch.zeros(n, device="cuda")
    inputs = [dev(data(n, O.BF16, G, seed=20 + i), O.BF16) for i in range(2)]
    x.copy_(inputs[0])

    def calls(src, accumulate):
        y = pt.hadamard_grouped(src, group_size=G, seed=SEED)
        q, s, z = pt.quantize_grouped_rotated(src, dtype=QDT[qd], group_size=G, seed=SEED)
        back = pt.dequantize_grouped_rotated(q, s, z, dtype=torch.bfloat16, group_size=G, seed=SEED)
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=G, seed=SEED, reduce_op="add", out=accumulate)
        return y, q, s, z, back

    calls(x, torch.zeros_like(acc))   # warm-up outside capture (code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = calls(x, acc)
    want_acc = torch.zeros_like(acc)
    for fresh in inputs:
        x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = calls(fresh, want_acc)
        torch.cuda.synchronize()
        for got, want, name in zip(captured, eager, ("rotated", "packed", "scales", "zero points", "round trip")):
            g = pt.packed_bytes(got) if got.dtype in QDT.values() and got.dtype != torch.uint8 else got
            w = pt.packed_bytes(want) if want.dtype in QDT.values() and want.dtype != torch.uint8 else want
            same(host(g), host(w), f"captured {name}")
        same(host(acc), host(want_acc), "captured ADD")


# ---- what the rotation is for

def test_rotation_gains_on_outliers_on_the_device(ctx):
    """The CPU test's one fixed ratio on the device: G = 128, uint4, N(0, 1) with one 50 sigma element per group, 4 096 groups: the rotated round
    trip's MSE is at most 0.25 of the un-rotated one's."""
    import piquant.torch as pt

    G = 128
    ctx.set_stochastic_per_element(False)
    x = R.outlier_data(G, 4096, 11)
    xd = dev(x, O.F32)
    q, s, z = pt.quantize_grouped(xd, dtype=torch.quint4x2, group_size=G)
    plain = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=G)
    q, s, z = pt.quantize_grouped_rotated(xd, dtype=torch.quint4x2, group_size=G, seed=SEED)
    rotated = pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=G, seed=SEED)
    mse_plain = float(np.mean((host(plain).astype(np.float64) - x) ** 2))
    mse_rotated = float(np.mean((host(rotated).astype(np.float64) - x) ** 2))
    print(f"G=128 uint4 outliers on the device: MSE rotated / plain = {mse_rotated:.6g} / {mse_plain:.6g} = {mse_rotated / mse_plain:.4f}")
    assert mse_rotated <= 0.25 * mse_plain


# ---- wrong arguments raise before any launch

def test_wrong_arguments_raise_value_error(ctx):
    import piquant.torch as pt

    x = torch.zeros(1000, device="cuda")
    q = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    s, z = torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")
    for bad in (100, 16, 8192, None):
        with pytest.raises(ValueError, match="group_size"):
            pt.hadamard_grouped(x, group_size=bad, seed=1)
        with pytest.raises(ValueError, match="group_size"):
            pt.quantize_grouped_rotated(x, dtype=torch.quint4x2, group_size=bad, seed=1)
        with pytest.raises(ValueError, match="group_size"):
            pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=bad, seed=1)
    for t in (q, torch.zeros(1000, dtype=torch.float16, device="cuda"), torch.zeros(1000, dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            pt.hadamard_grouped(t, seed=1)
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            pt.quantize_grouped_rotated(t, dtype=torch.quint4x2, seed=1)
    with pytest.raises(ValueError, match="must live on"):
        pt.dequantize_grouped_rotated(q, s.cpu(), z, dtype=torch.float32, group_size=128, seed=1)
    with pytest.raises(ValueError, match="on cuda"):
        pt.quantize_grouped_rotated(x, dtype=torch.quint4x2, seed=1, out_scales=s.cpu(), out_zero_points=z)
    with pytest.raises(ValueError, match="seed"):
        pt.hadamard_grouped(x)
    with pytest.raises(ValueError, match="seed"):
        pt.quantize_grouped_rotated(x, dtype=torch.quint4x2)
    with pytest.raises(ValueError, match="seed"):
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=128)
    with pytest.raises(ValueError, match="accumulates into out"):
        pt.dequantize_grouped_rotated(q, s, z, dtype=torch.float32, group_size=128, seed=1, reduce_op="add")
    with pytest.raises(ValueError, match="out must be"):
        pt.hadamard_grouped(x, seed=1, out=torch.zeros(999, device="cuda"))
    torch.cuda.synchronize()
