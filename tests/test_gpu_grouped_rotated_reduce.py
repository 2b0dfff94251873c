"""The two steps of a grouped collective in the rotated domain on the MI355X: piquant.torch.reduce_quantize_grouped_rotated and
dequantize_sum_grouped_rotated against the CPU model (tests/grouped_rotated_sim.py) and against the compositions of public calls that define
them, run on the device in the same process -- bit for bit; NaN positions are compared, NaN payloads are not.

Shape, for every group size G and width: with NG the groups of a wave's chunk of the float32 tile and four waves a block,
numel = 9 NG G + 3 G + 5 -- two full blocks, a chunk the tensor ends in that still holds whole groups, a ragged last group -- and numel < G,
numel == G.  Terms are records of rotated heavy-tailed values; counts 0 (reduce only), 1, 2, 7, 16."""
import functools

import numpy as np
import pytest

import oracle as O
import grouped_model as GM
import grouped_rotated_sim as S
import rot_model as R
import test_gpu_grouped_rotated as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ctx = T.ctx   # the module's context fixture: threshold and per-element mode restored at the end

SEED = 0x1234_5678_8765_4321
COUNTS = (0, 1, 2, 7, 16)
BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
# all eight group sizes for fp32 -> uint8 and bf16 -> uint4, three for the other four pairs
CASES = [(pair, G) for pair in T.PAIRS for G in (T.GROUP_SIZES if pair in ((O.F32, O.UINT8), (O.BF16, O.UINT4)) else (32, 128, 4096))]
CASE_IDS = [f"{T.PAIR_IDS[T.PAIRS.index(pair)]}-G{G}" for pair, G in CASES]


def chunk_groups(qd, G):
    """NG of GroupedQuantTile<float32, bits, G> (csrc/grouped_kernels.hpp)"""
    ob, v = 4 * BITS[qd] // 8, G // 4
    rpg, want = (1 if v < 64 else v // 64), max(16 // ob, 4)
    nv = max(rpg, min(v, want))
    assert nv * 256 % G == 0
    return nv * 256 // G


def numel_of(qd, G):
    return 9 * chunk_groups(qd, G) * G + 3 * G + 5


@functools.lru_cache(maxsize=None)
def terms_of(qd, G, n, k=16, base=40):
    """k records of rotated values on the host: (packed bytes, scales, zero points)"""
    return tuple(R.quantize_grouped_rotated(T.data(n, O.F32, G, seed=base + i), O.F32, qd, G, SEED) for i in range(k))


def put(a, tdtype, off=0):
    """a host array in a carved device buffer, `off` elements behind a 16-byte boundary -> (buffer, tensor, first byte)"""
    buf, t, first = T.carve(a.size, tdtype, off)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, t, first


def terms_dev(terms, off_q=0, off_p=0, which=None):
    """the records on the device; record `which` (None: every one) takes the offsets"""
    out = []
    for i, (q, s, z) in enumerate(terms):
        oq, op = (off_q, off_p) if which is None or which == i else (0, 0)
        out.append((put(q, torch.uint8, oq)[1], put(s, torch.float32, op)[1], put(z, torch.uint8, op)[1]))
    return out


def reduce_rotated(acc, terms, qd, G, mode, off_out=0, off_params=0):
    """reduce_quantize_grouped_rotated into carved buffers -> (bytes, scales, zero points) on the host, canaries checked"""
    import piquant.torch as pt

    n, ng, nb = acc.numel(), (acc.numel() + G - 1) // G, T.packed_nbytes(acc.numel(), qd)
    qb, q, q0 = T.carve(nb, torch.uint8, off_out)
    sb, s, s0 = T.carve(ng, torch.float32, off_params)
    zb, z, z0 = T.carve(ng, torch.uint8, off_params)
    got = pt.reduce_quantize_grouped_rotated(acc, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=T.QDT[qd], group_size=G,
                                             seed=SEED, round_mode=mode, out=q, out_scales=s, out_zero_points=z)
    torch.cuda.synchronize()
    assert got[0] is q and got[1] is s and got[2] is z
    T.canaries_intact(qb, q0, nb, "packed bytes")
    T.canaries_intact(sb, s0, ng * 4, "scales")
    T.canaries_intact(zb, z0, ng, "zero points")
    return q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()


def reduce_composition(acc, terms, qd, G, mode):
    """hadamard_grouped of the widened accumulator, one float32 dequantize ADD per term, quantize_grouped"""
    import piquant.torch as pt

    n = acc.numel()
    y = pt.hadamard_grouped(acc.float(), group_size=G, seed=SEED)
    for q, s, z in terms:
        pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=G, reduce_op="add", out=y, quant_dtype=T.QDT[qd], shape=(n,))
    q, s, z = pt.quantize_grouped(y, dtype=T.QDT[qd], group_size=G, round_mode=mode)
    return (pt.packed_bytes(q).cpu().numpy() if n else np.zeros(0, dtype=np.uint8)), s.cpu().numpy(), z.cpu().numpy()


def sum_rotated(terms, qd, dt, n, G, op, prev, off_out=0):
    """dequantize_sum_grouped_rotated into a carved buffer (holding `prev`) -> the tensor's bits on the host, canaries checked"""
    import piquant.torch as pt

    buf, out, first = T.carve(n, T.FDT[dt], off_out)
    out.copy_(T.dev(prev, dt))
    got = pt.dequantize_sum_grouped_rotated([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=T.FDT[dt], group_size=G, seed=SEED,
                                            reduce_op=op, out=out, quant_dtype=T.QDT[qd], shape=(n,))
    torch.cuda.synchronize()
    assert got is out
    T.canaries_intact(buf, first, n * out.element_size(), "out")
    return T.host(out)


def sum_composition(terms, qd, dt, n, G, op, prev):
    """float32 dequantize SET of the first term and ADD of the others, hadamard_grouped inverse, then the convert or the one add"""
    import piquant.torch as pt

    kw = dict(dtype=torch.float32, group_size=G, quant_dtype=T.QDT[qd], shape=(n,))
    s = pt.dequantize_grouped(*terms[0], **kw)
    for t in terms[1:]:
        pt.dequantize_grouped(*t, reduce_op="add", out=s, **kw)
    z = pt.hadamard_grouped(s, group_size=G, seed=SEED, inverse=True)
    return T.host(z.to(T.FDT[dt]) if op == "set" else (T.dev(prev, dt).float() + z).to(T.FDT[dt]))


def modes(ctx):
    """(name, the call's round_mode, arm the context, the model's quantize of the float32 sum y)"""
    def nearest():
        ctx.set_stochastic_per_element(False)
        ctx.set_stochastic_threshold(None)

    def stochastic():
        ctx.set_stochastic_per_element(False)
        ctx.set_stochastic_threshold(T.THRESHOLD)

    def per_element():
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(True, seed=T.ELEM_SEED, index_base=T.INDEX_BASE)

    import per_element_model as PE

    return [("nearest", "nearest", nearest, lambda y, qd, G: GM.quantize_grouped(y, O.F32, qd, G)),
            ("stochastic", "stochastic", stochastic, lambda y, qd, G: GM.quantize_grouped(y, O.F32, qd, G, O.STOCHASTIC, T.THRESHOLD)),
            ("per element", "stochastic", per_element, lambda y, qd, G: PE.quantize(y, O.F32, qd, G, T.ELEM_SEED, T.INDEX_BASE))]


# ---- reduce_quantize_grouped_rotated

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reduce_quantize_grouped_rotated(ctx, case):
    (dt, qd), G = case
    n = numel_of(qd, G)
    acc = T.data(n, dt, G, seed=30)
    ab, accd, a0 = T.carve(n, T.FDT[dt])
    accd.copy_(T.dev(acc, dt))
    host_terms = terms_of(qd, G, n)
    dev_terms = terms_dev(host_terms)
    try:
        for k in COUNTS:
            y = S.rotated_sum(acc, dt, host_terms[:k], qd, G, SEED)
            for name, mode, arm, model in modes(ctx):
                arm()
                got = reduce_rotated(accd, dev_terms[:k], qd, G, mode)
                T.triple_same(got, model(y, qd, G), f"{name}, {k} terms: model")
                T.triple_same(got, reduce_composition(accd, dev_terms[:k], qd, G, mode), f"{name}, {k} terms: composition")
                if k == 0:
                    T.triple_same(got, T.quantize_rotated(accd, qd, G, SEED, mode), f"{name}: no terms is quantize_grouped_rotated")
    finally:
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(False)
    T.same(T.host(accd), acc, "acc is only read")
    T.canaries_intact(ab, a0, n * accd.element_size(), "acc")


@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_reduce_of_short_tensors(ctx, pair):
    dt, qd = pair
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    for G in (32, 128, 4096):
        for n in (0, G - 1, G):
            acc = T.data(n, dt, G, seed=31)
            accd = T.dev(acc, dt)
            for k in (0, 2):
                host_terms = terms_of(qd, G, n, 2, 60)
                got = reduce_rotated(accd, terms_dev(host_terms[:k]), qd, G, "nearest")
                T.triple_same(got, S.reduce_quantize_grouped_rotated(acc, dt, host_terms[:k], qd, G, SEED), f"G={G}, n={n}, {k} terms")


# ---- dequantize_sum_grouped_rotated

def old_contents(n, dt, G):
    """what an ADD finds in out: heavy-tailed values with -0.0 and NaN among them"""
    prev = np.array(T.data(n, O.F32, G, seed=33))
    prev[::11] = -0.0
    prev[5::1013] = np.nan
    return prev if dt == O.F32 else O.f32_to_bf16(prev)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dequantize_sum_grouped_rotated(ctx, case):
    (dt, qd), G = case
    n = numel_of(qd, G)
    host_terms = terms_of(qd, G, n)
    dev_terms = terms_dev(host_terms)
    prev = old_contents(n, dt, G)
    for k in COUNTS[1:]:
        for op, o in (("set", O.SET), ("add", O.ADD)):
            got = sum_rotated(dev_terms[:k], qd, dt, n, G, op, prev)
            T.same(got, S.dequantize_sum_grouped_rotated(host_terms[:k], qd, dt, n, G, SEED, o, prev), f"{op}, {k} terms: model")
            T.same(got, sum_composition(dev_terms[:k], qd, dt, n, G, op, prev), f"{op}, {k} terms: composition")
            if k == 1:
                import piquant.torch as pt

                one = T.dev(prev, dt)
                pt.dequantize_grouped_rotated(*dev_terms[0], dtype=T.FDT[dt], group_size=G, seed=SEED, reduce_op=op, out=one, quant_dtype=T.QDT[qd],
                                              shape=(n,))
                T.same(got, T.host(one), f"{op}: one term is dequantize_grouped_rotated")


@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_sum_of_short_tensors(ctx, pair):
    dt, qd = pair
    for G in (32, 128, 4096):
        for n in (0, G - 1, G):
            host_terms = terms_of(qd, G, n, 2, 60)
            prev = old_contents(n, dt, G)
            for op, o in (("set", O.SET), ("add", O.ADD)):
                got = sum_rotated(terms_dev(host_terms), qd, dt, n, G, op, prev)
                T.same(got, S.dequantize_sum_grouped_rotated(host_terms, qd, dt, n, G, SEED, o, prev), f"G={G}, n={n}, {op}")


# ---- a NaN term and a sum that overflows

@pytest.mark.parametrize("pair", [(O.F32, O.UINT8), (O.BF16, O.UINT4)], ids=("f32-u8", "bf16-u4"))
def test_non_finite_terms(ctx, pair):
    """group 1 of the second term dequantizes to NaN (its scale is NaN); group 2 of the first two terms holds values near FLT_MAX, whose float32
    sum overflows to inf.  The reduce adds behind the rotation, the sum rotates behind the adds: both against the model and the composition."""
    dt, qd = pair
    G = 128
    n = numel_of(qd, G)
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    host_terms = [tuple(np.array(a) for a in t) for t in terms_of(qd, G, n, 3, 70)]
    host_terms[1][1][1] = np.nan
    host_terms[0][1][2] = host_terms[1][1][2] = np.float32(3.0e38) / np.float32((1 << BITS[qd]) - 1)
    host_terms[0][2][2] = host_terms[1][2][2] = 0
    host_terms[0][0][2 * G * BITS[qd] // 8: 3 * G * BITS[qd] // 8] = 0xFF
    host_terms[1][0][2 * G * BITS[qd] // 8: 3 * G * BITS[qd] // 8] = 0xFF
    dev_terms = terms_dev(host_terms)
    with np.errstate(over="ignore", invalid="ignore"):
        s = S.terms_sum(host_terms, qd, n, G)
        assert np.all(np.isnan(s[G: 2 * G])) and np.all(np.isinf(s[2 * G: 3 * G])) and np.all(np.isfinite(s[3 * G:]))
        prev = old_contents(n, dt, G)
        for op, o in (("set", O.SET), ("add", O.ADD)):
            got = sum_rotated(dev_terms, qd, dt, n, G, op, prev)
            T.same(got, S.dequantize_sum_grouped_rotated(host_terms, qd, dt, n, G, SEED, o, prev), f"sum {op}: model")
            T.same(got, sum_composition(dev_terms, qd, dt, n, G, op, prev), f"sum {op}: composition")
        acc = T.data(n, dt, G, seed=34)
        accd = T.dev(acc, dt)
        got = reduce_rotated(accd, dev_terms, qd, G, "nearest")
        T.triple_same(got, reduce_composition(accd, dev_terms, qd, G, "nearest"), "reduce: composition")
        T.triple_same(got, S.reduce_quantize_grouped_rotated(acc, dt, host_terms, qd, G, SEED), "reduce: model")


# ---- one buffer at a time off a 16-byte boundary: the guarded kernels, the same bytes

@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_misaligned_buffers_give_the_same_bytes(ctx, pair):
    dt, qd = pair
    k = 3
    try:
        for G, n in ((128, 128 * 9 + 77), (4096, 4096 * 2 + 1), (32, 32 * 40 + 31)):
            acc = T.data(n, dt, G, seed=35)
            host_terms = terms_of(qd, G, n, k, 80)
            prev = old_contents(n, dt, G)
            y = S.rotated_sum(acc, dt, host_terms, qd, G, SEED)
            for name, mode, arm, model in modes(ctx):
                arm()
                want = model(y, qd, G)
                for what, kw_acc, kw_terms, kw_out in (("acc", 1, {}, {}), ("out", 0, {}, dict(off_out=1)), ("a term", 0, dict(off_q=1, which=1), {}),
                                                       ("the parameter arrays", 0, dict(off_p=1), dict(off_params=1))):
                    ab, accm, a0 = T.carve(n, T.FDT[dt], kw_acc)
                    accm.copy_(T.dev(acc, dt))
                    got = reduce_rotated(accm, terms_dev(host_terms, **kw_terms), qd, G, mode, **kw_out)
                    T.triple_same(got, want, f"reduce, G={G}, {name}, {what} misaligned")
                    T.same(T.host(accm), acc, "acc is only read")
                    T.canaries_intact(ab, a0, n * accm.element_size(), "acc")
            ctx.set_stochastic_per_element(False)
            ctx.set_stochastic_threshold(None)
            for op, o in (("set", O.SET), ("add", O.ADD)):
                want = S.dequantize_sum_grouped_rotated(host_terms, qd, dt, n, G, SEED, o, prev)
                for what, kw_terms, off_out in (("out", {}, 1), ("a term", dict(off_q=1, which=2), 0), ("the parameter arrays", dict(off_p=1), 0)):
                    T.same(sum_rotated(terms_dev(host_terms, **kw_terms), qd, dt, n, G, op, prev, off_out), want, f"sum {op}, G={G}, {what} misaligned")
    finally:
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(False)


# ---- more than sixteen terms

def test_seventeen_terms_raise(ctx):
    import piquant.torch as pt

    G, n, qd = 128, 1000, O.UINT8
    terms = terms_dev(terms_of(qd, G, n, 1, 90) * 17)
    lists = ([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms])
    acc = torch.ones(n, device="cuda")
    with pytest.raises(ValueError, match="at most 16"):
        pt.reduce_quantize_grouped_rotated(acc, *lists, dtype=torch.uint8, group_size=G, seed=SEED)
    with pytest.raises(ValueError, match="at most 16"):
        pt.dequantize_sum_grouped_rotated(*lists, dtype=torch.float32, group_size=G, seed=SEED, quant_dtype=torch.uint8, shape=(n,))
    with pytest.raises(ValueError, match="seed"):
        pt.reduce_quantize_grouped_rotated(acc, *(x[:2] for x in lists), dtype=torch.uint8, group_size=G)
    with pytest.raises(ValueError, match="seed"):
        pt.dequantize_sum_grouped_rotated(*(x[:2] for x in lists), dtype=torch.float32, group_size=G, quant_dtype=torch.uint8, shape=(n,))
    with pytest.raises(ValueError, match="at least one"):
        pt.dequantize_sum_grouped_rotated([], [], [], dtype=torch.float32, group_size=G, seed=SEED, quant_dtype=torch.uint8, shape=(n,))
    torch.cuda.synchronize()
    assert bool((acc == 1).all())


# ---- hipGraph capture

def test_graph_capture_and_replay(ctx):
    import piquant.torch as pt

    G, qd, k = 128, O.UINT4, 3
    n = numel_of(qd, G)
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    terms = terms_dev(terms_of(qd, G, n, k, 95))
    lists = ([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms])
    inputs = [T.dev(T.data(n, O.BF16, G, seed=96 + i), O.BF16) for i in range(2)]
    x = inputs[0].clone()
    total = torch.zeros(n, device="cuda")

    def calls(src, accumulate):
        raw = torch.empty(T.packed_nbytes(n, qd), dtype=torch.uint8, device="cuda")
        q, s, z = pt.reduce_quantize_grouped_rotated(src, *lists, dtype=T.QDT[qd], group_size=G, seed=SEED, out=raw)
        kw = dict(group_size=G, seed=SEED, quant_dtype=T.QDT[qd], shape=(n,))
        back = pt.dequantize_sum_grouped_rotated([q] + lists[0][:1], [s] + lists[1][:1], [z] + lists[2][:1], dtype=torch.bfloat16, **kw)
        pt.dequantize_sum_grouped_rotated(*lists, dtype=torch.float32, reduce_op="add", out=accumulate, **kw)
        return q, s, z, back

    calls(x, torch.zeros_like(total))   # warm-up outside capture (code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = calls(x, total)
    want_total = torch.zeros_like(total)
    for fresh in inputs:
        x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = calls(fresh, want_total)
        torch.cuda.synchronize()
        for got, want, name in zip(captured, eager, ("packed", "scales", "zero points", "sum")):
            T.same(T.host(got), T.host(want), f"captured {name}")
        T.same(T.host(total), T.host(want_total), "captured ADD")
