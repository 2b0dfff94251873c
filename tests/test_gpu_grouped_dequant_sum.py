"""The grouped dequantize-sum (piquant_hip_dequantize_sum_grouped / piquant.torch.dequantize_sum_grouped) on the MI355X.

The call is specified as a composition of public calls that tests/test_gpu_grouped.py pins against the CPU group model: dequantize_grouped of
every term into out, in order, the first with the call's op and the others with ADD.  Its bytes are compared bit for bit with that composition
run on the device in the same process (every dtype pair, SET and ADD, the launch split at 16 terms, whole and ragged tiles), and with the CPU
model chained with prev=.  NaN positions are compared, NaN payloads are not."""
import numpy as np
import pytest

import oracle as O
from grouped_model import dequantize_grouped

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64                    # sentinel elements (out) / bytes (terms) on either side; keeps the 16-byte alignment of what lies between
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
COUNTS = (1, 2, 7, 16, 17, 33)   # one launch, the limit of one launch, the split at 16 and a third launch
SOME_COUNTS = (1, 2, 16, 17)     # the group sizes between 32, 128 and 4096: the instances of one and of several terms, and the split
GROUP_SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)


def tile_elems(dt, qd, G):
    """Elements of one wave's chunk: GroupedQuantTile<DT_OUT, BITS, G>::CHUNK_ELEMS of csrc/grouped_kernels.hpp, whose rows are 16-byte vectors of the
    FLOAT type (the kernel's geometry, restated: the sizes below must straddle it)."""
    epv = 4 if dt == O.F32 else 8
    ob = epv * BITS[qd] // 8
    v = G // epv
    rpg = 1 if v < 64 else v // 64
    nv_want = max(16 // ob, 4)
    nv = max(rpg, min(v, nv_want))
    return nv * 64 * epv


def sizes(dt, qd, G):
    t = tile_elems(dt, qd, G)
    return [1, G - 1, 3 * t + G + 5, t]   # 3 tiles + G + 5: a partial chunk whose ragged end lies inside a 16-byte vector


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    return piquant.Context.get(0)


def _ibits(t):
    return t.view(-1).view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rand(n, fdt, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(n, device="cuda", generator=g)
    if n > 16:
        x *= torch.linspace(0.01, 30.0, n, device="cuda")[torch.randperm(n, device="cuda", generator=g)]
    return x.to(fdt)


def make_terms(n, fdt, qd, G, k, seed):
    """k packed terms of n elements with their per-group parameters, each in a buffer with GUARD sentinel bytes on either side."""
    import piquant.torch as pt

    out = []
    for i in range(k):
        q, s, z = pt.quantize_grouped(_rand(n, fdt, seed + i), dtype=QDT[qd], group_size=G)
        raw = pt.packed_bytes(q) if q.dtype != torch.uint8 else q.view(-1)
        buf = torch.full((raw.numel() + 2 * GUARD,), 0x5C, dtype=torch.uint8, device="cuda")
        buf[GUARD: GUARD + raw.numel()] = raw
        out.append((buf, s, z))
    return out


def raw_of(term):
    return term[0][GUARD: term[0].numel() - GUARD]


def check_term_guards(terms, saved):
    for (buf, _, _), keep in zip(terms, saved):
        assert torch.equal(buf, keep), "a term buffer (or its guard band) was modified"


def new_out(init, n, fdt, fill):
    """out of n elements inside a buffer with GUARD sentinel elements on either side; `init` (ADD) or a fill value (SET)."""
    buf = torch.full((n + 2 * GUARD,), -7.0, dtype=fdt, device="cuda")
    mid = buf[GUARD: GUARD + n]
    if init is not None:
        mid.copy_(init)
    else:
        mid.fill_(fill)
    return buf, mid


def fused(terms, init, op, fdt, qd, G, n, fill=float("nan"), via="torch", c=None):
    """dequantize_sum_grouped into a guarded out; -> out on the device, guards of out and of the terms checked."""
    import piquant
    import piquant.torch as pt

    buf, mid = new_out(init, n, fdt, fill)
    saved = [t[0].clone() for t in terms]
    if via == "torch":
        got = pt.dequantize_sum_grouped([raw_of(t) for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=fdt, group_size=G, reduce_op=op,
                                        out=mid, quant_dtype=QDT[qd], shape=(n,))
        assert got is mid
    else:
        c = c or piquant.Context.get(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_blocking(False)
        c.dequantize_sum_grouped_ptr([raw_of(t).data_ptr() for t in terms], pt.torch_to_piquant_dtype(QDT[qd]), [t[1].data_ptr() for t in terms],
                                     [t[2].data_ptr() for t in terms], mid.data_ptr(), pt.torch_to_piquant_dtype(fdt), n, G,
                                     piquant.ReduceOp.ADD if op == "add" else piquant.ReduceOp.SET, _device_ptrs=True)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -7.0).all()), "wrote in front of out"
    assert bool((buf[GUARD + n:] == -7.0).all()), "wrote past the end of out"
    check_term_guards(terms, saved)
    return mid.clone()


def composition(terms, init, op, fdt, qd, G, n):
    """The specification: dequantize_grouped per term in order into out, the first with `op`, the others with 'add'."""
    import piquant.torch as pt

    a = init.clone() if init is not None else torch.full((n,), float("nan"), dtype=fdt, device="cuda")
    for i, t in enumerate(terms):
        pt.dequantize_grouped(raw_of(t), t[1], t[2], dtype=fdt, group_size=G, reduce_op=op if i == 0 else "add", out=a, quant_dtype=QDT[qd], shape=(n,))
    torch.cuda.synchronize()
    return a


def same(got, want, what=""):
    """Bit for bit, NaN positions but not NaN payloads."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ at {torch.nonzero(gn != wn).flatten()[:8].tolist()}"
    g, w = _ibits(got).clone(), _ibits(want).clone()
    g[gn.view(-1)] = 0
    w[wn.view(-1)] = 0
    bad = torch.nonzero(g != w).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at {bad[:8].tolist()}"


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_fused_equals_the_composition(ctx, dt, qd, G):
    fdt = FDT[dt]
    counts = COUNTS if G in (32, 128, 4096) else SOME_COUNTS
    for i, n in enumerate(sizes(dt, qd, G)):
        terms = make_terms(n, fdt, qd, G, max(counts), 100 * i + G + qd)
        init = _rand(n, fdt, 7 + i)
        for k in counts:
            for op in ("set", "add"):
                start = init if op == "add" else None
                same(fused(terms[:k], start, op, fdt, qd, G, n), composition(terms[:k], start, op, fdt, qd, G, n), f"n={n} k={k} {op}")


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_fused_equals_the_cpu_group_model(ctx, dt, qd):
    """Against tests/grouped_model.py directly: dequantize_grouped chained with prev=, the first term SET or ADD."""
    G = 128
    against_the_cpu_group_model(dt, qd, G, 3 * tile_elems(dt, qd, G) + G + 5, 3)


def against_the_cpu_group_model(dt, qd, G, n, k):
    fdt = FDT[dt]

    def host(t):
        return t.view(torch.int16).cpu().numpy().view(np.uint16) if dt == O.BF16 else t.cpu().numpy()

    terms = make_terms(n, fdt, qd, G, k, 900 + qd)
    init = _rand(n, fdt, 31)
    for op in ("set", "add"):
        a = host(init).copy() if op == "add" else None
        for i, t in enumerate(terms):
            a = dequantize_grouped(raw_of(t).cpu().numpy(), qd, dt, n, G, t[1].cpu().numpy(), t[2].cpu().numpy(), O.SET if (op == "set" and i == 0) else O.ADD,
                                   prev=a)
        got = host(fused(terms, init if op == "add" else None, op, fdt, qd, G, n))
        bad = np.flatnonzero(got.view(np.uint16 if dt == O.BF16 else np.uint32) != a.view(np.uint16 if dt == O.BF16 else np.uint32))
        assert bad.size == 0, f"G={G} n={n} k={k} {op}: {bad.size} elements differ from the CPU model, first at {bad[:8]}"


@pytest.mark.parametrize("dt,qd", PAIRS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_fused_equals_the_cpu_group_model_at_every_group_size(ctx, dt, qd, G):
    """Every group size has its own instances of grouped_set_term, grouped_add_term and grouped_park_term_partial: one tile less one element, exactly
    one tile, and three tiles with a ragged chunk and a ragged group; one term and three; SET and ADD."""
    tile = tile_elems(dt, qd, G)
    for n in (tile - 1, tile, 3 * tile + G + 5):
        for k in (1, 3):
            against_the_cpu_group_model(dt, qd, G, n, k)


def edge_terms(n, qd, G, k, seed):
    """Terms whose parameters the caller gives: per-group scales drawn from {negative, 0, -0, +-inf, NaN, denormal, 2^-8, ordinary}, arbitrary zero
    points, random bytes -- and in every third group bytes EQUAL to the zero point in every element, so that 0 * scale (-0.0 for a negative
    scale, NaN for an infinite one) is what the term contributes there."""
    rng = np.random.default_rng(seed)
    ng, bits = -(-n // G), BITS[qd]
    qmax, pack = (1 << bits) - 1, 8 // bits
    pool = np.array([-0.75, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-41, 2.0 ** -8, 0.0123, 3.5], dtype=np.float32)
    out = []
    for i in range(k):
        s = pool[(np.arange(ng) + i) % pool.size].copy()
        z = rng.integers(0, qmax + 1, ng).astype(np.uint8)
        raw = rng.integers(0, 256, (n * bits + 7) // 8).astype(np.uint8)
        for g in range(0, ng, 3):
            rep = 0
            for j in range(pack):
                rep |= int(z[g]) << (j * bits)
            raw[g * G // pack: min((g + 1) * G, n + pack - 1) // pack] = rep
        buf = torch.full((raw.size + 2 * GUARD,), 0x5C, dtype=torch.uint8, device="cuda")
        buf[GUARD: GUARD + raw.size] = torch.from_numpy(raw).cuda()
        out.append((buf, torch.from_numpy(s).cuda(), torch.from_numpy(z).cuda()))
    return out


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_edge_terms(ctx, dt, qd):
    """-0.0 and NaN in term 0 under SET (a row initialised to +0.0 would lose both), and ADD onto an out holding NaN, +-inf, -0.0 and values on
    which a term of 2^-8 makes a bfloat16 tie."""
    fdt = FDT[dt]
    for G in (32, 128):
        n = 3 * tile_elems(dt, qd, G) + G + 5
        for k in (1, 3):
            terms = edge_terms(n, qd, G, k, 5 + G + k)
            got = fused(terms, None, "set", fdt, qd, G, n)
            want = composition(terms, None, "set", fdt, qd, G, n)
            same(got, want, f"SET G={G} k={k}")
            if k == 1:
                neg0 = _ibits(want) == (-32768 if dt == O.BF16 else -(1 << 31))
                assert bool(torch.isnan(want).any()), "the edge terms must put NaN into term 0"
                # (q - zp) * scale gives -0.0 for q == zp and a negative scale; the fma form of uint4 / uint2 -> bfloat16 gives q s + (-zp s) = +0.0
                assert bool(neg0.any()) or (dt == O.BF16 and qd != O.UINT8), "the edge terms must put -0.0 into term 0"
            init = _rand(n, fdt, 17).float()
            init[0::7] = float("nan")
            init[1::7] = float("inf")
            init[2::7] = float("-inf")
            init[3::7] = -0.0
            init[4::7] = 1.0              # + 2^-8: a tie that rounds to even, down
            init[5::7] = 1.0078125        # + 2^-8: a tie that rounds to even, up
            init = init.to(fdt)
            same(fused(terms, init, "add", fdt, qd, G, n), composition(terms, init, "add", fdt, qd, G, n), f"ADD G={G} k={k}")


@pytest.mark.parametrize("dt,qd", [(O.F32, O.UINT8), (O.BF16, O.UINT4), (O.F32, O.UINT2)])
def test_set_does_not_read_out(ctx, dt, qd):
    """SET gives the same bytes whether out held NaNs or zeros (the guard bands are checked inside fused())."""
    G, fdt = 128, FDT[dt]
    for n in (G - 1, 3 * tile_elems(dt, qd, G) + G + 5):
        terms = make_terms(n, fdt, qd, G, 7, 60 + qd)
        a = fused(terms, None, "set", fdt, qd, G, n, fill=float("nan"))
        b = fused(terms, None, "set", fdt, qd, G, n, fill=0.0)
        assert torch.equal(_ibits(a), _ibits(b))


def test_misaligned_buffers_give_the_same_bytes(ctx):
    """out one element into its allocation (x[1:]) and a term one byte into its own: the composition through the guarded kernel, the same bytes."""
    G = 128
    for dt, qd in PAIRS:
        fdt = FDT[dt]
        n = 3 * tile_elems(dt, qd, G) + G + 5
        terms = make_terms(n, fdt, qd, G, 3, 70 + qd)
        init = _rand(n, fdt, 3)
        for op in ("set", "add"):
            start = init if op == "add" else None
            want = fused(terms, start, op, fdt, qd, G, n)
            # a misaligned out
            import piquant.torch as pt

            base = torch.full((n + 9,), -7.0, dtype=fdt, device="cuda")
            out = base[1: 1 + n]
            assert out.data_ptr() % 16 != 0
            if start is not None:
                out.copy_(start)
            pt.dequantize_sum_grouped([raw_of(t) for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=fdt, group_size=G, reduce_op=op, out=out,
                                      quant_dtype=QDT[qd], shape=(n,))
            torch.cuda.synchronize()
            assert float(base[0]) == -7.0 and bool((base[1 + n:] == -7.0).all())
            same(out, want, f"misaligned out, {op}")
            # a misaligned term
            raw = raw_of(terms[1])
            shifted = torch.full((raw.numel() + 2 * GUARD + 1,), 0x5C, dtype=torch.uint8, device="cuda")[1:]   # the guarded buffer, one byte in
            shifted[GUARD: GUARD + raw.numel()] = raw
            odd = [terms[0], (shifted, terms[1][1], terms[1][2]), terms[2]]
            assert raw_of(odd[1]).data_ptr() % 16 != 0 and torch.equal(raw_of(odd[1]), raw)
            same(fused(odd, start, op, fdt, qd, G, n), want, f"misaligned term, {op}")


def test_non_default_stream(ctx):
    G, n, fdt, qd = 128, 1 << 20, torch.float32, O.UINT8
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        init = torch.empty(n, device="cuda")
        init.normal_()
        init.mul_(3.0).add_(1.0)   # still in flight when the fused call is enqueued behind it on the same stream
        terms = make_terms(n, fdt, qd, G, 7, 11)
        got = fused(terms, init, "add", fdt, qd, G, n)
        want = composition(terms, init, "add", fdt, qd, G, n)
    side.synchronize()
    same(got, want)


def test_graph_capture_replay(ctx):
    """Captured once, replayed twice: ADD accumulates the terms twice."""
    import piquant.torch as pt

    G, n, fdt, qd = 128, 100_003, torch.float32, O.UINT4
    terms = make_terms(n, fdt, qd, G, 3, 21)
    args = ([raw_of(t) for t in terms], [t[1] for t in terms], [t[2] for t in terms])
    kw = dict(dtype=fdt, group_size=G, quant_dtype=QDT[qd], shape=(n,))
    start = _rand(n, fdt, 2)
    want = composition(terms, composition(terms, start, "add", fdt, qd, G, n), "add", fdt, qd, G, n)
    out = start.clone()
    pt.dequantize_sum_grouped(*args, reduce_op="add", out=out, **kw)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pt.dequantize_sum_grouped(*args, reduce_op="add", out=out, **kw)
    out.copy_(start)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    same(out, want)


def test_the_wrapper_and_the_ptr_entry_agree(ctx):
    G = 128
    for dt, qd in ((O.F32, O.UINT8), (O.BF16, O.UINT2)):
        fdt = FDT[dt]
        n = 3 * tile_elems(dt, qd, G) + G + 5
        terms = make_terms(n, fdt, qd, G, 17, 40 + qd)
        init = _rand(n, fdt, 8)
        for op in ("set", "add"):
            start = init if op == "add" else None
            a = fused(terms, start, op, fdt, qd, G, n, via="torch")
            b = fused(terms, start, op, fdt, qd, G, n, via="ptr", c=ctx)
            assert torch.equal(_ibits(a), _ibits(b)), op
    # the wrapper allocates for SET and returns what it wrote into
    t = make_terms(1000, torch.float32, O.UINT8, G, 2, 1)
    import piquant.torch as pt

    r = pt.dequantize_sum_grouped([raw_of(x) for x in t], [x[1] for x in t], [x[2] for x in t], dtype=torch.float32, group_size=G)
    same(r, composition(t, None, "set", torch.float32, O.UINT8, G, 1000))
