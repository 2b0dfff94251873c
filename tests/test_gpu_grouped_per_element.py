"""The global element index of every grouped kernel on the MI355X, pinned by per-element stochastic thresholds (RM_STOCH_ELEM).

In per-element mode the rounding of element i depends on index_base + i, and each kernel family computes that index in its own way: the streaming
tile from its vector and row, the guarded kernels from the group's base, a batch member relative to its own tensor.  Every entry point is compared
bit for bit with the model of tests/per_element_model.py -- the oracle's quantize_per_element group by group, and nothing of the library -- on
the inputs of tests/per_element_cases.py, of which tests/test_per_element_model_cpu.py proves that one wrong bit of the index, in any of eleven
ways, changes the bytes.  The bases put index 2^32 inside a vector of a chunk's first row, of its last row, on a chunk boundary and into the
ragged last chunk; one base lies above 2^33 and runs with a seed whose upper half is not zero.  Guard bytes stand in front of and behind
everything a call writes, inputs must not be written, NaNs compare by position."""
import numpy as np
import pytest

import oracle as O
import per_element_cases as C
import per_element_model as M
from ef_model import widen

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


@pytest.fixture(autouse=True)
def restore_round_mode(ctx):
    yield
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)


class Dev:
    """A host array on the device with GUARD bytes of 0xAA in front of and behind it, the data `shift` bytes off a 16-byte boundary."""

    def __init__(self, a, shift=0):
        self.host = np.ascontiguousarray(a)
        raw = self.host.view(np.uint8).reshape(-1)
        self.shift, self.nbytes = shift, raw.size
        self.buf = torch.full((raw.size + shift + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD + shift: GUARD + shift + raw.size]
        if raw.size:
            self.view.copy_(torch.from_numpy(raw.copy()))
        assert self.buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
        self.ptr = self.buf.data_ptr() + GUARD + shift   # also for an empty array, whose view has no storage offset to speak of

    def guards_ok(self):
        return bool((self.buf[: GUARD + self.shift] == 0xAA).all()) and bool((self.buf[GUARD + self.shift + self.nbytes:] == 0xAA).all())

    def unwritten(self):
        return np.array_equal(self.view.cpu().numpy(), self.host.view(np.uint8).reshape(-1))

    def get(self, dtype=None):
        a = self.view.cpu().numpy()
        return a.view(self.host.dtype if dtype is None else dtype)


def fresh(nbytes, shift=0):
    return Dev(np.full(nbytes, 0xAA, dtype=np.uint8), shift)


def ready(ctx, seed, base):
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.set_stochastic_threshold(None)
    ctx.set_stochastic_per_element(True, seed=seed, index_base=base)


def check_buffers(written, read, what):
    torch.cuda.synchronize()
    for name, d in written.items():
        assert d.guards_ok(), f"{what}: wrote outside {name}"
    for name, d in read.items():
        assert d.guards_ok() and d.unwritten(), f"{what}: {name} was written"


def same_bytes(got, want, qd, what):
    assert got.size == want.size, what
    if not np.array_equal(got, want):
        n = got.size * (8 // M.BITS[qd])
        bad = np.flatnonzero(M.unpack(got, qd, n) != M.unpack(want, qd, n))
        raise AssertionError(f"{what}: {bad.size} codes differ, first at element {bad[0]}, last at element {bad[-1]}")


def same_params(s, z, ws, wz, what):
    bad = np.flatnonzero((s.view(np.uint32) != ws.view(np.uint32)) | (z != wz))
    assert bad.size == 0, f"{what}: parameters of {bad.size} groups differ, first group {bad[0]}: got ({s[bad[0]]!r}, {z[bad[0]]}) want ({ws[bad[0]]!r}, {wz[bad[0]]})"


def same_floats(got, want, dt, what):
    """bit for bit, NaNs by position; float32 arrays or bfloat16 bit patterns"""
    assert got.size == want.size and got.dtype == want.dtype, what
    with np.errstate(invalid="ignore"):
        gn, wn = np.isnan(widen(got, dt)), np.isnan(widen(want, dt))
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8]}"
    bits = np.uint16 if dt == O.BF16 else np.uint32
    bad = np.flatnonzero((got.view(bits) != want.view(bits)) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:8]}"


def quantizing_call(ctx, entry, x, dt, qd, G, seed, base, r=None, dt_r=None, terms=(), guarded=False, misaligned_term=None):
    """One call of quantize_grouped ("q"), quantize_grouped_ef ("ef"), reduce_quantize_grouped ("reduce") or reduce_quantize_grouped_ef ("reduce_ef")
    on guarded buffers -> (packed bytes, scales, zero points, new residual or None).  guarded: the residual (the tensor, where there is none) one
    element off a 16-byte boundary, which takes the element-by-element kernel.  misaligned_term: that term one byte off, which takes the two-step
    composition."""
    import piquant

    DT, mode = piquant.DataType, piquant.RoundMode.STOCHASTIC
    n = x.size
    ng, nbytes = (n + G - 1) // G, O.packed_numel(n, qd)
    xd = Dev(x, x.itemsize if guarded and r is None else 0)
    od, sd, zd = fresh(nbytes), fresh(4 * ng), fresh(ng)
    rd = None if r is None else Dev(r, r.itemsize if guarded else 0)
    td = [[Dev(a, 1 if i == misaligned_term and j == 0 else 0) for j, a in enumerate(t)] for i, t in enumerate(terms)]
    lists = [[t[j].ptr for t in td] for j in range(3)]
    rdt = None if r is None or dt_r == dt else DT(dt_r)
    ready(ctx, seed, base)
    if entry == "q":
        ctx.quantize_grouped_ptr(xd.ptr, DT(dt), od.ptr, DT(qd), n, G, sd.ptr, zd.ptr, False, mode, _device_ptrs=True)
    elif entry == "ef":
        ctx.quantize_grouped_ef_ptr(xd.ptr, DT(dt), rd.ptr, od.ptr, DT(qd), n, G, sd.ptr, zd.ptr, mode, _device_ptrs=True, residual_dtype=rdt)
    elif entry == "reduce":
        ctx.reduce_quantize_grouped_ptr(xd.ptr, DT(dt), lists[0], lists[1], lists[2], od.ptr, DT(qd), n, G, sd.ptr, zd.ptr, mode, _device_ptrs=True)
    else:
        ctx.reduce_quantize_grouped_ef_ptr(xd.ptr, DT(dt), rd.ptr, lists[0], lists[1], lists[2], od.ptr, DT(qd), n, G, sd.ptr, zd.ptr, mode, _device_ptrs=True,
                                           residual_dtype=rdt)
    written = {"out": od, "scales": sd, "zero_points": zd}
    if rd is not None:
        written["the residual"] = rd
    read = {f"term {i}": d for i, t in enumerate(td) for d in t}
    if entry in ("q", "ef"):
        read["the input"] = xd
    else:
        written["acc"] = xd   # unspecified afterwards, but not a byte outside it
    check_buffers(written, read, entry)
    return od.get(), sd.get(np.float32), zd.get(), None if rd is None else rd.get()


def compare(got, want, qd, dt_r, what):
    same_params(got[1], got[2], want[1], want[2], what)
    same_bytes(got[0], want[0], qd, what)
    if len(want) > 3:
        same_floats(got[3], want[3], dt_r, what + ", residual")


# ---- 0. quantize_grouped itself, on these inputs (tests/test_gpu_grouped_step_edges.py pins it on the rounding edges, with one base)

@pytest.mark.parametrize("dt,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.SOME_G)
def test_quantize_grouped(ctx, dt, qd, G):
    x = C.single(dt, qd, G)[0]
    for name, base, seed in C.bases(M.tile(dt, qd, G)):
        want = M.quantize(x, dt, qd, G, seed, base)
        for guarded in (False, True):
            compare(quantizing_call(ctx, "q", x, dt, qd, G, seed, base, guarded=guarded), want, qd, None, f"base {name!r} guarded={guarded}")


# ---- 1. error feedback

@pytest.mark.parametrize("dt,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.GROUP_SIZES)
def test_quantize_grouped_ef_same_type(ctx, dt, qd, G):
    x, r, _ = C.ef_inputs("same", dt, qd, G)
    for name, base, seed in C.bases(M.tile(dt, qd, G)):
        want = M.ef_step(x, r, dt, qd, G, seed, base)
        for guarded in (False, True):
            compare(quantizing_call(ctx, "ef", x, dt, qd, G, seed, base, r, dt, guarded=guarded), want, qd, dt, f"base {name!r} guarded={guarded}")


@pytest.mark.parametrize("qd", C.QDS)
@pytest.mark.parametrize("G", C.GROUP_SIZES)
def test_quantize_grouped_ef_float32_residual(ctx, qd, G):
    x, r, dt_tile = C.ef_inputs("mixed", O.BF16, qd, G)
    for name, base, seed in C.bases(M.tile(dt_tile, qd, G)):
        want = M.ef_f32r_step(x, r, qd, G, seed, base)
        for guarded in (False, True):
            compare(quantizing_call(ctx, "ef", x, O.BF16, qd, G, seed, base, r, O.F32, guarded=guarded), want, qd, O.F32, f"base {name!r} guarded={guarded}")


# ---- 2. the fused reduce: 17 terms take the surplus path (one grouped dequantize ADD, then 16 fused); a misaligned term takes the composition

@pytest.mark.parametrize("dt,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.SOME_G)
def test_reduce_quantize_grouped(ctx, dt, qd, G):
    x = C.single(dt, qd, G)[0]
    for k in C.REDUCE_TERMS:
        terms = C.terms_for(dt, qd, G, k)
        acc = M.add_terms(x, terms, dt, qd, G)
        for name, base, seed in C.bases(M.tile(dt, qd, G)):
            want = M.quantize(acc, dt, qd, G, seed, base)
            compare(quantizing_call(ctx, "reduce", x, dt, qd, G, seed, base, terms=terms), want, qd, None, f"{k} terms, base {name!r}")
            if k == 7:
                compare(quantizing_call(ctx, "reduce", x, dt, qd, G, seed, base, terms=terms, misaligned_term=3), want, qd, None,
                        f"{k} terms, term 3 misaligned, base {name!r}")


@pytest.mark.parametrize("dt,qd", C.PAIRS + [("mixed", q) for q in C.QDS])
@pytest.mark.parametrize("G", C.SOME_G)
def test_reduce_quantize_grouped_ef(ctx, dt, qd, G):
    kind, dt = ("mixed", O.BF16) if dt == "mixed" else ("same", dt)
    x, r, dt_tile = C.ef_inputs(kind, dt, qd, G)
    dt_r = dt if kind == "same" else O.F32
    for k in C.REDUCE_EF_TERMS:
        terms = C.terms_for(dt, qd, G, k, None if kind == "same" else O.F32)
        for name, base, seed in C.bases(M.tile(dt_tile, qd, G)):
            want = M.reduce_ef(x, r, terms, dt, qd, G, seed, base) if kind == "same" else M.reduce_ef_f32r_per_element_model(x, r, terms, qd, G, seed, base)
            compare(quantizing_call(ctx, "reduce_ef", x, dt, qd, G, seed, base, r, dt_r, terms), want, qd, dt_r, f"{kind} {k} terms, base {name!r}")


# ---- 3. quantize-dequantize

def requant_call(ctx, x, dt, qd, G, seed, base, prev=None, given=None, params=True, in_place=False, guarded=False):
    """One quantize_dequantize_grouped call on guarded buffers -> (out, scales, zero points); prev: ADD onto it; in_place: out is in."""
    import piquant

    n = x.size
    ng = (n + G - 1) // G
    shift = x.itemsize if guarded else 0
    xd = Dev(x, shift)
    od = xd if in_place else (Dev(prev, shift) if prev is not None else Dev(np.full(n * x.itemsize, 0xAA, dtype=np.uint8).view(x.dtype), shift))
    sd = Dev(given[0]) if given else fresh(4 * ng)
    zd = Dev(given[1]) if given else fresh(ng)
    ready(ctx, seed, base)
    ctx.quantize_dequantize_grouped_ptr(xd.ptr, piquant.DataType(dt), od.ptr, piquant.DataType(qd), n, G, sd.ptr if params else 0, zd.ptr if params else 0,
                                        given is not None, piquant.RoundMode.STOCHASTIC, piquant.ReduceOp.ADD if prev is not None else piquant.ReduceOp.SET,
                                        _device_ptrs=True)
    untouched = {} if in_place else {"the input": xd}
    if given or not params:
        untouched.update({"scales": sd, "zero_points": zd})
    check_buffers({"out": od, "scales": sd, "zero_points": zd}, untouched, "quantize_dequantize_grouped")
    return od.get(x.dtype), sd.get(np.float32), zd.get()


@pytest.mark.parametrize("dt,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.GROUP_SIZES)
def test_quantize_dequantize_grouped(ctx, dt, qd, G):
    x, prev, _ = C.single(dt, qd, G)
    given = C.given_params(dt, qd, G)
    for name, base, seed in C.bases(M.tile(dt, qd, G)):
        w_set, ws, wz = M.quantize_dequantize(x, dt, qd, G, seed, base)
        w_add = M.quantize_dequantize(x, dt, qd, G, seed, base, prev=prev)[0]
        g_set = M.quantize_dequantize(x, dt, qd, G, seed, base, params=given)[0]
        g_add = M.quantize_dequantize(x, dt, qd, G, seed, base, params=given, prev=prev)[0]
        for guarded in (False, True):
            what = f"base {name!r} guarded={guarded}"
            d, s, z = requant_call(ctx, x, dt, qd, G, seed, base, guarded=guarded)
            same_params(s, z, ws, wz, what)
            same_floats(d, w_set, dt, what + " SET")
            d, s, z = requant_call(ctx, x, dt, qd, G, seed, base, prev=prev, guarded=guarded)
            same_params(s, z, ws, wz, what)
            same_floats(d, w_add, dt, what + " ADD")
            same_floats(requant_call(ctx, x, dt, qd, G, seed, base, given=given, guarded=guarded)[0], g_set, dt, what + " SET, given parameters")
            same_floats(requant_call(ctx, x, dt, qd, G, seed, base, given=given, prev=prev, guarded=guarded)[0], g_add, dt, what + " ADD, given parameters")
            same_floats(requant_call(ctx, x, dt, qd, G, seed, base, params=False, guarded=guarded)[0], w_set, dt, what + " SET, no parameter arrays")
            same_floats(requant_call(ctx, x, dt, qd, G, seed, base, prev=prev, params=False, guarded=guarded)[0], w_add, dt, what + " ADD, no parameter arrays")
            same_floats(requant_call(ctx, x, dt, qd, G, seed, base, in_place=True, guarded=guarded)[0], w_set, dt, what + " SET in place")


# ---- 4. the batches: 19 members, two launches and a member that runs alone; every member indexes its own elements from index_base + 0

def batch_buffers(members, dt, qd, G, kind=None):
    """-> per member (x, residual or None, out, scales, zero points) on the device; member 7 one element off a 16-byte boundary"""
    devs = []
    for i, (x, a) in enumerate(members):
        shift = x.itemsize if i == C.MISALIGNED_MEMBER else 0
        ng = (x.size + G - 1) // G
        r = None if kind is None else Dev(C.residual_from(a, dt, kind))
        devs.append((Dev(x, shift), r, fresh(O.packed_numel(x.size, qd)), fresh(4 * ng), fresh(ng)))
    assert devs[C.MISALIGNED_MEMBER][0].ptr % 16 != 0
    return devs


@pytest.mark.parametrize("dt,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.SOME_G)
def test_quantize_grouped_batch(ctx, dt, qd, G):
    import piquant

    members = C.batch_inputs(dt, qd, G)
    for name, base, seed in C.bases(M.tile(dt, qd, G)):
        devs = batch_buffers(members, dt, qd, G)
        ready(ctx, seed, base)
        ctx.quantize_grouped_batch_ptr([d[0].ptr for d in devs], piquant.DataType(dt), [d[2].ptr for d in devs], piquant.DataType(qd), [x.size for x, _ in members],
                                       G, [d[3].ptr for d in devs], [d[4].ptr for d in devs], False, piquant.RoundMode.STOCHASTIC, _device_ptrs=True)
        for i, ((x, _), (xd, _, od, sd, zd)) in enumerate(zip(members, devs)):
            what = f"base {name!r} member {i} ({x.size} elements)"
            check_buffers({"out": od, "scales": sd, "zero_points": zd}, {"the input": xd}, what)
            compare((od.get(), sd.get(np.float32), zd.get()), M.quantize(x, dt, qd, G, seed, base), qd, None, what)


@pytest.mark.parametrize("dt,qd", C.PAIRS + [("mixed", q) for q in C.QDS])
@pytest.mark.parametrize("G", C.SOME_G)
def test_quantize_grouped_ef_batch(ctx, dt, qd, G):
    import piquant

    kind, dt = ("mixed", O.BF16) if dt == "mixed" else ("same", dt)
    dt_r = dt if kind == "same" else O.F32
    members = C.batch_inputs(dt, qd, G, None if kind == "same" else O.F32)
    for name, base, seed in C.bases(M.tile(dt_r if kind == "mixed" else dt, qd, G)):
        devs = batch_buffers(members, dt, qd, G, kind)
        ready(ctx, seed, base)
        ctx.quantize_grouped_ef_batch_ptr([d[0].ptr for d in devs], piquant.DataType(dt), [d[1].ptr for d in devs], [d[2].ptr for d in devs], piquant.DataType(qd),
                                          [x.size for x, _ in members], G, [d[3].ptr for d in devs], [d[4].ptr for d in devs], piquant.RoundMode.STOCHASTIC,
                                          _device_ptrs=True, residual_dtype=None if kind == "same" else piquant.DataType(O.F32))
        for i, ((x, a), (xd, rd, od, sd, zd)) in enumerate(zip(members, devs)):
            what = f"{kind} base {name!r} member {i} ({x.size} elements)"
            check_buffers({"out": od, "scales": sd, "zero_points": zd, "the residual": rd}, {"the input": xd}, what)
            r = C.residual_from(a, dt, kind)
            want = M.ef_step(x, r, dt, qd, G, seed, base) if kind == "same" else M.ef_f32r_step(x, r, qd, G, seed, base)
            compare((od.get(), sd.get(np.float32), zd.get(), rd.get()), want, qd, dt_r, what)


@pytest.mark.parametrize("dt,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.SOME_G)
def test_quantize_dequantize_grouped_batch(ctx, dt, qd, G):
    """SET into fresh outputs with the parameters written, then ADD in place (out is in) with no parameter arrays"""
    import piquant

    members = C.batch_inputs(dt, qd, G)
    numels = [x.size for x, _ in members]
    DT, mode = piquant.DataType, piquant.RoundMode.STOCHASTIC
    for name, base, seed in C.bases(M.tile(dt, qd, G)):
        xs = [Dev(x, x.itemsize if i == C.MISALIGNED_MEMBER else 0) for i, (x, _) in enumerate(members)]
        outs = [Dev(np.full(x.nbytes, 0xAA, dtype=np.uint8).view(x.dtype), x.itemsize if i == C.MISALIGNED_MEMBER else 0) for i, (x, _) in enumerate(members)]
        sds = [fresh(4 * ((n + G - 1) // G)) for n in numels]
        zds = [fresh((n + G - 1) // G) for n in numels]
        ready(ctx, seed, base)
        ctx.quantize_dequantize_grouped_batch_ptr([d.ptr for d in xs], DT(dt), [d.ptr for d in outs], DT(qd), numels, G, [d.ptr for d in sds], [d.ptr for d in zds],
                                                  False, mode, piquant.ReduceOp.SET, _device_ptrs=True)
        wants = [M.quantize_dequantize(x, dt, qd, G, seed, base) for x, _ in members]
        for i, (w, xd, od, sd, zd) in enumerate(zip(wants, xs, outs, sds, zds)):
            what = f"base {name!r} member {i} ({numels[i]} elements)"
            check_buffers({"out": od, "scales": sd, "zero_points": zd}, {"the input": xd}, what)
            same_params(sd.get(np.float32), zd.get(), w[1], w[2], what)
            same_floats(od.get(members[i][0].dtype), w[0], dt, what + " SET")
        ctx.quantize_dequantize_grouped_batch_ptr([d.ptr for d in xs], DT(dt), [d.ptr for d in xs], DT(qd), numels, G, None, None, False, mode,
                                                  piquant.ReduceOp.ADD, _device_ptrs=True)
        for i, ((x, _), xd) in enumerate(zip(members, xs)):
            what = f"base {name!r} member {i} ({numels[i]} elements) ADD in place"
            check_buffers({"out": xd}, {}, what)
            same_floats(xd.get(x.dtype), M.quantize_dequantize(x, dt, qd, G, seed, base, prev=x)[0], dt, what)


# ---- 5. graph capture: the seed and the base of a captured call are those the context held at capture

def test_graph_capture_keeps_the_captured_base(ctx):
    import piquant.torch as pt

    dt, qd, G = C.CAPTURE
    t = M.tile(dt, qd, G)
    (_, base_a, seed), (_, base_b, _) = C.bases(t)[0], C.bases(t)[4]
    x0, a0, n = C.single(dt, qd, G)
    x1, r1 = C.capture_replay_inputs()

    def device(a):
        return torch.from_numpy(a.view(np.int16).copy()).cuda().view(torch.bfloat16)

    x, r = device(x0), device(C.residual_from(a0, dt, "same"))
    ctx.set_stochastic_per_element(True, seed=seed, index_base=base_a)
    pt.quantize_grouped(x, dtype=QDT[qd], group_size=G, round_mode="stochastic")   # eager warm-up (code objects)
    pt.quantize_grouped_ef(x, r.clone(), dtype=QDT[qd], group_size=G, round_mode="stochastic")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q, s, z = pt.quantize_grouped(x, dtype=QDT[qd], group_size=G, round_mode="stochastic")
        eq, es, ez = pt.quantize_grouped_ef(x, r, dtype=QDT[qd], group_size=G, round_mode="stochastic")
    ctx.set_stochastic_per_element(True, seed=seed ^ 0x5555, index_base=base_b)
    x.copy_(device(x1))
    r.copy_(device(r1))
    graph.replay()
    torch.cuda.synchronize()
    compare((pt.packed_bytes(q).cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()), M.quantize(x1, dt, qd, G, seed, base_a), qd, None, "captured quantize_grouped")
    compare((pt.packed_bytes(eq).cpu().numpy(), es.cpu().numpy(), ez.cpu().numpy(), r.view(torch.int16).cpu().numpy().view(np.uint16)),
            M.ef_step(x1, r1, dt, qd, G, seed, base_a), qd, dt, "captured quantize_grouped_ef")
    assert not np.array_equal(M.quantize(x1, dt, qd, G, seed, base_a)[0], M.quantize(x1, dt, qd, G, seed ^ 0x5555, base_b)[0])
