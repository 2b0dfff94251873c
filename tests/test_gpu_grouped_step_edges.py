"""Every group size and the rounding edges of the grouped kernels on the MI355X, bit for bit against the CPU models.

with_group_size (csrc/grouped_dispatch.hpp) instantiates every grouped kernel for eight group sizes, each its own tile; grouped_quantize_chunk
(csrc/grouped_kernels.hpp) picks the short or the long rounding step per wave, and misaligned buffers take a third, scalar step.  The inputs
(tests/grouped_edge_cases.py; tests/test_grouped_step_edges_cpu.py asserts what they hold) put the same groups -- ties, ranges far from zero,
NaNs, denormals, +-0 -- through all three: section S takes the short step, L and T the long one.  Every comparison is exact; canaries sit in front
of and behind every buffer a call writes, and inputs must not be written."""
import functools

import numpy as np
import pytest

import grouped_edge_cases as E
import oracle as O
from ef_f32r_model import ef_f32r_step
from ef_model import ef_step
from grouped_edge_cases import unpack
from grouped_model import PACK, QMAX, dequantize_grouped, group_params_all, quantize_grouped
from grouped_reduce_ef_sim import reduce_ef_step

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
QDS = [O.UINT8, O.UINT4, O.UINT2]
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
GROUP_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
TAUS = (0.0, 0.25, 0.375, 0.37499997, 0.5, 0.99999994)
EF_KINDS = ("f32", "bf16", "mixed")   # tensor and residual float32; both bfloat16; a bfloat16 tensor with a float32 residual
GUARD = 64
ELEM_SEED, INDEX_BASE = 0x1234_5678_9ABC, 2 ** 32 - 5000


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


def _dev(a: np.ndarray, shift=0):
    """numpy array -> device uint8 buffer with GUARD bytes of 0xAA in front of and behind the data, the data `shift` bytes off a 16-byte boundary;
    -> (buffer, view of the data)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((raw.size + shift + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    view = buf[GUARD + shift: GUARD + shift + raw.size]
    if raw.size:
        view.copy_(torch.from_numpy(raw.copy()))
    assert raw.size == 0 or view.data_ptr() % 16 == shift
    return buf, view


def _guard_ok(buf, n, shift=0):
    return bool((buf[:GUARD + shift] == 0xAA).all()) and bool((buf[GUARD + shift + n:] == 0xAA).all())


def _unwritten(view, a):
    return np.array_equal(view.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def as_input(bits, dt):
    return bits.view(np.float32) if dt == O.F32 else bits


@functools.lru_cache(maxsize=None)
def edge_case(dt_in, qd, G, seed=0):
    """-> (input bits, layout, scales, zero points of the model); computed once and shared, read-only"""
    bits, lay = E.edge_tensor(dt_in, qd, G, seed)
    s, z = group_params_all(E.values(bits), G, qd)
    for a in (bits, s, z):
        a.setflags(write=False)
    return bits, lay, s, z


@functools.lru_cache(maxsize=None)
def model_bytes(dt_in, qd, G, mode, tau, seed=0):
    bits, _, s, z = edge_case(dt_in, qd, G, seed)
    q = quantize_grouped(as_input(bits, dt_in), dt_in, qd, G, mode, tau or 0.0, params=(s, z))[0]
    q.setflags(write=False)
    return q


def assert_params(s, z, ws, wz, lay, what):
    bad = np.flatnonzero((s.view(np.uint32) != ws.view(np.uint32)) | (z != wz))
    assert bad.size == 0, (f"{what}: parameters of {bad.size} groups differ, first {lay.describe(bad[0])}: got ({s[bad[0]]!r}, {z[bad[0]]}) "
                           f"want ({ws[bad[0]]!r}, {wz[bad[0]]})")


def assert_bytes(q, want, lay, qd, what):
    assert q.size == want.size
    if not np.array_equal(q, want):
        got_c, want_c = unpack(q, qd, lay.n), unpack(want, qd, lay.n)
        bad = np.flatnonzero(got_c != want_c)
        assert bad.size, f"{what}: bits behind the tensor's end differ in the last byte: got {q[-1]:#x} want {want[-1]:#x}"
        raise AssertionError(f"{what}: {bad.size} codes differ, first {lay.describe_element(bad[0])}: got {got_c[bad[0]]} want {want_c[bad[0]]}")


def assert_steps_agree(q, s, z, lay, qd, what):
    """groups of L and T that repeat a group of S bit for bit (and got its parameters) must get its codes: S takes the short step, L and T the long"""
    codes = unpack(q, qd, lay.n)
    for g in list(lay.groups_of("L")) + list(lay.groups_of("T")):
        o = lay.origin[g]
        if o < 0 or s[g].view(np.uint32) != s[o].view(np.uint32) or z[g] != z[o]:
            continue
        b, e = lay.bounds(g)
        bad = np.flatnonzero(codes[b:e] != codes[o * lay.G: o * lay.G + e - b])
        assert bad.size == 0, (f"{what}: short and long step disagree: {lay.describe(g)} repeats {lay.describe(o)}, {bad.size} codes differ, "
                               f"first at + {bad[0]}: {codes[b + bad[0]]} against {codes[o * lay.G + bad[0]]}")


def assert_residual(got, want, lay, what):
    """bit for bit, NaNs by position; float32 arrays or bfloat16 bit patterns"""
    gf, wf = E.values(got.view(np.uint32 if got.dtype == np.float32 else np.uint16)), E.values(want.view(np.uint32 if want.dtype == np.float32 else np.uint16))
    gn, wn = np.isnan(gf), np.isnan(wf)
    bad = np.flatnonzero(gn != wn)
    assert bad.size == 0, f"{what}: NaN positions of the residual differ, first {lay.describe_element(bad[0])}"
    bad = np.flatnonzero((gf.view(np.uint32) != wf.view(np.uint32)) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} residual elements differ, first {lay.describe_element(bad[0])}: got {gf[bad[0]]!r} want {wf[bad[0]]!r}"


def run_quantize(ctx, bits, dt_in, qd, G, mode, given=None, misaligned=False):
    """One quantize_grouped call on guarded buffers -> (packed bytes, scales, zero points).  misaligned: x one element and out one byte off a
    16-byte boundary -- the guarded scalar kernel."""
    import piquant

    n = bits.size
    ng, nbytes = (n + G - 1) // G, O.packed_numel(n, qd)
    sx, so = (bits.itemsize, 1) if misaligned else (0, 0)
    xbuf, xin = _dev(bits, sx)
    obuf, oin = _dev(np.full(nbytes, 0xAA, dtype=np.uint8), so)
    sbuf, sin = _dev(np.zeros(ng, dtype=np.float32) if given is None else given[0])
    zbuf, zin = _dev(np.zeros(ng, dtype=np.uint8) if given is None else given[1])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_ptr(xin.data_ptr(), piquant.DataType(dt_in), oin.data_ptr(), piquant.DataType(qd), n, G, sin.data_ptr(), zin.data_ptr(),
                             given is not None, piquant.RoundMode(mode), _device_ptrs=True)
    torch.cuda.synchronize()
    assert _guard_ok(obuf, nbytes, so), "wrote outside out"
    assert _guard_ok(sbuf, 4 * ng), "wrote outside scales"
    assert _guard_ok(zbuf, ng), "wrote outside zero_points"
    assert _guard_ok(xbuf, bits.nbytes, sx) and _unwritten(xin, bits), "the input was written"
    if given is not None:
        assert _unwritten(sin, given[0]) and _unwritten(zin, given[1]), "given parameters must not be written"
    return oin.cpu().numpy(), sin.cpu().numpy().view(np.float32), zin.cpu().numpy()


# ---- 1. quantize_grouped with computed parameters: the three steps against the model and against one another

@pytest.mark.parametrize("dt_in,qd", PAIRS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_quantize_on_the_edges(ctx, dt_in, qd, G):
    bits, lay, ws, wz = edge_case(dt_in, qd, G)
    try:
        for mode, tau in [(O.NEAREST, None)] + [(O.STOCHASTIC, t) for t in TAUS]:
            what = f"dt_in={dt_in} qd={qd} G={G} mode={mode} tau={tau!r}"
            ctx.set_stochastic_threshold(tau)
            q, s, z = run_quantize(ctx, bits, dt_in, qd, G, mode)
            assert_params(s, z, ws, wz, lay, what)
            assert_bytes(q, model_bytes(dt_in, qd, G, mode, tau), lay, qd, what)
            assert_steps_agree(q, s, z, lay, qd, what)
            if tau in (None, 0.375):
                mq, ms, mz = run_quantize(ctx, bits, dt_in, qd, G, mode, misaligned=True)
                assert_params(ms, mz, s, z, lay, what + ", scalar kernel against streaming kernel")
                assert_bytes(mq, q, lay, qd, what + ", scalar kernel against streaming kernel")
        # per-element thresholds: the element's global index is index_base + its position, and it crosses 2^32 inside the tensor
        assert INDEX_BASE < 2 ** 32 < INDEX_BASE + lay.n
        x = as_input(bits, dt_in)
        want = np.concatenate([O.quantize_per_element(x[b:e], dt_in, qd, float(ws[g]), int(wz[g]), ELEM_SEED, INDEX_BASE + b)
                               for g in range(ws.size) for b, e in [lay.bounds(g)]])
        ctx.set_stochastic_threshold(None)
        for misaligned in (False, True):
            what = f"dt_in={dt_in} qd={qd} G={G} per-element thresholds" + (", scalar kernel" if misaligned else "")
            ctx.set_stochastic_per_element(True, seed=ELEM_SEED, index_base=INDEX_BASE)
            q, s, z = run_quantize(ctx, bits, dt_in, qd, G, O.STOCHASTIC, misaligned=misaligned)
            assert_params(s, z, ws, wz, lay, what)
            assert_bytes(q, want, lay, qd, what)
    finally:
        ctx.set_stochastic_per_element(False)
        ctx.set_stochastic_threshold(None)


# ---- 2. given parameters

def odd_scales(ng, qd, seed):
    """one scale per group from: 0, -0, +-inf, NaN, a negative number, a denormal, 2^127 (its reciprocal is denormal), and two ordinary ones"""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -2.5, 1.0e-40, 2.0 ** 127, 0.37, 1.0], dtype=np.float32)
    scales = pool[np.arange(ng) % pool.size][rng.permutation(ng)]
    return scales, rng.choice(np.array([0, QMAX[qd]], dtype=np.uint8), ng)


@pytest.mark.parametrize("dt_in,qd", PAIRS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_given_parameters(ctx, dt_in, qd, G):
    bits, lay, ws, wz = edge_case(dt_in, qd, G)
    x = as_input(bits, dt_in)
    scales, zps = odd_scales(ws.size, qd, G + qd)
    assert ws.size >= 10
    try:
        for mode, tau in ((O.NEAREST, None), (O.STOCHASTIC, 0.375)):
            what = f"dt_in={dt_in} qd={qd} G={G} mode={mode} tau={tau!r}"
            ctx.set_stochastic_threshold(tau)
            # the call's own parameters given back: the long step (given parameters always take it) against the short step of the computed call
            q, s, z = run_quantize(ctx, bits, dt_in, qd, G, mode)
            gq, _, _ = run_quantize(ctx, bits, dt_in, qd, G, mode, given=(s, z))
            assert_bytes(gq, q, lay, qd, what + ", own parameters given back")
            assert_bytes(gq, model_bytes(dt_in, qd, G, mode, tau), lay, qd, what + ", own parameters given back, against the model")
            gq, _, _ = run_quantize(ctx, bits, dt_in, qd, G, mode, given=(scales, zps))
            want = quantize_grouped(x, dt_in, qd, G, mode, tau or 0.0, params=(scales, zps))[0]
            if not np.array_equal(gq, want):
                bad = np.flatnonzero(unpack(gq, qd, lay.n) != unpack(want, qd, lay.n))
                g = bad[0] // G
                raise AssertionError(f"{what}: {bad.size} codes differ, first {lay.describe_element(bad[0])} with the given ({scales[g]!r}, {zps[g]})")
    finally:
        ctx.set_stochastic_threshold(None)


# ---- 4. error feedback: x and r chosen so that y = x + r is the edge tensor exactly

@functools.lru_cache(maxsize=None)
def ef_inputs(kind, qd, G, seed=0):
    """-> (x, its dtype code, r, its dtype code, layout); f32 arrays are float32, bf16 ones bit patterns.  For a float32 y: x = the edge tensor rounded to
    bfloat16 (and widened for "f32"), r = edge - x, which is exact; for "bf16": the bfloat16 edge tensor and r = 0."""
    if kind == "bf16":
        bits, lay, _, _ = edge_case(O.BF16, qd, G, seed)
        out = (bits, O.BF16, np.zeros(bits.size, dtype=np.uint16), O.BF16, lay)
    else:
        bits, lay, _, _ = edge_case(O.F32, qd, G, seed)
        edge, xb = bits.view(np.float32), E.narrow_bits(bits)
        xw = E.values(xb)
        with np.errstate(invalid="ignore"):
            r = np.where(np.isfinite(edge), edge - xw, np.float32(0)).astype(np.float32)
            assert np.array_equal((xw + r)[np.isfinite(edge)], edge[np.isfinite(edge)])
        out = (xw, O.F32, r, O.F32, lay) if kind == "f32" else (xb, O.BF16, r, O.F32, lay)
    for a in out[:3:2]:
        a.setflags(write=False)
    return out


def model_ef(kind, x, r, terms, qd, G, mode, tau):
    """-> (packed bytes, scales, zero points, new residual) of tests/grouped_reduce_ef_sim.py / tests/ef_f32r_model.py"""
    if kind != "mixed":
        return reduce_ef_step(x, r, terms, O.F32 if kind == "f32" else O.BF16, qd, G, mode, tau)[:4]
    acc = x
    for q, s, z in terms:
        acc = dequantize_grouped(q, qd, O.BF16, acc.size, G, s, z, O.ADD, prev=acc)
    return ef_f32r_step(acc, r, qd, G, mode, tau)[:4]


def run_reduce(ctx, x, dt_x, r, dt_r, terms, qd, G, mode, reduce_entry):
    """One call on guarded buffers: quantize_grouped_ef (r given, no terms), reduce_quantize_grouped_ef (r given, reduce_entry) or
    reduce_quantize_grouped (r None) -> (packed bytes, scales, zero points, new residual or None)"""
    import piquant

    n = x.size
    ng, nbytes = (n + G - 1) // G, O.packed_numel(n, qd)
    xbuf, xin = _dev(x)
    obuf, oin = _dev(np.full(nbytes, 0xAA, dtype=np.uint8))
    sbuf, sin = _dev(np.zeros(ng, dtype=np.float32))
    zbuf, zin = _dev(np.zeros(ng, dtype=np.uint8))
    tdev = [[_dev(a) for a in t] for t in terms]
    ptrs = [[t[i][1].data_ptr() for t in tdev] for i in range(3)]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    DT, rm = piquant.DataType, piquant.RoundMode(mode)
    if r is None:
        ctx.reduce_quantize_grouped_ptr(xin.data_ptr(), DT(dt_x), ptrs[0], ptrs[1], ptrs[2], oin.data_ptr(), DT(qd), n, G, sin.data_ptr(), zin.data_ptr(), rm,
                                        _device_ptrs=True)
    else:
        rbuf, rin = _dev(r)
        rdt = DT(dt_r) if dt_r != dt_x else None
        if reduce_entry:
            ctx.reduce_quantize_grouped_ef_ptr(xin.data_ptr(), DT(dt_x), rin.data_ptr(), ptrs[0], ptrs[1], ptrs[2], oin.data_ptr(), DT(qd), n, G, sin.data_ptr(),
                                               zin.data_ptr(), rm, _device_ptrs=True, residual_dtype=rdt)
        else:
            ctx.quantize_grouped_ef_ptr(xin.data_ptr(), DT(dt_x), rin.data_ptr(), oin.data_ptr(), DT(qd), n, G, sin.data_ptr(), zin.data_ptr(), rm,
                                        _device_ptrs=True, residual_dtype=rdt)
    torch.cuda.synchronize()
    assert _guard_ok(obuf, nbytes), "wrote outside out"
    assert _guard_ok(sbuf, 4 * ng), "wrote outside scales"
    assert _guard_ok(zbuf, ng), "wrote outside zero_points"
    assert _guard_ok(xbuf, x.nbytes), "wrote outside the tensor"
    for t, host in zip(tdev, terms):
        for (buf, view), a in zip(t, host):
            assert _guard_ok(buf, a.nbytes) and _unwritten(view, a), "a term was written"
    rn = None
    if r is not None:
        assert _guard_ok(rbuf, r.nbytes), "wrote outside the residual"
        rn = rin.cpu().numpy().view(r.dtype)
    if not reduce_entry:
        assert _unwritten(xin, x), "the input was written"
    return oin.cpu().numpy(), sin.cpu().numpy().view(np.float32), zin.cpu().numpy(), rn


def check_ef(ctx, kind, qd, G, terms, mode, tau, reduce_entry, what):
    x, dt_x, r, dt_r, lay = ef_inputs(kind, qd, G)
    ctx.set_stochastic_threshold(tau)
    q, s, z, rn = run_reduce(ctx, x, dt_x, r, dt_r, terms, qd, G, mode, reduce_entry)
    wq, ws, wz, wr = model_ef(kind, x, r, terms, qd, G, mode, tau or 0.0)
    assert_params(s, z, ws, wz, lay, what)
    assert_bytes(q, wq, lay, qd, what)
    assert_residual(rn, wr, lay, what)
    return wr, ws


@pytest.mark.parametrize("kind", EF_KINDS)
@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_error_feedback_on_the_edges(ctx, kind, qd, G):
    try:
        for mode, tau in ((O.NEAREST, None), (O.STOCHASTIC, 0.375)):
            wr, ws = check_ef(ctx, kind, qd, G, (), mode, tau, False, f"{kind} qd={qd} G={G} mode={mode} tau={tau!r}")
            if mode == O.NEAREST and kind != "bf16":   # on a tie the residual is exactly half a step, the largest it can be
                lay = ef_inputs(kind, qd, G)[4]
                b, e = lay.sections["S"]
                assert (np.abs(wr[b:e]) == np.repeat(ws[: (e - b) // G], G) * np.float32(0.5)).any()
    finally:
        ctx.set_stochastic_threshold(None)


# ---- 5. the fused reduce, plain and with error feedback

def zero_terms(k, n, qd, G, seed):
    """k terms that add exactly zero: a power of two as scale, every code equal to the zero point"""
    rng = np.random.default_rng(seed)
    ng, per, bits = (n + G - 1) // G, PACK[qd], E.BITS[qd]
    terms = []
    for _ in range(k):
        zps = rng.integers(0, QMAX[qd] + 1, ng).astype(np.uint8)
        codes = np.zeros(O.packed_numel(n, qd) * per, dtype=np.uint8)
        codes[:n] = np.repeat(zps, G)[:n]
        q = np.zeros(codes.size // per, dtype=np.uint8)
        for j in range(per):
            q |= codes[j::per] << np.uint8(j * bits)
        terms.append((q, (2.0 ** rng.integers(-12, 13, ng)).astype(np.float32), zps))
    return tuple(terms)


def ordinary_terms(k, n, qd, G, seed):
    rng = np.random.default_rng(seed)
    ng = (n + G - 1) // G
    terms = []
    for _ in range(k):
        q = rng.integers(0, 256, O.packed_numel(n, qd)).astype(np.uint8)
        if n % PACK[qd]:   # bits past the tensor's end are zero, as every quantize call leaves them
            q[-1] &= (1 << ((n % PACK[qd]) * E.BITS[qd])) - 1
        terms.append((q, rng.uniform(0.001, 3.0, ng).astype(np.float32), rng.integers(0, QMAX[qd] + 1, ng).astype(np.uint8)))
    return tuple(terms)


@pytest.mark.parametrize("kind", EF_KINDS)
@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_reduce_with_error_feedback(ctx, kind, qd, G):
    n = ef_inputs(kind, qd, G)[4].n
    try:
        for k, mode, tau in ((0, O.NEAREST, None), (1, O.NEAREST, None), (3, O.NEAREST, None), (3, O.STOCHASTIC, 0.375)):
            check_ef(ctx, kind, qd, G, zero_terms(k, n, qd, G, k), mode, tau, True, f"{kind} qd={qd} G={G} {k} zero terms mode={mode} tau={tau!r}")
        check_ef(ctx, kind, qd, G, ordinary_terms(3, n, qd, G, 9), O.NEAREST, None, True, f"{kind} qd={qd} G={G} 3 ordinary terms")
    finally:
        ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("dt_in,qd", PAIRS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_reduce(ctx, dt_in, qd, G):
    """reduce_quantize_grouped against model dequantize ADD per term followed by model quantize; with terms that add zero the sum stays the edge tensor"""
    bits, lay, ws, wz = edge_case(dt_in, qd, G)
    x = as_input(bits, dt_in)
    try:
        for terms, mode, tau, name in [(zero_terms(k, lay.n, qd, G, k), O.NEAREST, None, f"{k} zero terms") for k in (0, 1, 3)] + \
                                      [(zero_terms(3, lay.n, qd, G, 3), O.STOCHASTIC, 0.375, "3 zero terms"), (ordinary_terms(3, lay.n, qd, G, 9), O.NEAREST, None, "3 ordinary terms")]:
            what = f"dt_in={dt_in} qd={qd} G={G} {name} mode={mode} tau={tau!r}"
            ctx.set_stochastic_threshold(tau)
            q, s, z, _ = run_reduce(ctx, x, dt_in, None, None, terms, qd, G, mode, True)
            acc = x
            for tq, ts, tz in terms:
                acc = dequantize_grouped(tq, qd, dt_in, lay.n, G, ts, tz, O.ADD, prev=acc)
            if name.endswith("zero terms"):
                with np.errstate(invalid="ignore"):
                    fin = np.isfinite(E.values(bits))
                    assert np.array_equal(E.values(acc.view(bits.dtype))[fin], E.values(bits)[fin]), "the zero terms moved the sum"
                want, s_want, z_want = model_bytes(dt_in, qd, G, mode, tau), ws, wz
            else:
                want, s_want, z_want = quantize_grouped(acc, dt_in, qd, G, mode, tau or 0.0)
            assert_params(s, z, s_want, z_want, lay, what)
            assert_bytes(q, want, lay, qd, what)
            if name.endswith("zero terms"):
                assert_steps_agree(q, s, z, lay, qd, what)
    finally:
        ctx.set_stochastic_threshold(None)


# ---- 3. the batches against their single calls

def _bits_tensor(a, dt):
    """numpy bits or float32 array -> device tensor of the float dtype"""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.itemsize == 4 else np.int16).copy()).cuda()
    return t.view(FDT[dt])


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b)


@pytest.mark.parametrize("qd", [O.UINT8, O.UINT4])
@pytest.mark.parametrize("G", [64, 512, 2048])
def test_batches_equal_their_single_calls(ctx, qd, G):
    """17 members (two launches): edge tensors of different seeds, member 4 empty, member 7 one element off a 16-byte boundary"""
    import piquant.torch as pt

    def members(make):
        xs, rs = [], []
        for i in range(17):
            x, dt_x, r, dt_r = make(i)
            xt, rt = _bits_tensor(x, dt_x), _bits_tensor(r, dt_r)
            if i == 4:
                xt, rt = xt[:0], rt[:0]
            if i == 7:
                xt = torch.cat([xt[:1], xt])[1:]
                assert xt.data_ptr() % 16 == xt.element_size()
            xs.append(xt)
            rs.append(rt)
        return xs, rs

    for dt_in in (O.F32, O.BF16):
        xs, _ = members(lambda i: (edge_case(dt_in, qd, G, i)[0], dt_in, np.zeros(1, dtype=np.float32), O.F32))
        for mode, tau in (("nearest", None), ("stochastic", 0.375)):
            ctx.set_stochastic_threshold(tau)
            singles = [pt.quantize_grouped(x, dtype=QDT[qd], group_size=G, round_mode=mode) for x in xs]
            outs, ss, zs = pt.quantize_grouped_batch(xs, dtype=QDT[qd], group_size=G, round_mode=mode)
            torch.cuda.synchronize()
            for i, (wq, ws, wz) in enumerate(singles):
                assert _same(pt.packed_bytes(outs[i]), pt.packed_bytes(wq)) and _same(ss[i], ws) and _same(zs[i], wz), f"dt_in={dt_in} {mode} member {i}"
    for kind in EF_KINDS:
        for mode, tau in (("nearest", None), ("stochastic", 0.375)):
            ctx.set_stochastic_threshold(tau)
            xs, rs = members(lambda i: ef_inputs(kind, qd, G, i)[:4])
            singles = []
            for x, r in zip(xs, rs):
                rr = r.clone()
                q, s, z = pt.quantize_grouped_ef(x, rr, dtype=QDT[qd], group_size=G, round_mode=mode)
                singles.append((q, s, z, rr))
            outs, ss, zs = pt.quantize_grouped_ef_batch(xs, rs, dtype=QDT[qd], group_size=G, round_mode=mode)
            torch.cuda.synchronize()
            for i, (wq, ws, wz, wr) in enumerate(singles):
                assert _same(pt.packed_bytes(outs[i]), pt.packed_bytes(wq)) and _same(ss[i], ws) and _same(zs[i], wz), f"{kind} {mode} member {i}"
                assert _same(rs[i], wr), f"{kind} {mode} member {i}: residual"
    ctx.set_stochastic_threshold(None)


# ---- 6. dequantize_grouped around its own chunk

@pytest.mark.parametrize("op", [O.SET, O.ADD])
@pytest.mark.parametrize("dt_out", [O.F32, O.BF16])
@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_dequantize(ctx, qd, dt_out, op, G):
    import piquant

    rng = np.random.default_rng([G, qd, dt_out, op])
    chunk = 2048 * PACK[qd]   # GroupedDequantTile::CHUNK_ELEMS: what one wave dequantizes
    for n in (chunk - 1, chunk, chunk + 1, G - 1, 3 * chunk + G // 2 + 1):
        q = rng.integers(0, 256, O.packed_numel(n, qd)).astype(np.uint8)
        if n % PACK[qd]:   # bits past the tensor's end are zero, as every quantize call leaves them
            q[-1] &= (1 << ((n % PACK[qd]) * E.BITS[qd])) - 1
        ng = (n + G - 1) // G
        scales = rng.choice(np.array([1.0e-30, 1.0e30, 0.0078125, 0.37, 2.5], dtype=np.float32), ng)
        scales[rng.integers(0, ng)] = np.float32(rng.uniform(0.001, 3.0))
        zps = rng.choice(np.array([0, QMAX[qd], QMAX[qd] // 2, 1], dtype=np.uint8), ng)
        pf = rng.uniform(-5, 5, n).astype(np.float32)
        prev = pf if dt_out == O.F32 else O.f32_to_bf16(pf)
        qbuf, qin = _dev(q)
        obuf, oin = _dev(prev)
        sbuf, sin = _dev(scales)
        zbuf, zin = _dev(zps)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_blocking(False)
        ctx.dequantize_grouped_ptr(qin.data_ptr(), piquant.DataType(qd), oin.data_ptr(), piquant.DataType(dt_out), n, G, sin.data_ptr(), zin.data_ptr(),
                                   piquant.ReduceOp(op), _device_ptrs=True)
        torch.cuda.synchronize()
        assert _guard_ok(obuf, prev.nbytes), f"n={n}: wrote outside out"
        assert _unwritten(qin, q) and _unwritten(sin, scales) and _unwritten(zin, zps), f"n={n}: an input was written"
        got = oin.cpu().numpy().view(prev.dtype)
        want = dequantize_grouped(q, qd, dt_out, n, G, scales, zps, op, prev if op == O.ADD else None)
        bits = np.uint32 if dt_out == O.F32 else np.uint16
        bad = np.flatnonzero(got.view(bits) != want.view(bits))
        assert bad.size == 0, (f"n={n}: {bad.size} elements differ, first element {bad[0]} (group {bad[0] // G}, scale {scales[bad[0] // G]!r}, zero point "
                               f"{zps[bad[0] // G]}): got {got[bad[0]]!r} want {want[bad[0]]!r}")
