"""Error feedback in the rotated domain on the MI355X: piquant.torch.quantize_grouped_rotated_ef and reduce_quantize_grouped_rotated_ef against
the CPU model (tests/rot_ef_model.py) and against the composition of public calls that defines them, run on the device in the same process --
bit for bit in packed bytes, scales, zero points AND residual; NaN positions are compared, NaN payloads are not.

Shapes as tests/test_gpu_grouped_rotated_reduce.py: numel = 9 NG G + 3 G + 5 per group size and width (two full blocks, a chunk the tensor ends
in that still holds whole groups, a ragged last group), and numel < G, numel == G, numel == 0.  Term counts 0, 1, 2, 7, 16."""
import numpy as np
import pytest

import oracle as O
import rot_ef_model as RE
import rot_model as R
import test_gpu_grouped_rotated as T
import test_gpu_grouped_rotated_reduce as RR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ctx = T.ctx   # the module's context fixture: threshold and per-element mode restored at the end

SEED = RR.SEED
COUNTS = RR.COUNTS


def residual_of(n, G, seed=41):
    """a float32 residual of the size one step leaves: a hundredth of heavy-tailed values"""
    return (np.array(T.data(n, O.F32, G, seed=seed)) * np.float32(0.01)).astype(np.float32)


def call_ef(acc, r_host, terms, qd, G, mode, off_res=0, off_out=0, off_params=0, plain=False):
    """reduce_quantize_grouped_rotated_ef (plain: quantize_grouped_rotated_ef) into carved buffers, the residual in a carved buffer of its own
    -> (bytes, scales, zero points, residual) on the host, canaries checked"""
    import piquant.torch as pt

    n, ng, nb = acc.numel(), (acc.numel() + G - 1) // G, T.packed_nbytes(acc.numel(), qd)
    rb, r, r0 = RR.put(r_host, torch.float32, off_res)
    qb, q, q0 = T.carve(nb, torch.uint8, off_out)
    sb, s, s0 = T.carve(ng, torch.float32, off_params)
    zb, z, z0 = T.carve(ng, torch.uint8, off_params)
    kw = dict(dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode=mode, out=q, out_scales=s, out_zero_points=z)
    if plain:
        got = pt.quantize_grouped_rotated_ef(acc, r, **kw)
    else:
        got = pt.reduce_quantize_grouped_rotated_ef(acc, r, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], **kw)
    torch.cuda.synchronize()
    assert got[0] is q and got[1] is s and got[2] is z
    T.canaries_intact(rb, r0, n * 4, "residual")
    T.canaries_intact(qb, q0, nb, "packed bytes")
    T.canaries_intact(sb, s0, ng * 4, "scales")
    T.canaries_intact(zb, z0, ng, "zero points")
    return q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy(), r.cpu().numpy()


def composition(acc, r_host, terms, qd, G, mode):
    """hadamard_grouped of the widened tensor, one float32 dequantize ADD per term, quantize_grouped_ef with the float32 residual"""
    import piquant.torch as pt

    n = acc.numel()
    r = torch.from_numpy(r_host.copy()).cuda()
    y = pt.hadamard_grouped(acc.float(), group_size=G, seed=SEED)
    for q, s, z in terms:
        pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=G, reduce_op="add", out=y, quant_dtype=T.QDT[qd], shape=(n,))
    q, s, z = pt.quantize_grouped_ef(y, r, dtype=T.QDT[qd], group_size=G, round_mode=mode)
    return (pt.packed_bytes(q).cpu().numpy() if n else np.zeros(0, dtype=np.uint8)), s.cpu().numpy(), z.cpu().numpy(), r.cpu().numpy()


def quad_same(got, want, what):
    T.triple_same(got[:3], want[:3], what)
    T.same(got[3], np.asarray(want[3], dtype=np.float32), what + ": residual")


def modes(ctx):
    """(name, the call's round_mode, arm the context, the model)"""
    base = RR.modes(ctx)
    models = [lambda acc, dt, r, terms, qd, G: RE.reduce_quantize_grouped_rotated_ef(acc, dt, r, terms, qd, G, SEED),
              lambda acc, dt, r, terms, qd, G: RE.reduce_quantize_grouped_rotated_ef(acc, dt, r, terms, qd, G, SEED, O.STOCHASTIC, T.THRESHOLD),
              lambda acc, dt, r, terms, qd, G: RE.reduce_quantize_grouped_rotated_ef_per_element(acc, dt, r, terms, qd, G, SEED, T.ELEM_SEED, T.INDEX_BASE)]
    return [(name, mode, arm, model) for (name, mode, arm, _), model in zip(base, models)]


def restore(ctx):
    ctx.set_stochastic_threshold(None)
    ctx.set_stochastic_per_element(False)


# ---- both calls, every dtype pair, group size, rounding mode and term count

@pytest.mark.parametrize("case", RR.CASES, ids=RR.CASE_IDS)
def test_rotated_ef_calls(ctx, case):
    (dt, qd), G = case
    n = RR.numel_of(qd, G)
    acc, r0 = T.data(n, dt, G, seed=30), residual_of(n, G)
    ab, accd, a0 = T.carve(n, T.FDT[dt])
    accd.copy_(T.dev(acc, dt))
    host_terms = RR.terms_of(qd, G, n)
    dev_terms = RR.terms_dev(host_terms)
    try:
        for k in COUNTS:
            for name, mode, arm, model in modes(ctx):
                arm()
                got = call_ef(accd, r0, dev_terms[:k], qd, G, mode)
                with np.errstate(over="ignore", invalid="ignore"):
                    quad_same(got, model(acc, dt, r0, host_terms[:k], qd, G), f"{name}, {k} terms: model")
                quad_same(got, composition(accd, r0, dev_terms[:k], qd, G, mode), f"{name}, {k} terms: composition")
                if k == 0:
                    quad_same(call_ef(accd, r0, [], qd, G, mode, plain=True), got, f"{name}: no terms is quantize_grouped_rotated_ef")
        restore(ctx)
        zero = call_ef(accd, np.zeros(n, dtype=np.float32), [], qd, G, "nearest", plain=True)
        T.triple_same(zero[:3], T.quantize_rotated(accd, qd, G, SEED, "nearest"), "a zero residual gives the bytes of quantize_grouped_rotated")
    finally:
        restore(ctx)
    T.same(T.host(accd), acc, "the tensor is only read")
    T.canaries_intact(ab, a0, n * accd.element_size(), "the tensor")


@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_short_tensors(ctx, pair):
    dt, qd = pair
    restore(ctx)
    for G in (32, 128, 4096):
        for n in (0, G - 1, G):
            acc, r0 = T.data(n, dt, G, seed=31), residual_of(n, G, 42)
            accd = T.dev(acc, dt)
            for k in (0, 2):
                host_terms = RR.terms_of(qd, G, n, 2, 60)
                got = call_ef(accd, r0, RR.terms_dev(host_terms[:k]), qd, G, "nearest", plain=(k == 0))
                quad_same(got, RE.reduce_quantize_grouped_rotated_ef(acc, dt, r0, host_terms[:k], qd, G, SEED), f"G={G}, n={n}, {k} terms")


def test_an_empty_tensor_draws_no_threshold(ctx):
    """numel == 0 is a no-op: with a seeded generator, the next call's threshold is the one it would have drawn anyway"""
    import piquant.torch as pt

    G, n, qd = 128, 1000, O.UINT8
    x = T.dev(T.data(n, O.F32, G, seed=32), O.F32)
    empty, none = torch.empty(0, device="cuda"), torch.empty(0, device="cuda")
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    outs = []
    for with_empty in (False, True):
        ctx.set_stochastic_seed(1234)
        if with_empty:
            pt.quantize_grouped_rotated_ef(empty, none, dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode="stochastic")
            pt.reduce_quantize_grouped_rotated_ef(empty, none, [], [], [], dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode="stochastic")
        r = torch.zeros(n, device="cuda")
        q, s, z = pt.quantize_grouped_rotated_ef(x, r, dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode="stochastic")
        outs.append((q.cpu().numpy(), r.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- four chained steps, the residual carried: outlier data with a NaN and a constant group among it

@pytest.mark.parametrize("pair", [(O.F32, O.UINT4), (O.BF16, O.UINT8), (O.BF16, O.UINT2)], ids=("f32-u4", "bf16-u8", "bf16-u2"))
@pytest.mark.parametrize("k", (0, 2))
def test_chained_steps_follow_the_model(ctx, pair, k):
    import piquant.torch as pt

    dt, qd = pair
    G, ng = 128, 40
    n = G * ng + 17
    restore(ctx)
    r_model = np.zeros(n, dtype=np.float32)
    rb, r_dev, r_first = T.carve(n, torch.float32)
    r_dev.zero_()
    for step in range(4):
        x = np.zeros(n, dtype=np.float32)
        x[: G * ng] = R.outlier_data(G, ng, 100 + step)
        x[G * ng:] = 0.5
        x[5 * G: 6 * G] = 3.25                 # a constant group
        if step == 1:
            x[9 * G + 11] = np.nan             # a NaN: its whole group's residual is NaN from here on
        x = x if dt == O.F32 else O.f32_to_bf16(x)
        host_terms = RR.terms_of(qd, G, n, k, 200 + 10 * step) if k else ()
        dev_terms = RR.terms_dev(host_terms)
        xd = T.dev(x, dt)
        lists = ([t[0] for t in dev_terms], [t[1] for t in dev_terms], [t[2] for t in dev_terms])
        if k:
            q, s, z = pt.reduce_quantize_grouped_rotated_ef(xd, r_dev, *lists, dtype=T.QDT[qd], group_size=G, seed=SEED)
        else:
            q, s, z = pt.quantize_grouped_rotated_ef(xd, r_dev, dtype=T.QDT[qd], group_size=G, seed=SEED)
        torch.cuda.synchronize()
        with np.errstate(over="ignore", invalid="ignore"):
            want = RE.reduce_quantize_grouped_rotated_ef(x, dt, r_model, host_terms, qd, G, SEED)
        r_model = want[3]
        quad_same((pt.packed_bytes(q).cpu().numpy(), s.cpu().numpy(), z.cpu().numpy(), r_dev.cpu().numpy()), want, f"step {step}")
        T.canaries_intact(rb, r_first, n * 4, "residual")
    nan = np.isnan(r_model)
    assert nan[9 * G: 10 * G].all() and nan.sum() == G


# ---- one buffer at a time off a 16-byte boundary: the guarded kernel, the same bytes

@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_misaligned_buffers_give_the_same_bytes(ctx, pair):
    dt, qd = pair
    try:
        for G, n in ((128, 128 * 9 + 77), (4096, 4096 * 2 + 1), (32, 32 * 40 + 31)):
            acc, r0 = T.data(n, dt, G, seed=35), residual_of(n, G, 43)
            for k in (0, 3):
                host_terms = RR.terms_of(qd, G, n, k, 80) if k else ()
                for name, mode, arm, model in modes(ctx):
                    arm()
                    with np.errstate(over="ignore", invalid="ignore"):
                        want = model(acc, dt, r0, host_terms, qd, G)
                    for what, off_acc, kw_terms, kw in (("the tensor", 1, {}, {}), ("the residual", 0, {}, dict(off_res=1)), ("out", 0, {}, dict(off_out=1)),
                                                        ("a term", 0, dict(off_q=1, which=1), {}),
                                                        ("the parameter arrays", 0, dict(off_p=1), dict(off_params=1))):
                        if what == "a term" and not k:
                            continue
                        ab, accm, a0 = T.carve(n, T.FDT[dt], off_acc)
                        accm.copy_(T.dev(acc, dt))
                        got = call_ef(accm, r0, RR.terms_dev(host_terms, **kw_terms), qd, G, mode, plain=(k == 0), **kw)
                        quad_same(got, want, f"G={G}, {k} terms, {name}, {what} misaligned")
                        T.same(T.host(accm), acc, "the tensor is only read")
                        T.canaries_intact(ab, a0, n * accm.element_size(), "the tensor")
    finally:
        restore(ctx)


# ---- wrong arguments raise before any launch

def test_wrong_arguments_raise_value_error(ctx):
    import piquant.torch as pt

    G, n, qd = 128, 1000, O.UINT8
    terms = RR.terms_dev(RR.terms_of(qd, G, n, 1, 90) * 17)
    lists = ([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms])
    acc, r = torch.ones(n, device="cuda"), torch.full((n,), 2.0, device="cuda")
    kw = dict(dtype=torch.uint8, group_size=G, seed=SEED)
    with pytest.raises(ValueError, match="at most 16"):
        pt.reduce_quantize_grouped_rotated_ef(acc, r, *lists, **kw)
    with pytest.raises(ValueError, match="seed"):
        pt.reduce_quantize_grouped_rotated_ef(acc, r, *(x[:2] for x in lists), dtype=torch.uint8, group_size=G)
    with pytest.raises(ValueError, match="seed"):
        pt.quantize_grouped_rotated_ef(acc, r, dtype=torch.uint8, group_size=G)
    bf = torch.ones(n, dtype=torch.bfloat16, device="cuda")
    for bad, match in ((torch.zeros(n, dtype=torch.bfloat16, device="cuda"), "float32"), (torch.zeros(n, dtype=torch.float64, device="cuda"), "float32"),
                       (torch.zeros(n - 1, device="cuda"), "numel"), (torch.zeros(2 * n, device="cuda")[::2], "contiguous"), (torch.zeros(n), "device"),
                       (None, "torch.Tensor")):
        for x in (acc, bf):
            with pytest.raises(ValueError, match=match):
                pt.quantize_grouped_rotated_ef(x, bad, **kw)
            with pytest.raises(ValueError, match=match):
                pt.reduce_quantize_grouped_rotated_ef(x, bad, *(v[:2] for v in lists), **kw)
    for bad in (100, 16, 8192, None):
        with pytest.raises(ValueError, match="group_size"):
            pt.quantize_grouped_rotated_ef(acc, r, dtype=torch.uint8, group_size=bad, seed=SEED)
    torch.cuda.synchronize()
    assert bool((acc == 1).all()) and bool((r == 2).all())


# ---- hipGraph capture: a replay advances the residual as an eager call does

def test_graph_capture_and_replay(ctx):
    import piquant.torch as pt

    G, qd, k = 128, O.UINT4, 3
    n = RR.numel_of(qd, G)
    restore(ctx)
    terms = RR.terms_dev(RR.terms_of(qd, G, n, k, 95))
    lists = ([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms])
    x = T.dev(T.data(n, O.BF16, G, seed=96), O.BF16)

    def calls(r_plain, r_reduce):
        raw = [torch.empty(T.packed_nbytes(n, qd), dtype=torch.uint8, device="cuda") for _ in range(2)]
        a = pt.quantize_grouped_rotated_ef(x, r_plain, dtype=T.QDT[qd], group_size=G, seed=SEED, out=raw[0])
        b = pt.reduce_quantize_grouped_rotated_ef(x, r_reduce, *lists, dtype=T.QDT[qd], group_size=G, seed=SEED, out=raw[1])
        return a + b

    calls(torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"))   # warm-up outside capture (code objects)
    torch.cuda.synchronize()
    captured_r = [torch.zeros(n, device="cuda") for _ in range(2)]
    eager_r = [torch.zeros(n, device="cuda") for _ in range(2)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = calls(*captured_r)
    for r in captured_r:
        r.zero_()          # whatever the capture did to them
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        eager = calls(*eager_r)
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            T.same(T.host(got), T.host(want), f"replay {replay}: captured output")
        for got, want in zip(captured_r, eager_r):
            T.same(T.host(got), T.host(want), f"replay {replay}: residual")
    assert bool((captured_r[0] != 0).any())
