"""The fused grouped reduce + quantize with error feedback of a bfloat16 accumulator with a FLOAT32 residual on the MI355X
(piquant_hip_reduce_quantize_grouped_ef_mixed with dtype_acc = BF16, dtype_residual = F32; csrc/grouped_kernels.hpp:
reduce_quantize_grouped_ef_f32r_kernel).

The call is defined by a composition: grouped dequantize ADD of every term into the bfloat16 acc, in order, then the mixed
quantize_grouped_ef(acc, float32 residual).  Here: the call is ONE kernel launch where its alignment rule holds (counted in a captured graph);
its packed bytes, scales, zero points and residual equal, bit for bit (NaNs by position), the CPU model (tests/grouped_ef_f32r_sim.py:
reduce_ef_f32r_step) and that composition run on the device; the running sum is rounded to bfloat16 after every term (hand-built ties,
tests/reduce_ef_f32r_cases.py); stochastic rounding; misaligned buffers; conservation at float32 precision over chained steps.  0xAA canaries
stand in front of and behind every buffer of the call."""
import ctypes
import functools

import numpy as np
import pytest

import grouped_edge_cases as E
import oracle as O
from ef_model import EPS
from grouped_ef_f32r_sim import reduce_ef_f32r_step
from per_element_model import reduce_ef_f32r_per_element_model
from reduce_ef_f32r_cases import TIE_ORDERS, reduce_ef_f32r_model, tie_case
from test_gpu_grouped_ef_f32r import BITS, GROUP_SIZES, GUARD, QDS, QDT, assert_residual_equal, chunk_elems, make_input

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def _place(a, shift=0):
    """numpy array -> (device uint8 buffer, view of the data) with GUARD bytes of 0xAA in front of and behind the data, the data `shift` bytes
    off its 16-byte alignment"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((GUARD + shift + raw.size + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    view = buf[GUARD + shift: GUARD + shift + raw.size]
    if raw.size:
        view.copy_(torch.from_numpy(raw.copy()))
    assert view.data_ptr() % 16 == shift % 16
    return buf, view


def _intact(pair):
    buf, view = pair
    lo = view.data_ptr() - buf.data_ptr()
    return bool((buf[:lo] == 0xAA).all()) and bool((buf[lo + view.numel():] == 0xAA).all())


class Call:
    """One call's buffers on the device, preallocated: acc, residual, terms, out, scales, zero points, each between canaries.  shifts: bytes off
    the 16-byte alignment for "acc", "residual", "out" and ("term", i)."""

    def __init__(self, acc, r, terms, qd, G, shifts=None):
        shifts = shifts or {}
        self.n, self.qd, self.G = acc.size, qd, G
        self.ng, self.nbytes = (acc.size + G - 1) // G, O.packed_numel(acc.size, qd)
        self.acc0, self.r0, self.terms0 = acc, r, terms
        self.acc = _place(acc, shifts.get("acc", 0))
        self.res = _place(r, shifts.get("residual", 0))
        self.out = _place(np.full(self.nbytes, 0xAA, dtype=np.uint8), shifts.get("out", 0))
        self.scales = _place(np.zeros(self.ng, dtype=np.float32))
        self.zps = _place(np.zeros(self.ng, dtype=np.uint8))
        self.terms = [(_place(q, shifts.get(("term", i), 0)), _place(s), _place(z)) for i, (q, s, z) in enumerate(terms)]

    def restore(self):
        """acc is unspecified after a call and the residual is replaced: both as they were"""
        for (_, view), a in ((self.acc, self.acc0), (self.res, self.r0)):
            if a.size:
                view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))

    def enqueue(self, ctx, mode=O.NEAREST):
        import piquant

        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_blocking(False)
        ctx.reduce_quantize_grouped_ef_ptr(self.acc[1].data_ptr(), piquant.DataType.BF16, self.res[1].data_ptr(), [t[0][1].data_ptr() for t in self.terms],
                                           [t[1][1].data_ptr() for t in self.terms], [t[2][1].data_ptr() for t in self.terms], self.out[1].data_ptr(),
                                           piquant.DataType(self.qd), self.n, self.G, self.scales[1].data_ptr(), self.zps[1].data_ptr(),
                                           piquant.RoundMode(mode), _device_ptrs=True, residual_dtype=piquant.DataType.F32)

    def result(self):
        """after a synchronize: canaries, the terms untouched -> (packed bytes, scales, zero points, new residual) on the host"""
        for name, pair in (("out", self.out), ("scales", self.scales), ("zero_points", self.zps), ("the residual", self.res), ("acc", self.acc)):
            assert _intact(pair), f"wrote outside {name}"
        for i, (t, (q, s, z)) in enumerate(zip(self.terms, self.terms0)):
            for pair, a in zip(t, (q, s, z)):
                assert _intact(pair) and np.array_equal(pair[1].cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), f"term {i} was written"
        return (self.out[1].cpu().numpy(), self.scales[1].cpu().numpy().view(np.float32), self.zps[1].cpu().numpy(),
                self.res[1].cpu().numpy().view(np.float32))

    def run(self, ctx, mode=O.NEAREST):
        self.enqueue(ctx, mode)
        torch.cuda.synchronize()
        return self.result()


def composition(acc, r, terms, qd, G, mode="nearest"):
    """The definition on the device, through the public calls: dequantize_grouped(..., reduce_op="add", out=acc) per term, then the mixed
    quantize_grouped_ef(acc, residual) -> the four on the host"""
    import piquant.torch as pt

    a = torch.from_numpy(acc.view(np.int16).copy()).cuda().view(torch.bfloat16)
    rr = torch.from_numpy(r.copy()).cuda()
    for q, s, z in terms:
        pt.dequantize_grouped(torch.from_numpy(q.copy()).cuda(), torch.from_numpy(s.copy()).cuda(), torch.from_numpy(z.copy()).cuda(), dtype=torch.bfloat16,
                              group_size=G, reduce_op="add", out=a, quant_dtype=QDT[qd], shape=(acc.size,))
    cq, cs, cz = pt.quantize_grouped_ef(a, rr, dtype=QDT[qd], group_size=G, round_mode=mode)
    torch.cuda.synchronize()
    return pt.packed_bytes(cq).cpu().numpy().reshape(-1), cs.cpu().numpy(), cz.cpu().numpy(), rr.cpu().numpy()


def same(got, want, what):
    (q, s, z, r), (wq, ws, wz, wr) = got, want
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), f"{what}: scales differ at groups {np.flatnonzero(s.view(np.uint32) != ws.view(np.uint32))[:8]}"
    assert np.array_equal(z, wz), f"{what}: zero points differ at groups {np.flatnonzero(z != wz)[:8]}"
    bad = np.flatnonzero(q != wq)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at byte {bad[:8]}"
    assert_residual_equal(r, wr, what)


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def sizes(qd, G):
    """5 elements; one chunk - 1; exactly 2 chunks; 3 chunks + a partial group (n odd, n % 4 = 1: the last packed byte of uint4 and uint2 is partial)"""
    chunk = chunk_elems(qd, G)
    return [5, chunk - 1, 2 * chunk, 3 * chunk + G // 2 + 1]


@functools.lru_cache(maxsize=None)
def _edge_groups(qd, G):
    """whole groups of tests/grouped_edge_cases.py (float32 bits), one per class: NaNs, +-0, denormals, constant groups, infinities, one-sided
    groups far from zero and, for uint8, the two sides of the 1e9 line"""
    bits, lay = E.edge_tensor(E.F32, qd, G, 0)
    first = {}
    for g, c in enumerate(lay.cls):
        if lay.section[g] != "T":
            first.setdefault(c, bits[g * G: (g + 1) * G])
    names = ["nan_among", "zeros", "denormal_among", "const_near", "line_below", "line_above", "all_nan", "const_far", "pos_inf", "far_pos", "all_denormal",
             "far_neg", "neg_inf"]
    required = ["nan_among", "all_nan", "zeros", "denormal_among", "all_denormal", "const_near", "const_far"] + (["line_below", "line_above"] if qd == O.UINT8 else [])
    missing = [c for c in required if c not in first]
    assert not missing, f"tests/grouped_edge_cases.py no longer builds {missing}: NaN, +-0, denormal, constant and 1e9-line groups must be covered"
    return [(c, first[c]) for c in names if c in first]


def make_case(n, qd, G, seed):
    """acc (bf16 bits) and the float32 residual: make_input's varying magnitudes with planted outliers, and whole groups of the edge classes planted
    over it.  An edge group's float32 values x go in as acc = bf16(x), residual = x - widen(acc), which is exact for finite x: with no terms
    y = rn_f32(widen(acc) + r) is x bit for bit, so that the float32-only classes (the 1e9 line) reach the quantize step."""
    acc, r = make_input(n, seed)
    acc, r = acc.copy(), r.copy()
    full = n // G
    edges = _edge_groups(qd, G)
    slots = list(range(1, full, 2)) if full >= 2 * len(edges) else list(range(full))
    for j, g in enumerate(slots[: len(edges)]):
        xb = edges[(j + seed) % len(edges)][1]
        ab = E.narrow_bits(xb)
        x, a = xb.view(np.float32), E.widen_bits(ab).view(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.where(np.isfinite(x) & np.isfinite(a), x - a, np.float32(0.0)).astype(np.float32)
        acc[g * G: (g + 1) * G], r[g * G: (g + 1) * G] = ab, d
    return acc, r


def make_terms(n, qd, G, k, seed):
    """k terms of the wire type, quantized on the device from make_input-style tensors -> host (packed bytes, scales, zero points)"""
    import piquant.torch as pt

    out = []
    for i in range(k):
        x = torch.from_numpy(make_input(n, seed + 31 * i)[0].view(np.int16).copy()).cuda().view(torch.bfloat16)
        q, s, z = pt.quantize_grouped(x, dtype=QDT[qd], group_size=G)
        out.append((pt.packed_bytes(q).cpu().numpy().reshape(-1).copy(), s.cpu().numpy(), z.cpu().numpy()))
    return out


# ---- 1. one launch ---------------------------------------------------------------------------------------------------------------------
def _hip():
    """the HIP runtime this process has loaded (torch's)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    return hip


HIP_GRAPH_NODE_TYPE_KERNEL = 0


def _graph_shape(graph):
    """-> (node types, edges as (from, to) pairs) of a captured graph kept with keep_graph=True"""
    hip, g = _hip(), ctypes.c_void_p(int(graph.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    types = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) == 0
        types.append(t.value)
    m = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(m)) == 0
    src, dst = (ctypes.c_void_p * max(m.value, 1))(), (ctypes.c_void_p * max(m.value, 1))()
    if m.value:
        assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(m)) == 0
    return types, [(src[i], dst[i]) for i in range(m.value)]


@pytest.mark.parametrize("qd", [O.UINT8, O.UINT4])
@pytest.mark.parametrize("k,acc_shift,want_nodes", [(1, 0, 1), (7, 0, 1), (17, 0, 2), (1, 8, 1), (1, 2, 2), (7, 2, 8)])
def test_the_call_is_one_launch(ctx, qd, k, acc_shift, want_nodes):
    """Kernel nodes of the captured call: 1 for up to 16 terms, 2 with 17 (one grouped dequantize ADD, then the fused kernel with 16), and the
    composition's k + 1 when acc is moved by one element and is not 8-byte aligned; acc at 8 bytes off a 16-byte boundary is still 1 (its rows are
    8-byte loads).  The chain is linear; one replay gives the eager bytes."""
    G = 128
    n = 3 * chunk_elems(qd, G) + 5
    acc, r = make_input(n, 50 + k)
    call = Call(acc, r, make_terms(n, qd, G, k, 60 + k), qd, G, {"acc": acc_shift})
    ctx.set_stochastic_threshold(None)
    eager = call.run(ctx)
    same(eager, composition(acc, r, call.terms0, qd, G), "eager vs composition")
    call.restore()
    call.out[1].fill_(0xAA)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        call.enqueue(ctx)
    types, edges = _graph_shape(graph)
    kernels = sum(t == HIP_GRAPH_NODE_TYPE_KERNEL for t in types)
    print(f"qd={qd} k={k} acc shifted by {acc_shift} bytes: {len(types)} nodes, {kernels} of them kernels, {len(edges)} edges")
    assert kernels == want_nodes, (kernels, want_nodes, types)
    assert len(edges) == len(types) - 1 and len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges), "not a linear chain"
    graph.instantiate()
    graph.replay()
    torch.cuda.synchronize()
    same(call.result(), eager, "replay vs eager")


# ---- 2. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_parity_with_the_model_and_the_device_composition(ctx, qd, G):
    ctx.set_stochastic_threshold(None)
    for k in ([0, 1, 2, 7, 16, 17] if G == 128 else [1, 3]):
        for i, n in enumerate(sizes(qd, G)):
            seed = 7000 * G + 100 * k + 10 * i + qd
            acc, r = make_case(n, qd, G, seed)
            terms = make_terms(n, qd, G, k, seed + 1)
            got = Call(acc, r, terms, qd, G).run(ctx)
            what = f"qd={qd} G={G} k={k} n={n}"
            same(got, reduce_ef_f32r_step(acc, r, terms, qd, G)[:4], what + " vs model")
            same(got, composition(acc, r, terms, qd, G), what + " vs composition")


# ---- 3. the running sum is rounded to bfloat16 after every term ------------------------------------------------------------------------
@pytest.mark.parametrize("qd", QDS)
def test_running_sum_rounds_to_bfloat16_after_every_term(ctx, qd):
    """Hand-built terms on ties (tests/reduce_ef_f32r_cases.py; tests/test_grouped_reduce_ef_f32r_cpu.py proves that a float32 running sum gives
    other bytes on them), in several orders -- "AC" and "CA" differ in the result.  A full chunk, and a ragged one."""
    G = 128
    ctx.set_stochastic_threshold(None)
    for n in (2 * chunk_elems(qd, G), chunk_elems(qd, G) + G + 65):
        acc, r, t = tie_case(qd, G, n)
        results = {}
        for order in TIE_ORDERS:
            terms = [t[c] for c in order]
            results[order] = Call(acc, r, terms, qd, G).run(ctx)
            same(results[order], reduce_ef_f32r_step(acc, r, terms, qd, G)[:4], f"qd={qd} n={n} order={order} vs model")
        assert np.any(results["AC"][0] != results["CA"][0]) or np.any(results["AC"][3].view(np.uint32) != results["CA"][3].view(np.uint32))


# ---- 4. stochastic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qd", QDS)
def test_stochastic_pinned_thresholds_and_per_element(ctx, qd):
    """ONE threshold per call, pinned; and the per-element mode, which indexes the global element -- both against the model"""
    G, k = 128, 2
    n = sizes(qd, G)[3]
    acc, r = make_input(n, 900 + qd)
    terms = make_terms(n, qd, G, k, 910 + qd)
    seed, base = 0x1234_5678_9ABC, 77
    try:
        for tau in (0.0, 0.37, 0.999):
            ctx.set_stochastic_threshold(tau)
            got = Call(acc, r, terms, qd, G).run(ctx, O.STOCHASTIC)
            same(got, reduce_ef_f32r_model(acc, r, terms, qd, G, O.STOCHASTIC, tau), f"qd={qd} tau={tau} vs model")
            ctx.set_stochastic_threshold(tau)
            same(got, composition(acc, r, terms, qd, G, "stochastic"), f"qd={qd} tau={tau} vs composition")
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(True, seed=seed, index_base=base)
        got = Call(acc, r, terms, qd, G).run(ctx, O.STOCHASTIC)
        same(got, reduce_ef_f32r_per_element_model(acc, r, terms, qd, G, seed, base), f"qd={qd} per element vs model")
    finally:
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(False)


# ---- 5. alignment ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qd", QDS)
@pytest.mark.parametrize("which,shift", [("acc", 8), ("acc", 2), ("residual", 4), ("out", 1), (("term", 1), 1)])
def test_misaligned_buffers_give_the_aligned_call_s_bytes(ctx, qd, which, shift):
    """acc at 8 bytes off 16 still takes the fused kernel (its rows are 8-byte loads); acc off by one element, the residual by one float, out or
    one term by one byte take the composition: the same bytes, canaries intact"""
    G, k = 128, 3
    n = sizes(qd, G)[3]
    acc, r = make_input(n, 300 + qd)
    terms = make_terms(n, qd, G, k, 310 + qd)
    ctx.set_stochastic_threshold(None)
    same(Call(acc, r, terms, qd, G, {which: shift}).run(ctx), Call(acc, r, terms, qd, G).run(ctx), f"qd={qd} {which} off by {shift}")


# ---- 6. conservation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qd", QDS)
def test_conservation_over_chained_reduce_steps(ctx, qd):
    """K = 8 chained steps with k = 2 terms on the device, finite inputs: with a_t the bfloat16 partial sum the step quantizes (acc and its terms,
    by the public dequantize ADD) and d_t = dequantize_grouped(q_t, dtype=float32), S = sum_t d_t + r_K - sum_t widen(a_t) in float64 stays within
    K 2^-23 M: two float32 roundings per step (y = rn(a + r), r = rn(y - d)) of at most half an ulp each, M the largest |y| or |d| seen -- the
    bound of test_conservation_on_the_device (tests/test_gpu_grouped_ef_f32r.py)."""
    import piquant.torch as pt

    G, K, k = 128, 8, 2
    n = sizes(qd, G)[3]
    res = torch.zeros(n, dtype=torch.float32, device="cuda")
    S, M = np.zeros(n, dtype=np.float64), 0.0
    ctx.set_stochastic_threshold(None)
    for t in range(K):
        acc = torch.from_numpy(make_input(n, 400 + t)[0].view(np.int16).copy()).cuda().view(torch.bfloat16)
        terms = [tuple(torch.from_numpy(a.copy()).cuda() for a in term) for term in make_terms(n, qd, G, k, 500 + 10 * t)]
        a = acc.clone()
        for tq, ts, tz in terms:
            pt.dequantize_grouped(tq, ts, tz, dtype=torch.bfloat16, group_size=G, reduce_op="add", out=a, quant_dtype=QDT[qd], shape=(n,))
        y = torch.add(a.float(), res)
        q, s, z = pt.reduce_quantize_grouped_ef(acc, res, [x[0] for x in terms], [x[1] for x in terms], [x[2] for x in terms], dtype=QDT[qd], group_size=G)
        d = pt.dequantize_grouped(q, s, z, dtype=torch.float32, group_size=G)
        S += d.double().cpu().numpy() - a.double().cpu().numpy()
        M = max(M, float(y.abs().max()), float(d.abs().max()))
    S += res.double().cpu().numpy()
    defect, bound = float(np.abs(S).max()), K * EPS[O.F32] * M
    print(f"qd={qd}: max|S| = {defect:.3g} (bound {bound:.3g})")
    assert np.isfinite(S).all() and defect <= bound, (defect, bound)
