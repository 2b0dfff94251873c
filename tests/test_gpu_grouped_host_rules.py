"""Rules of the host path of the group-wise entry points (csrc/capi_grouped.cpp) that no kernel test pins: how many stochastic thresholds a
call draws, that a blocking call has completed when it returns in every wait mode, that the independent-calls scope keeps a call with given
parameters behind the call that wrote them, and where the surplus of a reduce over 16 terms goes.

Every comparison is bit for bit against the same work done by other calls on the device; none of it depends on the values quantized."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pq(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    return piquant


def _raw(q):
    import piquant.torch as pt

    return q.view(-1) if q.dtype == torch.uint8 else pt.packed_bytes(q)


def _data(n, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.rand(n, device="cuda", generator=g) * 6.0 - 3.0).to(dtype)


def _off_by_one(t):
    """a copy of t that starts one element behind a 16-byte boundary"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    base[1:].copy_(t)
    assert base[1:].data_ptr() % 16 != 0
    return base[1:]


def _terms(n, G, k, qdtype, seed, fdt=torch.float32):
    """k packed terms (raw bytes, scales, zero points) of n elements"""
    import piquant.torch as pt

    out = []
    for i in range(k):
        q, s, z = pt.quantize_grouped(_data(n, seed + i, fdt), dtype=qdtype, group_size=G)
        out.append((_raw(q).clone(), s, z))
    return out


class _Out:
    """packed bytes, scales and zero points of n elements in groups of G"""

    def __init__(self, n, G, qdt, shift=0):
        nb, ng = qdt.packed_nbytes(n), -(-n // G)
        self.out = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")[shift: shift + nb]
        self.scales = torch.zeros(ng, dtype=torch.float32, device="cuda")
        self.zp = torch.zeros(ng, dtype=torch.uint8, device="cuda")

    def ptrs(self):
        return self.out.data_ptr(), self.scales.data_ptr(), self.zp.data_ptr()

    def tensors(self):
        return [self.out, self.scales.view(torch.uint8), self.zp]


def _term_ptrs(terms):
    return [t[0].data_ptr() for t in terms], [t[1].data_ptr() for t in terms], [t[2].data_ptr() for t in terms]


# ---- 1. draws ----------------------------------------------------------------------------------------------------------------------------------

def _sequence_with_eight_draws(pq, ctx):
    """Twelve stochastic grouped calls (fp32 -> uint8, G = 32) of which eight draw a threshold; the number each must draw stands beside it."""
    F32, BF16, U8, ST = pq.DataType.F32, pq.DataType.BF16, pq.DataType.UINT8, pq.RoundMode.STOCHASTIC
    G, n = 32, 96
    x, res = _data(n, 1), torch.zeros(n, device="cuda")
    xb, res32 = _data(33, 2, torch.bfloat16), torch.zeros(33, device="cuda")
    o, ob = _Out(n, G, pq.DataType.UINT8), _Out(33, G, pq.DataType.UINT8)
    terms17, termsb = _terms(n, G, 17, torch.uint8, 10), _terms(33, G, 2, torch.uint8, 40, torch.bfloat16)
    members = [(_data(n, 50 + i), torch.zeros(n, device="cuda"), _Out(n, G, pq.DataType.UINT8), n) for i in range(17)]
    members[3] = members[3][:3] + (0,)                                                       # an empty member
    members[9] = (_off_by_one(members[9][0]),) + members[9][1:]                              # a member that runs alone, guarded
    res_off, acc_f, acc = _off_by_one(res), x.clone(), x.clone()
    torch.cuda.synchronize()
    qp, sp, zp = o.ptrs()
    # a: 0
    ctx.quantize_grouped_ptr(x.data_ptr(), F32, qp, U8, 0, G, sp, zp, False, ST, _device_ptrs=True)
    # b: 1 -- a batch whose members are all empty still draws
    ctx.quantize_grouped_batch_ptr([x.data_ptr()] * 3, F32, [qp] * 3, U8, [0, 0, 0], G, [sp] * 3, [zp] * 3, False, ST, _device_ptrs=True)
    # c: 0 -- through the method (which returns by itself) and through the entry point
    ctx.quantize_grouped_batch_ptr([], F32, [], U8, [], G, [], [], False, ST, _device_ptrs=True)
    pq.C.piquant_hip_quantize_grouped_batch(ctx._ctx, None, F32.value, None, U8.value, None, G, None, None, 0, 0, ST.value)
    # d: 0
    ctx.quantize_grouped_ef_ptr(x.data_ptr(), F32, res.data_ptr(), qp, U8, 0, G, sp, zp, ST, _device_ptrs=True)
    # e: 1
    ctx.quantize_grouped_ef_batch_ptr([m[0].data_ptr() for m in members], F32, [m[1].data_ptr() for m in members], [m[2].ptrs()[0] for m in members], U8,
                                      [m[3] for m in members], G, [m[2].ptrs()[1] for m in members], [m[2].ptrs()[2] for m in members], ST,
                                      _device_ptrs=True)
    # f: 1
    ctx.reduce_quantize_grouped_ptr(acc_f.data_ptr(), F32, [], [], [], qp, U8, n, G, sp, zp, ST, _device_ptrs=True)
    # g: 1 -- one grouped dequantize ADD and the fused kernel
    ctx.reduce_quantize_grouped_ef_ptr(acc.data_ptr(), F32, res.data_ptr(), *_term_ptrs(terms17), qp, U8, n, G, sp, zp, ST, _device_ptrs=True)
    # h: 1 -- the two-step form
    ctx.reduce_quantize_grouped_ef_ptr(acc.data_ptr(), F32, res_off.data_ptr(), *_term_ptrs(terms17[:2]), qp, U8, n, G, sp, zp, ST, _device_ptrs=True)
    qb, sb, zb = ob.ptrs()
    # i: 1
    ctx.quantize_grouped_ef_ptr(xb.data_ptr(), BF16, res32.data_ptr(), qb, U8, 33, G, sb, zb, ST, _device_ptrs=True, residual_dtype=F32)
    # j: 0
    ctx.quantize_grouped_ef_ptr(xb.data_ptr(), BF16, res32.data_ptr(), qb, U8, 0, G, sb, zb, ST, _device_ptrs=True, residual_dtype=F32)
    # k: 1
    ctx.reduce_quantize_grouped_ef_ptr(xb.data_ptr(), BF16, res32.data_ptr(), *_term_ptrs(termsb), qb, U8, 33, G, sb, zb, ST, _device_ptrs=True,
                                       residual_dtype=F32)
    # l: 1 -- forwards to the plain entry, which draws; the forwarding one does not
    ctx.quantize_grouped_ef_ptr(x.data_ptr(), F32, res.data_ptr(), qp, U8, n, G, sp, zp, ST, _device_ptrs=True, residual_dtype=F32)


def _plain_calls(pq, ctx, count):
    G, n = 32, 96
    x, o = _data(n, 1), _Out(n, G, pq.DataType.UINT8)
    qp, sp, zp = o.ptrs()
    torch.cuda.synchronize()
    for _ in range(count):
        ctx.quantize_grouped_ptr(x.data_ptr(), pq.DataType.F32, qp, pq.DataType.UINT8, n, G, sp, zp, False, pq.RoundMode.STOCHASTIC, _device_ptrs=True)


def _probe(pq, ctx, x):
    o = _Out(x.numel(), 32, pq.DataType.UINT8)
    torch.cuda.synchronize()
    ctx.quantize_grouped_ptr(x.data_ptr(), pq.DataType.F32, o.ptrs()[0], pq.DataType.UINT8, x.numel(), 32, o.ptrs()[1], o.ptrs()[2], False,
                             pq.RoundMode.STOCHASTIC, _device_ptrs=True)
    torch.cuda.synchronize()
    return o.out.clone()


def test_stochastic_draws_per_call(pq):
    """One threshold per entry-point call whichever path runs, none for a call that returns at numel == 0 (count == 0 for a batch).  The generator of
    a seeded context is the witness: after the twelve calls of the sequence it stands where eight plain calls leave it, and not where seven do.
    The probe holds 4096 values whose positions inside their quantization step are spread evenly: two thresholds further apart than a few
    1/4096 round some of them differently."""
    ctxs = [pq.Context(1) for _ in range(3)]   # blocking, each on its own stream
    for c in ctxs:
        c.set_stochastic_seed(0x5EED)
    _sequence_with_eight_draws(pq, ctxs[0])
    _plain_calls(pq, ctxs[1], 8)
    _plain_calls(pq, ctxs[2], 7)
    x = _data(4096, 99)
    a, b, control = (_probe(pq, c, x) for c in ctxs)
    assert not torch.equal(b, control), "the probe does not tell eight draws from seven"
    assert torch.equal(a, b), "the sequence did not draw eight thresholds"


# ---- 2. blocking calls -------------------------------------------------------------------------------------------------------------------------

class _BlockingCase:
    """The five calls of test_blocking_calls_have_completed_when_they_return on fresh buffers; call(i) makes call i, outputs(i) lists what it wrote."""
    N, G = 4099, 128

    def __init__(self, pq, given):
        U8 = pq.DataType.UINT8
        n, G = self.N, self.G
        self.pq = pq
        self.x = _data(n, 7)
        self.q, self.s, self.z = given                                                            # a quantized tensor for the dequantize
        self.o = _Out(n, G, U8)
        self.deq = torch.zeros(n, device="cuda")
        self.batch = [(_data(n, 100 + i), _Out(n, G, U8)) for i in range(17)]
        self.ef = [(_data(n, 200), _data(n, 201) * 0.01, _Out(n, G, U8)), (_off_by_one(_data(n, 202)), _data(n, 203) * 0.01, _Out(n, G, U8))]
        self.acc, self.res, self.ro = _data(n, 300), _data(n, 301) * 0.01, _Out(n, G, U8)
        self.term = _terms(n, G, 1, torch.uint8, 310)

    def call(self, i, ctx):
        pq, n, G = self.pq, self.N, self.G
        F32, U8, NEAR = pq.DataType.F32, pq.DataType.UINT8, pq.RoundMode.NEAREST
        if i == 0:
            ctx.quantize_grouped_ptr(self.x.data_ptr(), F32, self.o.ptrs()[0], U8, n, G, self.o.ptrs()[1], self.o.ptrs()[2], False, NEAR, _device_ptrs=True)
        elif i == 1:
            ctx.dequantize_grouped_ptr(self.q.data_ptr(), U8, self.deq.data_ptr(), F32, n, G, self.s.data_ptr(), self.z.data_ptr(), pq.ReduceOp.SET,
                                       _device_ptrs=True)
        elif i == 2:
            ctx.quantize_grouped_batch_ptr([x.data_ptr() for x, _ in self.batch], F32, [o.ptrs()[0] for _, o in self.batch], U8, [n] * 17, G,
                                           [o.ptrs()[1] for _, o in self.batch], [o.ptrs()[2] for _, o in self.batch], False, NEAR, _device_ptrs=True)
        elif i == 3:
            ctx.quantize_grouped_ef_batch_ptr([m[0].data_ptr() for m in self.ef], F32, [m[1].data_ptr() for m in self.ef], [m[2].ptrs()[0] for m in self.ef],
                                              U8, [n] * 2, G, [m[2].ptrs()[1] for m in self.ef], [m[2].ptrs()[2] for m in self.ef], NEAR, _device_ptrs=True)
        else:
            ctx.reduce_quantize_grouped_ef_ptr(self.acc.data_ptr(), F32, self.res.data_ptr(), *_term_ptrs(self.term), self.ro.ptrs()[0], U8, n, G,
                                               self.ro.ptrs()[1], self.ro.ptrs()[2], NEAR, _device_ptrs=True)

    def outputs(self, i):
        if i == 0:
            return self.o.tensors()
        if i == 1:
            return [self.deq.view(torch.uint8)]
        if i == 2:
            return [t for _, o in self.batch for t in o.tensors()]
        if i == 3:
            return [t for m in self.ef for t in m[2].tensors() + [m[1].view(torch.uint8)]]
        return self.ro.tensors() + [self.res.view(torch.uint8)]


def test_blocking_calls_have_completed_when_they_return(pq):
    """Each grouped entry family as a blocking call on the context's own stream, in every wait mode: what it wrote is copied out on ANOTHER stream
    the moment it returns, with nothing waiting for the call's stream -- right only if the call had completed.  Compared with the same calls made
    stream-ordered and synchronised."""
    import piquant.torch as pt

    q, s, z = pt.quantize_grouped(_data(_BlockingCase.N, 8), dtype=torch.uint8, group_size=_BlockingCase.G)
    ctx = pq.Context(1)
    side = torch.cuda.Stream()
    try:
        ctx.set_blocking(False)
        ordered = _BlockingCase(pq, (q, s, z))
        torch.cuda.synchronize()
        for i in range(5):
            ordered.call(i, ctx)
        torch.cuda.synchronize()
        want = [[t.cpu() for t in ordered.outputs(i)] for i in range(5)]
        ctx.set_blocking(True)
        for mode in ('sync', 'write32', 'kernel', 'event'):
            ctx.set_blocking_wait(mode)
            case = _BlockingCase(pq, (q, s, z))
            hosts = [[torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in case.outputs(i)] for i in range(5)]
            torch.cuda.synchronize()
            for i in range(5):
                case.call(i, ctx)
                with torch.cuda.stream(side):
                    for h, t in zip(hosts[i], case.outputs(i)):
                        h.copy_(t, non_blocking=True)
            torch.cuda.synchronize()
            for i in range(5):
                for j, (h, w) in enumerate(zip(hosts[i], want[i])):
                    assert torch.equal(h, w), f"wait mode {mode}: output {j} of call {i} was not complete when the call returned"
    finally:
        ctx.set_blocking_wait('kernel')
        ctx.set_blocking(False)


# ---- 3. independent calls ----------------------------------------------------------------------------------------------------------------------

def test_independent_calls_scope_keeps_given_parameters_ordered(pq):
    """Six quantize_grouped calls that compute their parameters may overtake one another inside independent_calls(); the seventh reads the sixth's
    parameters and must stay behind it.  All seven give the bytes of the ordered run."""
    F32, U8, NEAR = pq.DataType.F32, pq.DataType.UINT8, pq.RoundMode.NEAREST
    n, G = 4099, 32
    x = _data(n, 21)

    def run(ctx, independent):
        import contextlib

        outs = [_Out(n, G, U8) for _ in range(7)]
        torch.cuda.synchronize()
        with (ctx.independent_calls() if independent else contextlib.nullcontext()):
            for o in outs[:6]:
                ctx.quantize_grouped_ptr(x.data_ptr(), F32, o.ptrs()[0], U8, n, G, o.ptrs()[1], o.ptrs()[2], False, NEAR, _device_ptrs=True)
            ctx.quantize_grouped_ptr(x.data_ptr(), F32, outs[6].ptrs()[0], U8, n, G, outs[5].ptrs()[1], outs[5].ptrs()[2], True, NEAR, _device_ptrs=True)
        torch.cuda.synchronize()
        return outs

    ctx = pq.Context(1)
    stream = torch.cuda.Stream()
    ctx.set_blocking(False)
    ctx.set_stream(stream.cuda_stream)
    try:
        want = run(ctx, False)
        got = run(ctx, True)
    finally:
        ctx.reset_stream()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g.out, w.out), f"call {i}: bytes"
        if i < 6:
            assert torch.equal(g.scales.view(torch.int32), w.scales.view(torch.int32)) and torch.equal(g.zp, w.zp), f"call {i}: parameters"


# ---- 4. term counts ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 1, 16, 17, 33])
def test_reduce_term_counts_around_the_fusion_limit(pq, k):
    """reduce_quantize_grouped with every buffer aligned equals grouped dequantize ADD per term, in order, then quantize_grouped -- bytes, scales and
    zero points; and acc afterwards holds the surplus over 16 terms, the FIRST k - 16, which go in by grouped dequantize ADD before the rest is
    fused (no surplus: acc as it was)."""
    import piquant.torch as pt

    n, G, qdtype = 1000, 32, torch.quint4x2
    acc0 = _data(n, 31, torch.bfloat16)
    terms = _terms(n, G, k, qdtype, 400, torch.bfloat16)
    acc = acc0.clone()
    q, s, z = pt.reduce_quantize_grouped(acc, [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], dtype=qdtype, group_size=G)
    torch.cuda.synchronize()
    want_acc = acc0.clone()
    surplus = None
    for i, (raw, ts, tz) in enumerate(terms):
        if i == max(k - 16, 0):
            surplus = want_acc.clone()
        pt.dequantize_grouped(raw, ts, tz, dtype=torch.bfloat16, group_size=G, reduce_op="add", out=want_acc, quant_dtype=qdtype, shape=(n,))
    if surplus is None:
        surplus = want_acc.clone()
    wq, ws, wz = pt.quantize_grouped(want_acc, dtype=qdtype, group_size=G)
    torch.cuda.synchronize()
    assert torch.equal(s.view(torch.int32), ws.view(torch.int32)), "scales"
    assert torch.equal(z, wz), "zero points"
    assert torch.equal(_raw(q), _raw(wq)), "bytes"
    assert torch.equal(acc.view(torch.int16), surplus.view(torch.int16)), "acc: the surplus terms, and only they, are added into it"
