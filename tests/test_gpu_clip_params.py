"""The histogram clip search for per-tensor parameters on the MI355X (piquant_hip_clip_histogram, piquant_hip_quant_params_from_histogram,
piquant_hip_compute_quant_params_clipped_device and the piquant.torch wrappers): the 8192 counts, all 63 error words, the choice and the 16 bytes of
the record bit for bit against the CPU model (tests/clip_params_model.py), which tests/test_clip_params_cpu.py shows to notice eight wrong variants (and why a ninth cannot show)
on the committed cases -- all of which run here.  Every device buffer the tests hand to a call carries guard bytes, the tensors of the torch-level tests
included (views of guarded buffers); what a wrapper allocates itself (a choice, an error vector) cannot.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import clip_params_model as M
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
ESIZE = {O.F32: 4, O.BF16: 2}
WIRES = (O.UINT8, O.UINT4, O.UINT2)


def kernel_constant(name):
    """an integer constant of the histogram pass, read from the kernel header itself: a retuned tile moves the sizes below with it"""
    text = (Path(__file__).resolve().parent.parent / "pi-quant_amd" / "csrc" / "clip_params_kernels.hpp").read_text()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


HIST_BLOCK, HIST_U, HIST_BLOCKS_PER_CU = kernel_constant("kClipHistBlock"), kernel_constant("kClipHistU"), kernel_constant("kClipHistBlocksPerCU")
TILE = {O.F32: HIST_BLOCK * HIST_U * 4, O.BF16: HIST_BLOCK * HIST_U * 8}   # elements of one block's round of 16-byte loads


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    return piquant.Context.get(0)


class Buf:
    """`nbytes` device bytes at a 16-byte boundary plus `shift`, GUARD bytes of 0xAA on both sides."""

    def __init__(self, nbytes, shift=0, data=None):
        self.whole = torch.full((GUARD + shift + nbytes + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.n = GUARD + shift, nbytes
        self.view = self.whole[self.lo: self.lo + nbytes]
        if data is not None and nbytes:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()))

    @property
    def ptr(self):
        return self.view.data_ptr() if self.n else self.whole.data_ptr() + self.lo

    def guards_ok(self):
        return bool((self.whole[: self.lo] == 0xAA).all()) and bool((self.whole[self.lo + self.n:] == 0xAA).all())

    def get(self, dtype=np.uint8):
        return self.view.cpu().numpy().view(dtype)


def attach(ctx):
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)


def one_call(ctx, x, dt_in, qd, steps, shift=0, xb=None):
    """-> (record bytes, choice, errors as uint64 words) of piquant_hip_compute_quant_params_clipped_device"""
    import piquant

    xb = xb or Buf(x.nbytes, shift, x)
    pb, cb, eb = Buf(16), Buf(4), Buf(63 * 8)
    attach(ctx)
    ctx.compute_quant_params_clipped_device_ptr(xb.ptr if x.size else 0, piquant.DataType(dt_in), x.size, piquant.DataType(qd), steps, pb.ptr, cb.ptr, eb.ptr,
                                                _device_ptrs=True)
    torch.cuda.synchronize()
    for b, what in ((xb, "x"), (pb, "record"), (cb, "choice"), (eb, "errors")):
        assert b.guards_ok(), f"wrote outside {what}"
    return pb.get().tobytes(), int(cb.get(np.int32)[0]), eb.get(np.uint64).copy()


def device_keys(ctx, x, dt_in, xb):
    import piquant

    kb = Buf(8)
    attach(ctx)
    ctx.minmax_keys_ptr(xb.ptr if x.size else 0, piquant.DataType(dt_in), x.size, kb.ptr, init=True, _device_ptrs=True)
    return kb


def three_calls(ctx, x, dt_in, qd, steps, shift=0, xb=None):
    """-> (counts, record bytes, choice, error words): keys, histogram and search as three calls on the caller's buffers"""
    import piquant

    xb = xb or Buf(x.nbytes, shift, x)
    kb = device_keys(ctx, x, dt_in, xb)
    hb, pb, cb, eb = Buf(8 * M.BINS), Buf(16), Buf(4), Buf(63 * 8)
    ctx.clip_histogram_ptr(xb.ptr if x.size else 0, piquant.DataType(dt_in), x.size, kb.ptr, hb.ptr, init=True, _device_ptrs=True)
    ctx.quant_params_from_histogram_ptr(kb.ptr, hb.ptr, piquant.DataType(qd), steps, pb.ptr, cb.ptr, eb.ptr)
    torch.cuda.synchronize()
    for b, what in ((xb, "x"), (kb, "keys"), (hb, "counts"), (pb, "record"), (cb, "choice"), (eb, "errors")):
        assert b.guards_ok(), f"wrote outside {what}"
    return hb.get(np.uint64).copy(), pb.get().tobytes(), int(cb.get(np.int32)[0]), eb.get(np.uint64).copy()


def plain_record(ctx, x, dt_in, qd, xb=None):
    import piquant

    xb = xb or Buf(x.nbytes, 0, x)
    pb = Buf(16)
    attach(ctx)
    ctx.compute_quant_params_device_ptr(xb.ptr if x.size else 0, piquant.DataType(dt_in), x.size, piquant.DataType(qd), pb.ptr, _device_ptrs=True)
    torch.cuda.synchronize()
    return pb.get().tobytes()


def want_of(x, dt_in, qd, steps):
    s, z, k, E, c = M.compute_quant_params_clipped(x, dt_in, qd, steps)
    return M.record_bytes(s, z), k, E.view(np.uint64), c


def check(ctx, x, dt_in, qd, steps, shift=0, what="", counts=True):
    rec, k, E, c = want_of(x, dt_in, qd, steps)
    xb = Buf(x.nbytes, shift, x)
    got = one_call(ctx, x, dt_in, qd, steps, xb=xb)
    assert got[1] == k, f"{what}: choice {got[1]} for {k}"
    assert np.array_equal(got[2], E), f"{what}: error words differ at {np.flatnonzero(got[2] != E)[:8]}"
    assert got[0] == rec, f"{what}: record {got[0].hex()} for {rec.hex()}"
    if counts:
        gc, grec, gk, gE = three_calls(ctx, x, dt_in, qd, steps, xb=xb)
        assert np.array_equal(gc, c), f"{what}: counts differ at bins {np.flatnonzero(gc != c)[:8]}: {gc[gc != c][:8]} for {c[gc != c][:8]}"
        assert (grec, gk) == (rec, k) and np.array_equal(gE, E), f"{what}: the three-call form differs from the one-call form"
    return rec, k


def guarded(data=None, nbytes=None, dtype=torch.uint8):
    """-> (Buf, 1-D tensor of `dtype` that is a view of its bytes): a torch tensor with guard bytes on both sides"""
    b = Buf(nbytes if data is None else data.nbytes, 0, data)
    return b, b.view.view(dtype)


def quantize_dp(t, params, tq, out=None):
    """piquant_hip_quantize_dp on torch tensors, on the current stream"""
    import piquant
    import piquant.torch as pt

    out = torch.empty(t.shape, dtype=tq, device=t.device) if out is None else out
    pt._ctx_for(t, None).quantize_dp_ptr(t.data_ptr(), pt.torch_to_piquant_dtype(t.dtype), out.data_ptr(), pt.torch_to_piquant_dtype(tq), t.numel(),
                                         params.data_ptr(), piquant.RoundMode.NEAREST, _device_ptrs=True)
    return out


def gaussian(n, seed, dt_in):
    v = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    return M.as_input(v, dt_in)


@pytest.mark.parametrize("dt_in", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_small_sizes_and_one_block_tile(ctx, dt_in):
    for i, n in enumerate((0, 1, 3, 4, 5, 63, 64, 65, 8191, 8193, TILE[dt_in] - 1, TILE[dt_in], TILE[dt_in] + 1)):
        x = gaussian(n, 100 + i, dt_in)
        for qd in WIRES:
            check(ctx, x, dt_in, qd, 63, what=f"n={n} wire={qd}", counts=qd == O.UINT2)


@pytest.mark.parametrize("dt_in", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_three_trips_of_every_block_and_a_ragged_tail(ctx, dt_in):
    blocks = HIST_BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count   # the grid's cap: one row of the scratch per block
    n = 3 * blocks * TILE[dt_in] + TILE[dt_in] // 2 + 5
    x = gaussian(n, 3, dt_in)
    _, k = check(ctx, x, dt_in, O.UINT4, 63, what=f"n={n}")
    assert k > 0
    check(ctx, x[1:], dt_in, O.UINT2, 63, shift=ESIZE[dt_in], what=f"n={n - 1}, one element off")


@pytest.mark.parametrize("steps", [1, 2, 17, 63])
@pytest.mark.parametrize("dt_in,qd", [(O.F32, O.UINT8), (O.F32, O.UINT2), (O.BF16, O.UINT4)])
def test_steps(ctx, dt_in, qd, steps):
    x = gaussian(50_000 + 3, 11, dt_in)
    rec, k = check(ctx, x, dt_in, qd, steps, what=f"steps={steps}")
    assert k < steps
    if steps == 1:
        assert (rec, k) == (plain_record(ctx, x, dt_in, qd), 0)


@pytest.mark.parametrize("dt_in", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_one_element_off_a_16_byte_boundary(ctx, dt_in):
    for n in (1, 2, 7, 9, 4099, TILE[dt_in] + 3):
        x = gaussian(n, 20 + n % 7, dt_in)
        for qd in (O.UINT4, O.UINT2):
            check(ctx, x, dt_in, qd, 63, shift=ESIZE[dt_in], what=f"n={n} shifted")


EDGES = M.edge_tensors()


@pytest.mark.parametrize("dt_in", [O.F32, O.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edge_tensors(ctx, i, dt_in):
    name, v = EDGES[i]
    x = M.as_input(v, dt_in)
    if name == "tie" and dt_in == O.F32:
        lo, hi = M.minmax(x, dt_in)
        M.assert_tie(lo, hi, M.histogram(x, dt_in, lo, hi), O.UINT2, 63, M.TIE_KS)
    for qd in WIRES:
        for steps in (63, 17):
            rec, k = check(ctx, x, dt_in, qd, steps, what=f"{name} wire={qd} steps={steps}")
            if name in ("constant", "all_nan"):
                assert (rec, k) == (plain_record(ctx, x, dt_in, qd), 0)
        check(ctx, x, dt_in, qd, 63, shift=ESIZE[dt_in], what=f"{name} wire={qd} shifted")


@pytest.mark.parametrize("qd", WIRES)
def test_the_empty_tensor_is_the_plain_call(ctx, qd):
    x = np.zeros(0, dtype=np.float32)
    for steps in (1, 63):
        rec, k, E = one_call(ctx, x, O.F32, qd, steps)
        assert (rec, k) == (plain_record(ctx, x, O.F32, qd), 0) and np.isnan(E.view(np.float64)).all()


def test_histogram_over_two_shards_accumulates_to_the_whole(ctx):
    import piquant

    for dt_in in (O.F32, O.BF16):
        x = gaussian(70_001, 31, dt_in)
        cut = 23_457                                      # the second shard starts off a 16-byte boundary
        xb = Buf(x.nbytes, 0, x)
        kb = device_keys(ctx, x, dt_in, xb)
        whole, parts = Buf(8 * M.BINS), Buf(8 * M.BINS)
        dt = piquant.DataType(dt_in)
        ctx.clip_histogram_ptr(xb.ptr, dt, x.size, kb.ptr, whole.ptr, init=True, _device_ptrs=True)
        ctx.clip_histogram_ptr(xb.ptr, dt, cut, kb.ptr, parts.ptr, init=True, _device_ptrs=True)
        ctx.clip_histogram_ptr(xb.ptr + cut * ESIZE[dt_in], dt, x.size - cut, kb.ptr, parts.ptr, init=False, _device_ptrs=True)
        ctx.clip_histogram_ptr(0, dt, 0, kb.ptr, parts.ptr, init=False, _device_ptrs=True)   # nothing to add
        torch.cuda.synchronize()
        assert whole.guards_ok() and parts.guards_ok() and xb.guards_ok()
        lo, hi = M.minmax(x, dt_in)
        assert np.array_equal(whole.get(np.uint64), M.histogram(x, dt_in, lo, hi))
        assert np.array_equal(parts.get(np.uint64), whole.get(np.uint64))


@pytest.mark.parametrize("dt_in,qd,tq", [(O.F32, O.UINT2, "quint2x4"), (O.BF16, O.UINT4, "quint4x2"), (O.F32, O.UINT8, "quint8")])
def test_the_record_drives_quantize_dp_and_dequantize_dp_to_the_oracles_bytes(ctx, dt_in, qd, tq):
    import piquant.torch as pt

    n = 40_003
    x = gaussian(n, 41, dt_in)
    tdt = torch.bfloat16 if dt_in == O.BF16 else torch.float32
    xb, t = guarded(x, dtype=tdt)
    pb, own = guarded(nbytes=16)
    qb, qout = guarded(nbytes=O.packed_numel(n, qd))
    db, dout = guarded(nbytes=x.nbytes, dtype=tdt)
    params, choice = pt.compute_quant_params_clipped_device(t, dtype=getattr(torch, tq), out=own, return_choice=True)
    assert params is own
    s, z, k, _, _ = M.compute_quant_params_clipped(x, dt_in, qd, 63)
    assert params.cpu().numpy().tobytes() == M.record_bytes(s, z) and int(choice.cpu()[0]) == k
    assert pt.compute_quant_params_clipped(t, dtype=getattr(torch, tq)) == (float(s), z)
    quantize_dp(t, params, getattr(torch, tq), out=qout)
    want_q = O.quantize(x, dt_in, qd, float(s), z)
    assert np.array_equal(qout.cpu().numpy(), want_q)
    d = pt.dequantize_dynamic(qout, params, dtype=t.dtype, out=dout, quant_dtype=getattr(torch, tq), shape=(n,))
    want_d = O.dequantize(want_q, qd, dt_in, n, float(s), z)
    got_d = d.view(torch.int16).cpu().numpy().view(np.uint16) if dt_in == O.BF16 else d.cpu().numpy()
    assert np.array_equal(got_d.view(np.uint8), want_d.view(np.uint8))
    assert all(b.guards_ok() for b in (xb, pb, qb, db))


def test_graph_capture_replayed_on_changed_data(ctx):
    import piquant.torch as pt

    n = 100_000 + 77
    a, b = gaussian(n, 51, O.F32), (gaussian(n, 52, O.F32) * np.float32(3.0) + np.float32(1.0)).astype(np.float32)
    xb, x = guarded(a, dtype=torch.float32)
    pb, gp = guarded(nbytes=16)
    qb, gq = guarded(nbytes=O.packed_numel(n, O.UINT4))
    quantize_dp(x, pt.compute_quant_params_clipped_device(x, dtype=torch.quint4x2), torch.quint4x2, out=gq)   # eager warm-up (scratch, code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gc = pt.compute_quant_params_clipped_device(x, dtype=torch.quint4x2, out=gp, return_choice=True)
        quantize_dp(x, gp, torch.quint4x2, out=gq)
    for v in (b, a):
        x.copy_(torch.from_numpy(v).cuda())
        gp.zero_()
        gc.fill_(99)
        graph.replay()
        torch.cuda.synchronize()
        s, z, k, _, _ = M.compute_quant_params_clipped(v, O.F32, O.UINT4, 63)
        assert gp.cpu().numpy().tobytes() == M.record_bytes(s, z) and int(gc.cpu()[0]) == k
        assert np.array_equal(gq.cpu().numpy(), O.quantize(v, O.F32, O.UINT4, float(s), z))
        eager = pt.compute_quant_params_clipped_device(x, dtype=torch.quint4x2)
        assert torch.equal(eager, gp)
        assert all(b.guards_ok() for b in (xb, pb, qb))


def test_torch_wrappers_and_argument_checks(ctx):
    import piquant.distributed as pd
    import piquant.torch as pt

    x = gaussian(30_000, 61, O.F32)
    xb, t = guarded(x, dtype=torch.float32)
    hb, hist_own = guarded(nbytes=8 * M.BINS, dtype=torch.int64)
    pb, own = guarded(nbytes=16)
    keys = pd.local_minmax_keys(t)
    hist = pt.clip_histogram(t, keys, out=hist_own)
    assert hist is hist_own
    lo, hi = M.minmax(x, O.F32)
    c = M.histogram(x, O.F32, lo, hi)
    assert hist.dtype == torch.int64 and np.array_equal(hist.cpu().numpy().view(np.uint64), c)
    twice = pt.clip_histogram(t, keys, out=hist.clone(), accumulate=True)
    assert np.array_equal(twice.cpu().numpy().view(np.uint64), 2 * c)
    params, choice, errors = pt.quant_params_from_histogram(keys, hist, dtype=torch.quint2x4, steps=40, return_choice=True, return_errors=True)
    s, z, k, E = M.search(lo, hi, c, O.UINT2, 40)
    assert params.cpu().numpy().tobytes() == M.record_bytes(s, z) and int(choice.cpu()[0]) == k
    assert np.array_equal(errors.cpu().numpy().view(np.uint64), E.view(np.uint64))
    assert torch.equal(pt.quant_params_from_histogram(keys, hist, dtype=torch.quint2x4, steps=40), params)
    assert pt.compute_quant_params_clipped_device(t, dtype=torch.quint2x4, steps=40, out=own) is own and torch.equal(own, params)
    torch.cuda.synchronize()
    assert all(b.guards_ok() for b in (xb, hb, pb))

    calls = (lambda **kw: pt.compute_quant_params_clipped_device(t, **{"dtype": torch.quint2x4, **kw}),
             lambda **kw: pt.compute_quant_params_clipped(t, **{"dtype": torch.quint2x4, **kw}),
             lambda **kw: pt.quant_params_from_histogram(keys, hist, **{"dtype": torch.quint2x4, **kw}),
             lambda **kw: pd.compute_quant_params_clipped(t, **{"dtype": torch.quint2x4, **kw}))
    for call in calls:
        for bad in (0, 64, -1, 2.0, True, None, "9"):
            with pytest.raises(ValueError, match="steps"):
                call(steps=bad)
        with pytest.raises(ValueError, match="quantized dtype"):
            call(dtype=torch.float32)
    for bad_shard in (t.cpu(), t.to(torch.float16)):   # refused before the scan is launched and before any collective is entered
        with pytest.raises(ValueError, match="tensor"):
            pd.compute_quant_params_clipped(bad_shard, dtype=torch.quint2x4)
    with pytest.raises(ValueError):
        pt.compute_quant_params_clipped_device(t.cpu(), dtype=torch.quint2x4)
    with pytest.raises(ValueError):
        pt.compute_quant_params_clipped_device(t.to(torch.float16), dtype=torch.quint2x4)
    with pytest.raises(ValueError, match="out"):
        pt.compute_quant_params_clipped_device(t, dtype=torch.quint2x4, out=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        pt.compute_quant_params_clipped_device(t, dtype=torch.quint2x4, out=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="tensor"):
        pt.clip_histogram(t.to(torch.float16), keys)
    with pytest.raises(ValueError, match="tensor"):
        pt.clip_histogram(t.cpu(), keys)
    for bad_keys in (keys.cpu(), keys.to(torch.int64), torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(1, 2, dtype=torch.int32, device="cuda"), None):
        with pytest.raises(ValueError, match="keys"):
            pt.clip_histogram(t, bad_keys)
        with pytest.raises(ValueError, match="keys"):
            pt.quant_params_from_histogram(bad_keys, hist, dtype=torch.quint2x4)
    for bad_hist in (hist.cpu(), hist.to(torch.int32), torch.zeros(M.BINS + 1, dtype=torch.int64, device="cuda"), torch.zeros(2, M.BINS // 2, dtype=torch.int64, device="cuda"), None):
        with pytest.raises(ValueError, match="hist"):
            pt.quant_params_from_histogram(keys, bad_hist, dtype=torch.quint2x4)
        if bad_hist is not None:
            with pytest.raises(ValueError, match="out"):
                pt.clip_histogram(t, keys, out=bad_hist)
    with pytest.raises(ValueError, match="accumulate"):
        pt.clip_histogram(t, keys, accumulate=True)


@pytest.mark.parametrize("dt_in", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_input_that_is_not_even_element_aligned(ctx, dt_in):
    """one byte off: the histogram pass goes element by element (and the scan takes its scalar kernel), over more than one trip of the grid"""
    blocks = HIST_BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    for n in (1, 5, 4099, 2 * blocks * HIST_BLOCK + 77):
        x = gaussian(n, 70 + n % 5, dt_in)
        check(ctx, x, dt_in, O.UINT4, 63, shift=1, what=f"n={n}, one byte off")


def test_stand_alone_calls_on_two_streams_share_the_contexts_scratch_in_order(ctx):
    """a large tensor's histogram and search on stream A, a small one's on stream B right behind: B's launches must wait for A's, whose rows and
    errors lie in the same scratch of the context -- both against the model; then the one-call form on A followed by the stand-alone calls on B"""
    import piquant

    dt = piquant.DataType.F32
    big, small = gaussian(20_000_003, 81, O.F32), (gaussian(3_001, 82, O.F32) * np.float32(0.25) + np.float32(2.0)).astype(np.float32)
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    sets = []
    for x in (big, small):
        xb = Buf(x.nbytes, 0, x)
        sets.append((x, xb, device_keys(ctx, x, O.F32, xb), Buf(8 * M.BINS), Buf(16), Buf(4), Buf(63 * 8), Buf(16)))
    torch.cuda.synchronize()
    wants = [want_of(x, O.F32, O.UINT2, 63) for x in (big, small)]
    for one_call_first in (False, True):
        for (x, xb, kb, hb, pb, cb, eb, ob), stream in zip(sets, streams):
            with torch.cuda.stream(stream):
                attach(ctx)
                if one_call_first and x is big:
                    ctx.compute_quant_params_clipped_device_ptr(xb.ptr, dt, x.size, piquant.DataType.UINT2, 63, ob.ptr, _device_ptrs=True)
                ctx.clip_histogram_ptr(xb.ptr, dt, x.size, kb.ptr, hb.ptr, init=True, _device_ptrs=True)
                ctx.quant_params_from_histogram_ptr(kb.ptr, hb.ptr, piquant.DataType.UINT2, 63, pb.ptr, cb.ptr, eb.ptr)
        torch.cuda.synchronize()
        for (x, xb, kb, hb, pb, cb, eb, ob), (rec, k, E, c) in zip(sets, wants):
            assert all(b.guards_ok() for b in (xb, kb, hb, pb, cb, eb, ob))
            assert np.array_equal(hb.get(np.uint64), c), f"counts of the {x.size}-element tensor differ at bins {np.flatnonzero(hb.get(np.uint64) != c)[:8]}"
            assert (pb.get().tobytes(), int(cb.get(np.int32)[0])) == (rec, k) and np.array_equal(eb.get(np.uint64), E)
            if one_call_first and x is big:
                assert ob.get().tobytes() == rec
            for b in (hb, pb, cb, eb):
                b.view.fill_(0x55)
    attach(ctx)
