"""GPU: piquant_quantize / piquant_dequantize / piquant_compute_quant_params_* called with HOST pointers, at their seams, bit for bit.

How csrc/capi.cpp routes a call with a host buffer: both buffers pageable -> libpiquant_cpu.so (unless the call is per-element stochastic or the
context says 'stage'); one buffer pageable, per-element stochastic, or 'stage' -> the staging loop, 2^24 elements at a time on two alternating
stage slots; pinned host memory -> the HIP kernels, in place.  Cases, model and the proof that the cases notice a staging loop gone wrong:
tests/host_boundary_cases.py, tests/test_host_boundary_cases_cpu.py.

Every comparison is exact (helpers.same_floats for floats).  Every buffer a call writes has 0xAA guard bytes in front of it and behind it, on
the host and on the device, and every input is compared with what was put in.  All calls use the position-independent form (uniform=True): the
reference layout across staged chunks has its own tests (tests/test_gpu_parity.py).
"""
from functools import lru_cache

import numpy as np
import pytest

import host_boundary_cases as H
from helpers import same_floats

pytestmark = pytest.mark.gpu

C, N2, N3 = H.C, H.N2, H.N3
N_PINNED = 300_003
FILL = 0xAA


@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


@pytest.fixture(scope="module")
def contexts():
    import piquant
    import torch

    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    made = {}
    for path in ("stage", "auto"):
        made[path] = piquant.Context()
        made[path].set_host_path(path)
    return made


class Buf:
    """nbytes of pageable ('host'), pinned or device memory between guard bytes; the payload starts `misalign` bytes behind a 64-byte boundary"""

    def __init__(self, kind, nbytes, misalign=0):
        import torch

        total = nbytes + misalign + 3 * 64
        self.kind, self.nbytes = kind, nbytes
        if kind == "host":
            self.raw = np.full(total, FILL, dtype=np.uint8)
            addr = self.raw.ctypes.data
        elif kind == "pinned":
            self.t = torch.full((total,), FILL, dtype=torch.uint8).pin_memory()
            assert self.t.is_pinned()
            self.raw = self.t.numpy()
            addr = self.t.data_ptr()
        else:
            self.t = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
            addr = self.t.data_ptr()
        self.begin = (-addr) % 64 + 64 + misalign
        self.end = self.begin + nbytes
        self.ptr = addr + self.begin
        assert self.ptr % 64 == misalign % 64

    @property
    def view(self):
        return (self.t if self.kind == "device" else self.raw)[self.begin: self.end]

    def write(self, data):
        import torch

        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert data.size == self.nbytes
        if self.kind == "device":
            self.view.copy_(torch.from_numpy(np.array(data)))
        else:
            self.view[:] = data
        return self

    def write_in_flight(self, data, stream):
        """device only: the payload is produced by torch ops on `stream` that are still running when this returns"""
        import torch

        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        source = torch.from_numpy(np.array(data)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            self.view.fill_(0x55)
            self.view.copy_(source, non_blocking=True)
        self._keep = source
        return self

    def read(self, stream=None):
        import torch

        if self.kind != "device":
            return self.view.copy()
        if stream is None:
            return self.view.cpu().numpy()
        with torch.cuda.stream(stream):
            return self.view.cpu().numpy()

    def guards_intact(self):
        whole = self.t if self.kind == "device" else self.raw
        return bool((whole[: self.begin] == FILL).all()) and bool((whole[self.end:] == FILL).all())


def _types(dt):
    import piquant

    return piquant.DataType(dt)


class rounding_of:
    """sets the context's stochastic state for one call and puts the default back"""

    def __init__(self, ctx, rounding):
        self.ctx, self.rounding = ctx, rounding

    def __enter__(self):
        import piquant

        r = self.rounding
        if r[0] == "call":
            self.ctx.set_stochastic_threshold(r[1])
        elif r[0] == "element":
            self.ctx.set_stochastic_per_element(True, r[1], r[2])
        return piquant.RoundMode.NEAREST if r[0] == "nearest" else piquant.RoundMode.STOCHASTIC

    def __exit__(self, *exc):
        self.ctx.set_stochastic_threshold(None)
        self.ctx.set_stochastic_per_element(False)


def own_stream_blocking(ctx):
    ctx.reset_stream()
    ctx.set_blocking(True)
    return None


def on_stream(ctx, stream, blocking=False):
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(blocking)
    return stream


def run_quantize(ctx, x, dt_f, dt_q, rounding, kinds=("host", "host"), misalign=(0, 0), stream=None, in_flight=False, sync_before_read=False, params=None):
    """one quantize call; -> the output bytes.  misalign: (input, output) in BYTES off a 64-byte boundary.  Asserts guards and the unchanged input."""
    import torch

    scale, zp = H.QUANT_PARAMS[dt_q] if params is None else params
    xb = x.view(np.uint8).reshape(-1)
    src = Buf(kinds[0], xb.size, misalign[0])
    if in_flight:
        src.write_in_flight(xb, stream)
    else:
        src.write(xb)
    dst = Buf(kinds[1], H.packed(x.size, dt_q), misalign[1])
    with rounding_of(ctx, rounding) as mode:
        ctx.quantize_ptr(src.ptr, _types(dt_f), dst.ptr, _types(dt_q), x.size, scale, zp, mode, uniform=True)
    if sync_before_read:
        (stream or torch.cuda.current_stream()).synchronize()
    got = dst.read(stream)
    assert dst.guards_intact(), "the call wrote outside its output"
    assert src.guards_intact() and np.array_equal(src.read(stream), xb), "the call changed its input"
    return got


def run_dequantize(ctx, q, dt_q, dt_f, n, op, acc, kinds=("host", "host"), misalign=(0, 0), stream=None, in_flight=False, sync_before_read=False):
    """one dequantize call onto a copy of acc; -> the output as an array of the float type"""
    import piquant
    import torch

    scale, zp = H.DEQUANT_PARAMS[dt_q]
    src = Buf(kinds[0], q.size, misalign[0])
    if in_flight:
        src.write_in_flight(q, stream)
    else:
        src.write(q)
    dst = Buf(kinds[1], acc.nbytes, misalign[1]).write(acc)
    ctx.dequantize_ptr(src.ptr, _types(dt_q), dst.ptr, _types(dt_f), n, scale, zp, piquant.ReduceOp(op), uniform=True)
    if sync_before_read:
        (stream or torch.cuda.current_stream()).synchronize()
    got = dst.read(stream).view(H.NP_OF[dt_f])
    assert dst.guards_intact(), "the call wrote outside its output"
    assert src.guards_intact() and np.array_equal(src.read(stream), q), "the call changed its input"
    return got


# the models: one oracle call over the whole tensor each, shared by the tests that need the same one
@lru_cache(maxsize=4)
def want_quantize(n, dt_f, dt_q, rounding):
    return H.quantize_model(H.quant_input(n, dt_f, dt_q), dt_f, dt_q, rounding)


@lru_cache(maxsize=4)
def want_dequantize(n, dt_q, dt_f, op):
    return H.dequantize_model(H.codes_input(n, dt_q), dt_q, dt_f, n, op, H.accumulator(n, dt_f))


def quant_id(case):
    return "-".join(str(H.NAME.get(v, v[0] if isinstance(v, tuple) else v)) for v in case)


def dequant_id(form):
    return f"{H.NAME[form[0]]}-{H.NAME[form[1]]}-{'add' if form[2] else 'set'}"


def first_difference(got, want):
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else (int(d[0]), int(d.size))


# ---------------------------------------------------------------------------------------------------
# staged, both sides pageable
# ---------------------------------------------------------------------------------------------------
STAGED_QUANT = [(N2, f, q, r) for f, q in H.QUANT_PAIRS for r in (H.NEAREST, H.STOCHASTIC)] + [(N3, H.BF16, H.UINT2, H.NEAREST)]


@pytest.mark.parametrize("n,dt_f,dt_q,rounding", STAGED_QUANT, ids=[quant_id(c) for c in STAGED_QUANT])
def test_staged_quantize_across_the_seams(O, contexts, n, dt_f, dt_q, rounding):
    ctx = contexts["stage"]
    assert ctx.host_path_in_effect() == "stage"
    own_stream_blocking(ctx)
    got = run_quantize(ctx, H.quant_input(n, dt_f, dt_q), dt_f, dt_q, rounding)
    want = want_quantize(n, dt_f, dt_q, rounding)
    assert np.array_equal(got, want), first_difference(got, want)


STAGED_DEQUANT = [(N2,) + form for form in H.DEQUANT_FORMS] + [(N3, H.UINT4, H.BF16, 1)]


@pytest.mark.parametrize("n,dt_q,dt_f,op", STAGED_DEQUANT, ids=[f"{c[0]}-{dequant_id(c[1:])}" for c in STAGED_DEQUANT])
def test_staged_dequantize_across_the_seams(O, contexts, n, dt_q, dt_f, op):
    ctx = contexts["stage"]
    own_stream_blocking(ctx)
    got = run_dequantize(ctx, H.codes_input(n, dt_q), dt_q, dt_f, n, op, H.accumulator(n, dt_f))
    assert same_floats(got, want_dequantize(n, dt_q, dt_f, op))


# ---------------------------------------------------------------------------------------------------
# per-element stochastic rounding on host memory: always staged, the element index runs on across the seam (and across 2^32)
# ---------------------------------------------------------------------------------------------------
PER_ELEMENT = [(f, q, r) for f, q in ((H.F32, H.UINT8), (H.BF16, H.UINT4), (H.F32, H.UINT2)) for r in (H.PER_ELEMENT_BELOW, H.PER_ELEMENT)]


@pytest.mark.parametrize("dt_f,dt_q,rounding", PER_ELEMENT, ids=[f"{H.NAME[f]}-{H.NAME[q]}-base_2^32-C-{(1 << 32) - C - r[2]}" for f, q, r in PER_ELEMENT])
def test_per_element_rounding_on_host_memory_counts_across_the_seam(O, contexts, dt_f, dt_q, rounding):
    """index_base 2^32 - C - 5000 keeps the second chunk's indices just below 2^32; 2^32 - C - 2000 puts index 2^32 inside the second chunk.  The
    companion has no per-element mode: 'auto' must stage such a call too, and give the same bytes."""
    x = H.quant_input(N2, dt_f, dt_q)
    want = want_quantize(N2, dt_f, dt_q, rounding)
    for path in ("stage", "auto"):
        ctx = contexts[path]
        own_stream_blocking(ctx)
        got = run_quantize(ctx, x, dt_f, dt_q, rounding)
        assert np.array_equal(got, want), (path, first_difference(got, want))


# ---------------------------------------------------------------------------------------------------
# mixed residency: one side pageable, the other in device memory, addressed by the chunk's offset
# ---------------------------------------------------------------------------------------------------
MIXED_QUANT = [(H.F32, H.UINT4, H.NEAREST), (H.F32, H.UINT4, H.PER_ELEMENT)]
MIXED_DEQUANT = [(H.UINT8, H.BF16, 1), (H.UINT2, H.F32, 0)]
RESIDENCY = [("host", "device"), ("device", "host")]


@pytest.mark.parametrize("kinds", RESIDENCY, ids=["pageable_in-device_out", "device_in-pageable_out"])
@pytest.mark.parametrize("dt_f,dt_q,rounding", MIXED_QUANT, ids=[quant_id(c) for c in MIXED_QUANT])
def test_mixed_residency_quantize(O, contexts, dt_f, dt_q, rounding, kinds):
    """aligned, and with the device buffer one element (input) or one byte (output) off a 16-byte boundary, so the launch peels a head on top of
    the chunk's offset; a device input is still being produced on the context's stream when the call is made"""
    import torch

    x = H.quant_input(N2, dt_f, dt_q)
    want = want_quantize(N2, dt_f, dt_q, rounding)
    stream = torch.cuda.Stream()
    for off in (0, 1):
        misalign = (off * H.ESIZE[dt_f] if kinds[0] == "device" else 0, off if kinds[1] == "device" else 0)
        for path in ("auto", "stage"):
            ctx = contexts[path]
            on_stream(ctx, stream)
            got = run_quantize(ctx, x, dt_f, dt_q, rounding, kinds, misalign, stream, in_flight=kinds[0] == "device")
            assert np.array_equal(got, want), (path, off, first_difference(got, want))


@pytest.mark.parametrize("kinds", RESIDENCY, ids=["pageable_in-device_out", "device_in-pageable_out"])
@pytest.mark.parametrize("dt_q,dt_f,op", MIXED_DEQUANT, ids=[dequant_id(c) for c in MIXED_DEQUANT])
def test_mixed_residency_dequantize(O, contexts, dt_q, dt_f, op, kinds):
    import torch

    q, acc = H.codes_input(N2, dt_q), H.accumulator(N2, dt_f)
    want = want_dequantize(N2, dt_q, dt_f, op)
    stream = torch.cuda.Stream()
    for off in (0, 1):
        misalign = (off if kinds[0] == "device" else 0, off * H.ESIZE[dt_f] if kinds[1] == "device" else 0)
        for path in ("auto", "stage"):
            ctx = contexts[path]
            on_stream(ctx, stream)
            got = run_dequantize(ctx, q, dt_q, dt_f, N2, op, acc, kinds, misalign, stream, in_flight=kinds[0] == "device")
            assert same_floats(got, want), (path, off)


# ---------------------------------------------------------------------------------------------------
# pinned host memory: the HIP kernels read and write it in place
# ---------------------------------------------------------------------------------------------------
PINNED = [("pinned", "pinned", 0), ("pinned", "device", 0), ("pinned", "pinned", 1)]
PINNED_IDS = ["pinned_in-pinned_out", "pinned_in-device_out", "pinned_one_element_off"]


@lru_cache(maxsize=1)
def pinned_inputs():
    rng = np.random.default_rng(300_003)
    x = rng.uniform(-1, 1, N_PINNED).astype(np.float32)
    x[[0, 1, 2, 3, 4, N_PINNED - 1]] = np.array([2.5 * 2.0 ** -7, np.nan, np.inf, -np.inf, -0.0, 1e-40], dtype=np.float32)
    acc = rng.uniform(-3, 3, N_PINNED).astype(np.float32)
    acc[[0, 1, 2, N_PINNED - 1]] = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    return x, acc, rng.integers(0, 256, N_PINNED, dtype=np.uint8)


def pinned_context(contexts, blocking):
    """non-blocking on torch's stream (the result is read after the stream is synchronised), or blocking (the result is read from the host as it is)"""
    import torch

    ctx = contexts["auto"]
    on_stream(ctx, torch.cuda.current_stream(), blocking)
    return ctx


@pytest.mark.parametrize("blocking", [False, True], ids=["stream_ordered", "blocking"])
@pytest.mark.parametrize("kind_in,kind_out,off", PINNED, ids=PINNED_IDS)
def test_pinned_memory_quantize(O, contexts, kind_in, kind_out, off, blocking):
    ctx = pinned_context(contexts, blocking)
    x32 = pinned_inputs()[0]
    for dt_f, dt_q in H.QUANT_PAIRS:
        x = x32 if dt_f == H.F32 else O.f32_to_bf16(x32)
        got = run_quantize(ctx, x, dt_f, dt_q, H.NEAREST, (kind_in, kind_out), (off * H.ESIZE[dt_f], off), sync_before_read=not blocking)
        want = H.quantize_model(x, dt_f, dt_q, H.NEAREST)
        assert np.array_equal(got, want), (H.NAME[dt_f], H.NAME[dt_q], first_difference(got, want))


@pytest.mark.parametrize("blocking", [False, True], ids=["stream_ordered", "blocking"])
@pytest.mark.parametrize("kind_in,kind_out,off", PINNED, ids=PINNED_IDS)
def test_pinned_memory_dequantize(O, contexts, kind_in, kind_out, off, blocking):
    ctx = pinned_context(contexts, blocking)
    _, acc32, codes = pinned_inputs()
    for dt_q, dt_f, op in H.DEQUANT_FORMS:
        q = codes[: H.packed(N_PINNED, dt_q)]
        acc = acc32 if dt_f == H.F32 else O.f32_to_bf16(acc32)
        got = run_dequantize(ctx, q, dt_q, dt_f, N_PINNED, op, acc, (kind_in, kind_out), (off, off * H.ESIZE[dt_f]), sync_before_read=not blocking)
        assert same_floats(got, H.dequantize_model(q, dt_q, dt_f, N_PINNED, op, acc)), dequant_id((dt_q, dt_f, op))


def test_pinned_buffers_are_served_in_stream_order(O, contexts):
    """What tells "in place, by the HIP kernels" from a hand-over to the companion or the staging loop: a pinned input that a copy on the context's
    stream is still filling when the call is made (a few milliseconds of work queued in front of the copy).  A stream-ordered launch reads it after
    the copy, always; a host-side path would read the 0x55 it held before."""
    import piquant
    import torch

    ctx = contexts["auto"]
    stream = torch.cuda.Stream()
    on_stream(ctx, stream)
    x, acc, codes = pinned_inputs()
    q4 = codes[: H.packed(N_PINNED, H.UINT4)]
    accb = O.f32_to_bf16(acc)
    ballast = torch.zeros(1 << 28, dtype=torch.uint8, device="cuda")
    for payload, call, want in ((x.view(np.uint8), "quantize", H.quantize_model(x, H.F32, H.UINT8, H.NEAREST)),
                                (q4, "dequantize", H.dequantize_model(q4, H.UINT4, H.BF16, N_PINNED, 1, accb))):
        src = Buf("pinned", payload.size)
        src.view[:] = 0x55
        source = torch.from_numpy(np.array(payload)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(24):
                ballast.add_(1)
            src.t[src.begin: src.end].copy_(source, non_blocking=True)
        if call == "quantize":
            dst = Buf("pinned", N_PINNED)
            ctx.quantize_ptr(src.ptr, _types(H.F32), dst.ptr, _types(H.UINT8), N_PINNED, *H.QUANT_PARAMS[H.UINT8], piquant.RoundMode.NEAREST, uniform=True)
        else:
            dst = Buf("pinned", accb.nbytes).write(accb)
            ctx.dequantize_ptr(src.ptr, _types(H.UINT4), dst.ptr, _types(H.BF16), N_PINNED, *H.DEQUANT_PARAMS[H.UINT4], piquant.ReduceOp.ADD, uniform=True)
        stream.synchronize()
        assert np.array_equal(src.read(), payload) and src.guards_intact() and dst.guards_intact()
        got = dst.read()
        assert np.array_equal(got, want) if call == "quantize" else same_floats(got.view(np.uint16), want), call


# ---------------------------------------------------------------------------------------------------
# the staged scan: the extremes at and behind the seams, NaNs in between, the scan state left armed
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_min,pos_max", H.scan_pairs(N3), ids=[f"min_at_{a}-max_at_{b}" for a, b in H.scan_pairs(N3)])
@pytest.mark.parametrize("dt_f", [H.F32, H.BF16], ids=["fp32", "bf16"])
def test_staged_scan_finds_the_extremes_at_the_seams(O, contexts, dt_f, pos_min, pos_max):
    import piquant
    import torch

    ctx = contexts["stage"]
    own_stream_blocking(ctx)
    x = H.scan_input(N3, dt_f, pos_min, pos_max)
    before = x.copy()
    scan = ctx.compute_quant_params_ptr_float32 if dt_f == H.F32 else ctx.compute_quant_params_ptr_bfloat16
    target = (H.UINT8, H.UINT4, H.UINT2)[(pos_min + pos_max) % 3]
    assert scan(x.ctypes.data, piquant.DataType(target), N3) == H.scan_model(x, dt_f, target)
    assert np.array_equal(x.view(np.uint8), before.view(np.uint8)), "the scan changed its input"
    # a device scan on the same context directly afterwards: the state was left armed
    small = H.scan_input(N3, dt_f, pos_min, pos_max)[C - 50_001: C + 50_002]
    small[7] = np.float32(np.nan) if dt_f == H.F32 else 0x7FC0
    device = torch.from_numpy(small.view(np.int16 if dt_f == H.BF16 else np.float32)).cuda()
    assert scan(device.data_ptr(), piquant.DataType(target), small.size) == H.scan_model(small, dt_f, target)


# ---------------------------------------------------------------------------------------------------
# the companion behind the C ABI, at the sizes where its non-temporal stores switch on (4 MiB of output)
# ---------------------------------------------------------------------------------------------------
COMPANION = [("quantize", H.F32, H.UINT8, 4 * 2 ** 20 + 12_345), ("quantize", H.BF16, H.UINT4, 8 * 2 ** 20 + 12_345), ("dequantize", H.UINT8, H.F32, 2 ** 20 + 77)]


@pytest.mark.parametrize("kind,dt_a,dt_b,n", COMPANION, ids=[f"{k}-{H.NAME[a]}-{H.NAME[b]}-{n}" for k, a, b, n in COMPANION])
def test_companion_behind_the_c_abi_at_its_streaming_threshold(O, contexts, monkeypatch, kind, dt_a, dt_b, n):
    import piquant

    monkeypatch.setenv("PIQUANT_CPU_THREADS", "16")     # read when a context first hands a call to the companion
    rng = np.random.default_rng(n)
    if kind == "quantize":
        x = rng.uniform(-1, 1, n).astype(np.float32)
        x = x if dt_a == H.F32 else O.f32_to_bf16(x)
        want = H.quantize_model(x, dt_a, dt_b, H.NEAREST)
    else:
        q, acc = rng.integers(0, 256, H.packed(n, dt_a), dtype=np.uint8), rng.uniform(-3, 3, n).astype(np.float32)
        want = H.dequantize_model(q, dt_a, dt_b, n, 0, acc)
    results = {}
    for path in ("auto", "cpu", "stage"):
        ctx = piquant.Context()
        ctx.set_host_path(path)
        assert ctx.host_path_in_effect() == ("stage" if path == "stage" else "cpu")
        own_stream_blocking(ctx)
        if kind == "quantize":
            results[path] = run_quantize(ctx, x, dt_a, dt_b, H.NEAREST)
            assert np.array_equal(results[path], want), (path, first_difference(results[path], want))
        else:
            results[path] = run_dequantize(ctx, q, dt_a, dt_b, n, 0, acc)
            assert same_floats(results[path], want), path
    for path in ("auto", "cpu"):
        assert np.array_equal(results[path].view(np.uint8), results["stage"].view(np.uint8)), path
