"""GPU: the HIP path against the oracle, bit for bit, through the C ABI of libpiquant.so.

Every call goes piquant.Context.*_ptr -> ctypes -> libpiquant.so -> HIP kernel on device pointers (or host
pointers for the staging tests).  The expected values come from the oracle's FORM_UNIFORM (the position-
independent formula the kernels implement) and from the committed vectors produced by the reference's own
kernels.  Integer outputs must be identical; float outputs must be bit-identical (any-NaN == any-NaN).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from helpers import gpu_dequantize, gpu_quantize, load_golden, same_floats, to_device

pytestmark = pytest.mark.gpu

N1 = 27_264_000   # BASELINE.json configs 1-4


@pytest.fixture(scope="module")
def ctx():
    import piquant
    import torch

    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    c = piquant.Context()
    c.set_reference_layout(False)   # this module's tests pin the position-independent kernels unless they switch the layout on themselves (the default-mode tests make their own contexts)
    return c


@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


# quantize tiles are 512 or 1024 elements (64- or 128-thread blocks, two 16-byte vectors per lane: csrc/tuning.hpp); 1024, 4096 and 8192 elements are
# dequantize's tiles.  Boundaries around all of them, odd and ragged sizes
SIZES = [1, 2, 3, 5, 63, 64, 65, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 65536 + 17, 1_000_003]


# ---------------------------------------------------------------------------------------------------
# golden vectors (outputs of the reference's own kernels)
# ---------------------------------------------------------------------------------------------------
def test_golden_quantize(ctx):
    cases, get = load_golden()
    n = 0
    for c in cases:
        if c["kind"] != "quantize":
            continue
        ctx.set_stochastic_threshold(c["tau"] if c["round_mode"] else None)
        got = gpu_quantize(ctx, get(c["name"], "x"), c["dt_in"], c["dt_out"], c["scale"], c["zp"], c["round_mode"])
        assert np.array_equal(got, get(c["name"], "uniform")), c
        n += 1
    ctx.set_stochastic_threshold(None)
    assert n > 500


def test_golden_dequantize(ctx):
    cases, get = load_golden()
    n = 0
    for c in cases:
        if c["kind"] != "dequantize":
            continue
        got = gpu_dequantize(ctx, get(c["name"], "q"), c["dt_in"], c["dt_out"], c["numel"], c["scale"], c["zp"], c["op"],
                             prev=get(c["name"], "prev"))
        assert same_floats(got, get(c["name"], "uniform")), c
        n += 1
    assert n > 400


def test_golden_minmax(ctx):
    import piquant

    cases, get = load_golden()
    for c in cases:
        if c["kind"] != "minmax":
            continue
        for field, dt, lo, hi in (("x", piquant.DataType.F32, c["min_f32"], c["max_f32"]), ("xb", piquant.DataType.BF16, c["min_bf16"], c["max_bf16"])):
            _, ptr = keep = to_device(get(c["name"], field))
            import torch

            keys = torch.empty(2, dtype=torch.int32, device="cuda")
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.minmax_keys_ptr(ptr, dt, c["numel"], keys.data_ptr(), init=True)
            k = keys.cpu()
            assert piquant.decode_minmax_keys(int(k[0]), int(k[1])) == (lo, hi), c
            del keep


# ---------------------------------------------------------------------------------------------------
# randomized parity, all 12 + 12 combinations
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_in", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("dt_out", [4, 3, 2], ids=["u8", "u4", "u2"])
@pytest.mark.parametrize("round_mode", [0, 1], ids=["nearest", "stochastic"])
def test_quantize_random(ctx, O, dt_in, dt_out, round_mode):
    rng = np.random.default_rng(100 * dt_in + 10 * dt_out + round_mode)
    qmax = {4: 255, 3: 15, 2: 3}[dt_out]
    for n in SIZES:
        x = rng.uniform(-1, 1, n).astype(np.float32)
        if n > 100:
            x[rng.choice(n, 6, replace=False)] = [np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0]
        xin = x if dt_in == 0 else O.f32_to_bf16(x)
        scale = float(np.float32(2.0 / qmax))
        for zp in (qmax // 2, -3, qmax + 10):
            tau = float(rng.uniform(0, 1)) if round_mode else 0.0
            ctx.set_stochastic_threshold(tau if round_mode else None)
            got = gpu_quantize(ctx, xin, dt_in, dt_out, scale, zp, round_mode)
            want = O.quantize(xin, dt_in, dt_out, scale, zp, round_mode, tau, form=O.FORM_UNIFORM)
            assert np.array_equal(got, want), (n, zp, np.nonzero(got != want)[0][:5])
    ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("dt_q", [4, 3, 2], ids=["u8", "u4", "u2"])
@pytest.mark.parametrize("dt_f", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("op", [0, 1], ids=["set", "add"])
def test_dequantize_random(ctx, O, dt_q, dt_f, op):
    rng = np.random.default_rng(1000 + 100 * dt_q + 10 * dt_f + op)
    for n in SIZES:
        q = rng.integers(0, 256, O.packed_numel(n, dt_q)).astype(np.uint8)
        prev = rng.uniform(-4, 4, n).astype(np.float32)
        prev = prev if dt_f == 0 else O.f32_to_bf16(prev)
        for scale, zp in ((0.0078431377, 127), (0.37, -5), (1e-3, 300)):
            got = gpu_dequantize(ctx, q, dt_q, dt_f, n, scale, zp, op, prev=prev)
            want = O.dequantize(q, dt_q, dt_f, n, scale, zp, op, form=O.FORM_UNIFORM, out=prev.copy())
            assert same_floats(got, want), (n, scale, zp)


def _fuzz_values(rng, n):
    """floats over the whole exponent range plus specials: denormals, +-0, +-inf, NaN, integers, half-way cases"""
    bits = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32).copy()
    k = max(1, n // 8)
    x[rng.choice(n, k)] = rng.integers(-300, 300, k).astype(np.float32) + np.float32(0.5)
    x[rng.choice(n, k)] = rng.uniform(-4, 4, k).astype(np.float32)
    x[rng.choice(n, min(n, 6))] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45], np.float32)[: min(n, 6)]
    return x


def test_fuzz_all_pairs_over_the_whole_float_range(ctx, O):
    """300 random configurations: any fp32 bit pattern as input, scales from 1e-30 to 1e30, zero points from the whole
    int64 range, every dtype pair / rounding mode / store op, ragged sizes -- the HIP result must equal the oracle bit for bit."""
    rng = np.random.default_rng(2025)
    for it in range(300):
        n = int(rng.integers(1, 20_000))
        x = _fuzz_values(rng, n)
        scale = float(np.float32(10.0 ** rng.uniform(-30, 30)))
        zp = int(rng.integers(-2**63, 2**63 - 1)) if it % 3 == 0 else int(rng.integers(-300, 300))
        dt_f = int(rng.integers(0, 2))
        dt_q = int(rng.integers(2, 5))
        xin = x if dt_f == 0 else O.f32_to_bf16(x)
        rm = int(rng.integers(0, 2))
        tau = float(rng.uniform(0, 1)) if rm else 0.0
        ctx.set_stochastic_threshold(tau if rm else None)
        got = gpu_quantize(ctx, xin, dt_f, dt_q, scale, zp, rm)
        want = O.quantize(xin, dt_f, dt_q, scale, zp, rm, tau)
        assert np.array_equal(got, want), ("quantize", it, n, scale, zp, dt_f, dt_q, rm, np.nonzero(got != want)[0][:4])
        op = int(rng.integers(0, 2))
        q = rng.integers(0, 256, O.packed_numel(n, dt_q)).astype(np.uint8)
        prev = _fuzz_values(rng, n) if it % 2 else rng.uniform(-5, 5, n).astype(np.float32)
        prev = prev if dt_f == 0 else O.f32_to_bf16(prev)
        got = gpu_dequantize(ctx, q, dt_q, dt_f, n, scale, zp, op, prev=prev)
        want = O.dequantize(q, dt_q, dt_f, n, scale, zp, op, out=prev.copy())
        assert same_floats(got, want), ("dequantize", it, n, scale, zp, dt_q, dt_f, op)
    ctx.set_stochastic_threshold(None)


def test_stochastic_short_step_edges(ctx, O):
    """The stochastic step has a float-domain short form (quant_kernels.hpp quantize_vec_bounded_stochastic) taken per wave tile when the
    zero point lies inside the quantized range and max|x| * |1/scale| < 1e9.  Its corners against the oracle's int64 form: fractional
    parts equal to the threshold (not above: no step), threshold 0 (every fraction steps away from zero), -0.0, integers at and above
    2^24 (no fraction left), products just below and just above 1e9 (the second sends its whole tile through the long step), NaN and
    infinities in otherwise ordinary tiles, zero points at both ends of the range and just outside it."""
    rng = np.random.default_rng(4242)
    n = 64 * 1024 + 37
    base = rng.uniform(-300, 300, n).astype(np.float32)
    frac = np.float32(0.375)
    base[::7] = np.trunc(base[::7]) + np.copysign(frac, base[::7])          # |r - trunc r| == 0.375 exactly at scale 1
    base[1::97] = np.float32(-0.0)
    base[2::101] = np.float32(16777216.0)
    base[3::103] = np.float32(-16777217.0)
    base[4::107] = np.float32(0.99999994)
    base[5::109] = np.float32(-0.99999994)
    cases = {"ordinary": base.copy()}
    for name, val in (("below_1e9", 9.9999994e8), ("above_1e9", 1.0000001e9), ("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf), ("huge", 3.0e38)):
        y = base.copy()
        y[rng.choice(n, 9)] = np.float32(val)
        cases[name] = y
    for name, x in cases.items():
        xb = O.f32_to_bf16(x)
        for dt_in, xin in ((0, x), (1, xb)):
            for dt_out, qmax in ((4, 255), (3, 15), (2, 3)):
                for zp in (0, qmax // 2, qmax, -1, qmax + 1):
                    for scale in (1.0, 0.5, 3.0):
                        for tau in (0.0, 0.375, 0.37499997, 0.99999994):
                            ctx.set_stochastic_threshold(tau)
                            got = gpu_quantize(ctx, xin, dt_in, dt_out, scale, zp, 1)
                            want = O.quantize(xin, dt_in, dt_out, scale, zp, 1, tau)
                            assert np.array_equal(got, want), (name, dt_in, dt_out, zp, scale, tau, np.nonzero(got != want)[0][:4])
    ctx.set_stochastic_threshold(None)
    # the per-element thresholds take the same short step
    import piquant
    x = cases["ordinary"]
    for dt_out in (4, 3, 2):
        ctx.set_stochastic_per_element(True, seed=0xfeed, index_base=(1 << 32) - 5000)
        got = gpu_quantize(ctx, x, 0, dt_out, 0.5, 1, 1)
        ctx.set_stochastic_per_element(False)
        assert np.array_equal(got, O.quantize_per_element(x, O.F32, dt_out, 0.5, 1, 0xfeed, (1 << 32) - 5000))


def gpu_compute_params(ctx, x, dt_in, dt_q):
    """piquant_compute_quant_params_* on a device copy of x -> (scale, zero_point)"""
    import piquant
    import torch

    keep, ptr = to_device(x)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    fn = ctx.compute_quant_params_ptr_float32 if dt_in == 0 else ctx.compute_quant_params_ptr_bfloat16
    got = fn(ptr, piquant.DataType(dt_q), x.size)
    del keep
    return got


def test_signaling_nans_do_not_poison_range_tests_or_scans(ctx, O):
    """Found by the parity soak (seed 777, iteration 110 308: one byte of 1.5 M).  v_min/v_max skip a QUIET NaN, but kernels run in IEEE mode, where
    a SIGNALING NaN operand turns the result into a NaN -- which the next min/max then skips together with everything folded before it.  So
    (a) the short step's range test forgot a value beyond 10^9 * scale that was followed, in the same lane, by a signaling NaN, and the tile
    took the short step (255 where the reference's cvttps2dq indefinite gives 0); (b) a min/max scan forgot its running extremes after a
    signaling NaN.  np.nan is quiet, which is why the NaN tests above never saw it; an fp32 bit-pattern fuzz draws both kinds."""
    import piquant
    rng = np.random.default_rng(110308)
    SNAN32, SNAN16 = 0x7f800001, 0x7f81
    # (a) quantize: a huge value first, signaling NaNs later in the same lane's elements (element 4l..4l+3 of vector l, then vector 64 + l, ...)
    for dt_in in (0, 1):
        for dt_out, qmax in ((4, 255), (3, 15), (2, 3)):
            for rm, tau in ((0, 0.0), (1, 0.3)):
                n = 64 * 1024 + 3
                x = rng.uniform(-100, 100, n).astype(np.float32)
                xin = x if dt_in == 0 else O.f32_to_bf16(x)
                bits = xin.view(np.uint32) if dt_in == 0 else xin.view(np.uint16)
                huge = np.array([3.0e9, -3.0e9, 2.6e38], dtype=np.float32)
                hb = huge.view(np.uint32) if dt_in == 0 else O.f32_to_bf16(huge).view(np.uint16)
                epv = 4 if dt_in == 0 else 8
                for j, lane in enumerate(rng.choice(4000, 60, replace=False)):
                    base = int(lane) * epv
                    bits[base] = hb[j % 3]                                   # first element of the lane's first vector
                    bits[base + 2 + (j % (epv - 2))] = SNAN32 if dt_in == 0 else SNAN16   # a later element of the same vector ...
                    if j % 2:
                        bits[base + 64 * epv + (j % epv)] = SNAN32 if dt_in == 0 else SNAN16   # ... or of the lane's next vector
                ctx.set_stochastic_threshold(tau if rm else None)
                for scale, zp in ((1.0, qmax // 2), (0.5, 0), (1.0e-3, qmax)):
                    got = gpu_quantize(ctx, xin, dt_in, dt_out, scale, zp, rm)
                    want = O.quantize(xin, dt_in, dt_out, scale, zp, rm, tau)
                    assert np.array_equal(got, want), (dt_in, dt_out, rm, scale, zp, np.nonzero(got != want)[0][:6])
    ctx.set_stochastic_threshold(None)
    # the block the soak tripped over, as data: elements [129 024, 130 048) of its 1 504 358-element fp32 tensor (uint32 bit patterns), scale 9.33e28, zp 105
    from pathlib import Path
    blk = np.load(Path(__file__).resolve().parent / "golden" / "soak_seed777_it110308_block126_f32.npy").view(np.float32)
    for lead in (0, 1024, 129_024):       # at the front, behind one ordinary block, and where it sat
        xs = np.concatenate([rng.uniform(-1, 1, lead).astype(np.float32), blk, rng.uniform(-1, 1, 102).astype(np.float32)])
        got = gpu_quantize(ctx, xs, 0, 4, 9.331063715550025e+28, 105, 0)
        assert np.array_equal(got, O.quantize(xs, 0, 4, 9.331063715550025e+28, 105)), lead
    # quieting an input must not flush it: a tensor of denormals scans to denormal extremes
    import torch
    den = np.array([3, 1, 7, 0x80000005, 0x80000002, 4] * 700, dtype=np.uint32).view(np.float32)
    keep, ptr = to_device(den)
    keys_d = torch.empty(2, dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.minmax_keys_ptr(ptr, piquant.DataType.F32, den.size, keys_d.data_ptr(), True)
    k = keys_d.cpu().numpy()
    lo, hi = piquant.decode_minmax_keys(int(k[0]), int(k[1]))
    assert np.float32(lo).view(np.uint32) == 0x80000005 and np.float32(hi).view(np.uint32) == 7, (lo, hi)
    ctx.set_blocking(True)
    # (b) scans: the extremes come first, signaling NaNs are sprinkled over the rest
    for dt_in in (0, 1):
        for n in (70_001, 1_000_003, 27_264_000 // 8):
            x = rng.uniform(-1, 1, n).astype(np.float32)
            x[0], x[1] = -5.0, 7.0
            xin = x if dt_in == 0 else O.f32_to_bf16(x)
            bits = xin.view(np.uint32) if dt_in == 0 else xin.view(np.uint16)
            bits[rng.choice(np.arange(2, n), n // 100, replace=False)] = SNAN32 if dt_in == 0 else SNAN16
            for dt_q in (4, 3, 2):
                want_p = O.compute_quant_params(xin, dt_in, dt_q)
                assert gpu_compute_params(ctx, xin, dt_in, dt_q) == want_p, (dt_in, n, dt_q)
                for fused in (True, False):
                    c = piquant.Context()
                    c.set_fusion(fused)
                    got, got_p = gpu_quantize_dynamic(c, xin, dt_in, dt_q)
                    assert got_p == want_p, (dt_in, n, dt_q, fused, got_p, want_p)
                    assert np.array_equal(got, O.quantize(xin, dt_in, dt_q, want_p[0], want_p[1])), (dt_in, n, dt_q, fused)
                    # the one-launch kernel takes the short step for the whole grid (the data range decides): NaN elements go through it, both roundings
                    c.set_stochastic_threshold(0.4375)
                    got, got_p = gpu_quantize_dynamic(c, xin, dt_in, dt_q, 1)
                    assert got_p == want_p and np.array_equal(got, O.quantize(xin, dt_in, dt_q, want_p[0], want_p[1], 1, 0.4375)), (dt_in, n, dt_q, fused, "stochastic")


def test_extreme_zero_points_wrap_like_the_reference(ctx, O):
    """int64 zero points are narrowed to int32 on the fast paths and kept on the generic ones (quantize.inl:111 vs :15)."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-100, 100, 5000).astype(np.float32)
    x[:4] = [np.nan, np.inf, -np.inf, 3e9]
    for zp in (2**31 - 1, -2**31, 2**32 + 5, -2**40, 2**62):
        for dt_out in (4, 3, 2):
            for rm, tau in ((0, 0.0), (1, 0.3)):
                ctx.set_stochastic_threshold(tau if rm else None)
                got = gpu_quantize(ctx, x, 0, dt_out, 0.5, zp, rm)
                assert np.array_equal(got, O.quantize(x, 0, dt_out, 0.5, zp, rm, tau)), (zp, dt_out, rm)
    ctx.set_stochastic_threshold(None)
    q = rng.integers(0, 256, 5000).astype(np.uint8)
    for zp in (2**31 - 1, -2**31, 2**32 + 5):
        for dt_q, dt_f in ((4, 0), (3, 1), (2, 0), (2, 1)):
            n = 5000 * (8 // {4: 8, 3: 4, 2: 2}[dt_q])
            got = gpu_dequantize(ctx, q, dt_q, dt_f, n, 0.5, zp)
            assert same_floats(got, O.dequantize(q, dt_q, dt_f, n, 0.5, zp)), (zp, dt_q, dt_f)


# ---------------------------------------------------------------------------------------------------
# pointer flavours: misaligned device buffers (guarded scalar kernels) and host buffers (PCIe staging)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off_in,off_out", [(4, 0), (0, 1), (8, 3), (2, 2)])
def test_misaligned_device_pointers(ctx, O, off_in, off_out):
    rng = np.random.default_rng(off_in * 16 + off_out)
    n = 70_001
    x = rng.uniform(-1, 1, n).astype(np.float32)
    for dt_in, xin in ((0, x), (1, O.f32_to_bf16(x))):
        if dt_in == 0 and off_in % 4:
            continue   # an fp32 array is at least 4-byte aligned
        for dt_out in (4, 3, 2):
            got = gpu_quantize(ctx, xin, dt_in, dt_out, 0.01, 7, 0, offset_in=off_in, offset_out=off_out)
            assert np.array_equal(got, O.quantize(xin, dt_in, dt_out, 0.01, 7))
    q = rng.integers(0, 256, n).astype(np.uint8)
    prev = rng.uniform(-1, 1, n).astype(np.float32)
    for dt_f, off in ((0, (off_out // 4) * 4 + 4), (1, (off_out // 2) * 2 + 2)):
        p = prev if dt_f == 0 else O.f32_to_bf16(prev)
        got = gpu_dequantize(ctx, q, 4, dt_f, n, 0.02, 9, 1, prev=p, offset_in=off_in, offset_out=off)
        assert same_floats(got, O.dequantize(q, 4, dt_f, n, 0.02, 9, 1, out=p.copy()))


# Round 3: buffers that are only element-aligned run through the VECTOR kernels (misaligned 16-byte loads; a scalar head peeled by block 0 so
# that the store stream is aligned, or misaligned stores where the head would not be a whole packed byte) -- reference shape:
# kernels_specialized.inl:52-82.  Every pair, both ops, both rounding modes, sizes around the tile edges, the offsets a torch slice produces.
@pytest.mark.parametrize("off_in,off_out", [(4, 0), (0, 4), (4, 4), (8, 1), (2, 15), (12, 8), (6, 2)])
def test_misaligned_pointers_take_the_vector_path_bit_exact(ctx, O, off_in, off_out):
    rng = np.random.default_rng(1000 + off_in * 16 + off_out)
    for n in (15, 16, 17, 100, 4096 + 15, 8192 + 16, 70_001, 1_000_003):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        if n > 50:
            x[rng.choice(n, 5, replace=False)] = [np.nan, np.inf, -1e30, 3e9, 0.0]
        for dt_in, xin in ((0, x), (1, O.f32_to_bf16(x))):
            esize = 4 if dt_in == 0 else 2
            oi = off_in - off_in % esize           # a float array is at least element-aligned
            for dt_out, qmax in ((4, 255), (3, 15), (2, 3)):
                scale = float(np.float32(2.0 / qmax))
                for rm, tau in ((0, 0.0), (1, 0.3)):
                    ctx.set_stochastic_threshold(tau if rm else None)
                    got = gpu_quantize(ctx, xin, dt_in, dt_out, scale, qmax // 2, rm, offset_in=oi, offset_out=off_out)
                    want = O.quantize(xin, dt_in, dt_out, scale, qmax // 2, rm, tau, form=O.FORM_UNIFORM)
                    assert np.array_equal(got, want), (n, dt_in, dt_out, rm, np.nonzero(got != want)[0][:5])
        ctx.set_stochastic_threshold(None)
        prev = rng.uniform(-1, 1, n).astype(np.float32)
        for dt_q in (4, 3, 2):
            q = rng.integers(0, 256, O.packed_numel(n, dt_q)).astype(np.uint8)
            for dt_f in (0, 1):
                esize = 4 if dt_f == 0 else 2
                oo = off_out - off_out % esize
                pv = prev if dt_f == 0 else O.f32_to_bf16(prev)
                for op in (0, 1):
                    got = gpu_dequantize(ctx, q, dt_q, dt_f, n, 0.02, 9, op, prev=pv, offset_in=off_in, offset_out=oo)
                    assert same_floats(got, O.dequantize(q, dt_q, dt_f, n, 0.02, 9, op, out=pv.copy())), (n, dt_q, dt_f, op)


def test_misaligned_minmax_scan(ctx, O):
    import piquant
    import torch

    rng = np.random.default_rng(5)
    for n in (7, 1000, 1_000_003):
        x = rng.uniform(-3, 3, n).astype(np.float32)
        for dt, xin, off in ((piquant.DataType.F32, x, 4), (piquant.DataType.F32, x, 12), (piquant.DataType.BF16, O.f32_to_bf16(x), 2), (piquant.DataType.BF16, O.f32_to_bf16(x), 10)):
            keep, ptr = to_device(xin, off)
            assert ptr % 16 == off
            keys = torch.empty(2, dtype=torch.int32, device="cuda")
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.minmax_keys_ptr(ptr, dt, n, keys.data_ptr(), init=True)
            k = keys.cpu()
            xf = xin if xin.dtype == np.float32 else O.bf16_to_f32(xin)
            assert piquant.decode_minmax_keys(int(k[0]), int(k[1])) == (float(xf.min()), float(xf.max()))
            del keep


def test_misaligned_full_size_slice_of_a_tensor(ctx, O, big_x):
    """x[1:] of the BASELINE tensor (4-byte-aligned input) and an output that starts 3 bytes into its buffer, at N1 - 1 elements: bit-exact."""
    x = big_x[1:]
    scale, zp = O.compute_quant_params(big_x, O.F32, O.UINT8)
    got = gpu_quantize(ctx, x, 0, 4, scale, zp, 0, offset_in=4, offset_out=3)
    want = O.quantize(x, 0, 4, scale, zp)
    assert np.array_equal(got, want)
    back = gpu_dequantize(ctx, want, 4, 0, x.size, scale, zp, 0, offset_in=3, offset_out=4)
    assert same_floats(back, O.dequantize(want, 4, 0, x.size, scale, zp, 0))


def test_host_pointers_are_staged_through_the_gpu(O):
    """The reference's callers pass host memory; asked to (`stage`), the drop-in takes it over PCIe in 2^24-element chunks to the HIP kernels."""
    import piquant

    ctx = piquant.Context()
    ctx.set_host_path("stage")
    assert ctx.host_path_in_effect() == "stage"
    rng = np.random.default_rng(77)
    n = (1 << 24) + 12_345     # two chunks
    x = rng.uniform(-1, 1, n).astype(np.float32)
    got = gpu_quantize(ctx, x, 0, 4, 0.0078431377, 127, 0, host=True)
    want = O.quantize(x, 0, 4, 0.0078431377, 127)
    assert np.array_equal(got, want)
    acc = rng.uniform(-1, 1, n).astype(np.float32)
    back = gpu_dequantize(ctx, got, 4, 0, n, 0.0078431377, 127, 1, prev=acc, host=True)
    assert same_floats(back, O.dequantize(want, 4, 0, n, 0.0078431377, 127, 1, out=acc.copy()))
    xb = O.f32_to_bf16(x[:100_001])
    assert np.array_equal(gpu_quantize(ctx, xb, 1, 3, 0.13, 7, 0, host=True), O.quantize(xb, 1, 3, 0.13, 7))
    import piquant

    assert ctx.compute_quant_params_ptr_float32(x.ctypes.data, piquant.DataType.UINT8, n) == O.compute_quant_params(x, 0, 4)


def test_host_pointers_on_the_cpu_companion_when_asked(O):
    """Host tensors stay on the host by default (`auto`, SURVEY 8b "host pointers -> CPU path"): calls on pageable host buffers are handed to
    libpiquant_cpu.so (AVX-512 on the host cores) instead of crossing PCIe twice; same bytes as the oracle and as the staged GPU path, also when
    asked for explicitly (`cpu`).  Device buffers of the same contexts still run the HIP kernels; reference-layout mode is staged."""
    import piquant
    import piquant.cpu
    import torch

    rng = np.random.default_rng(78)
    n = 3_000_001
    x = rng.uniform(-1, 1, n).astype(np.float32)
    staged, cpu_ctx, default_ctx = piquant.Context(), piquant.Context(), piquant.Context()
    staged.set_host_path("stage")
    cpu_ctx.set_host_path("cpu")
    assert staged.host_path_in_effect() == "stage" and cpu_ctx.host_path_in_effect() == "cpu"
    assert default_ctx.host_path_in_effect() == ("cpu" if piquant.cpu.has_avx512() else "stage")
    for c in (staged, cpu_ctx, default_ctx):
        got = gpu_quantize(c, x, 0, 4, 0.0078431377, 127, 0, host=True)
        want = O.quantize(x, 0, 4, 0.0078431377, 127)
        assert np.array_equal(got, want)
        acc = rng.uniform(-1, 1, n).astype(np.float32)
        back = gpu_dequantize(c, got, 4, 0, n, 0.0078431377, 127, 1, prev=acc, host=True)
        assert same_floats(back, O.dequantize(want, 4, 0, n, 0.0078431377, 127, 1, out=acc.copy()))
        xb = O.f32_to_bf16(x[:100_001])
        assert np.array_equal(gpu_quantize(c, xb, 1, 3, 0.13, 7, 0, host=True), O.quantize(xb, 1, 3, 0.13, 7))
        c.set_stochastic_threshold(0.25)
        assert np.array_equal(gpu_quantize(c, x, 0, 3, 0.13, 7, 1, host=True), O.quantize(x, 0, 3, 0.13, 7, 1, 0.25, form=O.FORM_UNIFORM))
        c.set_stochastic_threshold(None)
        assert c.compute_quant_params_ptr_float32(x.ctypes.data, piquant.DataType.UINT8, n) == O.compute_quant_params(x, 0, 4)
    # the CPU-path context on device buffers: the HIP kernels, as always
    assert np.array_equal(gpu_quantize(cpu_ctx, x, 0, 4, 0.0078431377, 127, 0), O.quantize(x, 0, 4, 0.0078431377, 127))


# ---------------------------------------------------------------------------------------------------
# BASELINE configs at full size: tests/test_gpu_00_baseline_configs.py (collected first)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_x():
    return np.random.default_rng(0).uniform(-1, 1, N1).astype(np.float32)


def test_more_than_2_pow_32_elements(O):
    """Maximum sizes: 64-bit element indexing end to end (numel > 2^32: 17 GB of fp32 in HBM).  The oracle checks
    windows around 0, 2^31, 2^32 and the ragged end; shard invariance (whole == three unequal chunks) covers the rest."""
    import piquant
    import torch

    n = (1 << 32) + 4099
    if torch.cuda.get_device_properties(0).total_memory < 80 * 2**30:
        pytest.skip("needs ~50 GB of HBM")
    x = torch.empty(n, dtype=torch.float32, device="cuda").uniform_(-1, 1)
    x[(1 << 32) + 77] = -3.5          # global extremes live beyond the 32-bit index range
    x[(1 << 31) + 5] = 2.75
    windows = [(0, 1 << 20), ((1 << 31) - (1 << 19), (1 << 31) + (1 << 19)), ((1 << 32) - (1 << 19), n)]

    scale, zp = piquant.torch.compute_quant_params(x, dtype=torch.quint8)
    assert (scale, zp) == O.quant_params_from_minmax(-3.5, 2.75, 4)
    q = piquant.torch.quantize(x, scale=scale, zero_point=zp, dtype=torch.uint8)
    for a, b in windows:
        assert np.array_equal(q[a:b].cpu().numpy(), O.quantize(x[a:b].cpu().numpy(), 0, 4, scale, zp)), (a, b)
    cuts = [0, (1 << 31) + 4096 * 3, (1 << 32) - 4096 * 5, n]
    q2 = torch.empty_like(q)
    for a, b in zip(cuts[:-1], cuts[1:]):
        piquant.torch.quantize(x[a:b], scale=scale, zero_point=zp, dtype=torch.uint8, out=q2[a:b])
    assert torch.equal(q, q2)
    del q2

    # packed uint4 from the same data (2 elements per byte: byte index = element index / 2 beyond 2^31)
    s4, z4 = piquant.torch.compute_quant_params(x, dtype=torch.quint4x2)
    q4 = piquant.torch.packed_bytes(piquant.torch.quantize(x, scale=s4, zero_point=z4, dtype=torch.quint4x2))
    assert q4.numel() == (n + 1) // 2
    for a, b in windows:
        assert a % 2 == 0
        assert np.array_equal(q4[a // 2: (b + 1) // 2].cpu().numpy(), O.quantize(x[a:b].cpu().numpy(), 0, 3, s4, z4)), (a, b)
    del q4

    # dequantize with the ADD store back over the whole range
    acc = torch.zeros(n, dtype=torch.float32, device="cuda")
    piquant.torch.dequantize(q, scale=scale, zero_point=zp, dtype=torch.float32, reduce_op="add", out=acc)
    for a, b in windows:
        want = O.dequantize(q[a:b].cpu().numpy(), 4, 0, b - a, scale, zp, 1, out=np.zeros(b - a, np.float32))
        assert same_floats(acc[a:b].cpu().numpy(), want), (a, b)
    assert float((acc - x).abs().max()) <= 0.5 * scale * 1.0001 + 1e-6


def test_stochastic_seed_makes_the_per_call_thresholds_reproducible(O):
    """The reference's per-call threshold comes from an unseedable thread-local generator (piquant.cpp:194-201); here the
    context owns the generator and piquant_hip_set_stochastic_seed makes a run repeatable: same seed -> same sequence of
    thresholds -> identical outputs call by call; each output equals the oracle for SOME threshold."""
    import piquant

    x = np.random.default_rng(2).uniform(-1, 1, 300_001).astype(np.float32)
    outs = []
    for _ in range(2):
        c = piquant.Context()
        c.set_stochastic_seed(1234)
        outs.append([gpu_quantize(c, x, 0, 4, 0.0078431377, 127, 1) for _ in range(4)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs[0][0], outs[0][1])          # consecutive calls draw different thresholds
    near = O.quantize(x, 0, 4, 0.0078431377, 127).astype(np.int16)
    for a in outs[0]:
        d = a.astype(np.int16) - near
        assert d.min() >= -1 and d.max() <= 1


def test_per_element_stochastic_extension(ctx, O):
    import piquant

    rng = np.random.default_rng(9)
    n = 1_000_003
    x = rng.uniform(-1, 1, n).astype(np.float32)
    c = piquant.Context()
    for dt_in, xin in ((0, x), (1, O.f32_to_bf16(x))):
        for dt_out, scale, zp in ((4, 0.0078431377, 127), (3, 0.13333334, 7), (2, 0.6666667, 1)):
            c.set_stochastic_per_element(True, seed=0x1234_5678_9ABC_DEF0, index_base=0)
            got = gpu_quantize(c, xin, dt_in, dt_out, scale, zp, 1)
            assert np.array_equal(got, O.quantize_per_element(xin, dt_in, dt_out, scale, zp, 0x1234_5678_9ABC_DEF0, 0))
    # shard invariance with index_base, and a base beyond 2^32
    base = (1 << 32) - 4096 * 3
    c.set_stochastic_per_element(True, seed=42, index_base=base)
    whole = gpu_quantize(c, x, 0, 4, 0.0078431377, 127, 1)
    assert np.array_equal(whole, O.quantize_per_element(x, 0, 4, 0.0078431377, 127, 42, base))
    cut = 4096 * 100
    c.set_stochastic_per_element(True, seed=42, index_base=base + cut)
    assert np.array_equal(gpu_quantize(c, x[cut:], 0, 4, 0.0078431377, 127, 1), whole[cut:])
    # unbiased: E[q] - zp == x/scale
    q = whole.astype(np.float64) - 127
    assert abs((q - x.astype(np.float64) / 0.0078431377).mean()) < 2e-3


# ---------------------------------------------------------------------------------------------------
# fused quantize -> dequantize ("requant", reference C++ API only; piquant_hip_quantize_dequantize here)
# ---------------------------------------------------------------------------------------------------
def gpu_requantize(ctx, x, dt, qd, scale, zp, rm, op, prev, in_place=False):
    import piquant
    import torch

    odt = np.float32 if dt == 0 else np.uint16
    _, pin = keep = to_device(x)
    obuf = torch.full((prev.nbytes + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    out = obuf[: prev.nbytes]
    if prev.nbytes:
        out.copy_(torch.from_numpy(prev.view(np.uint8).reshape(-1)))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    if in_place:
        ctx.quantize_dequantize_ptr(pin, piquant.DataType(dt), pin, piquant.DataType(qd), x.size, scale, zp, piquant.RoundMode(rm), piquant.ReduceOp(op))
        torch.cuda.synchronize()
        return keep[0].cpu().numpy().view(odt).copy()
    ctx.quantize_dequantize_ptr(pin, piquant.DataType(dt), out.data_ptr(), piquant.DataType(qd), x.size, scale, zp, piquant.RoundMode(rm),
                                piquant.ReduceOp(op))
    torch.cuda.synchronize()
    assert bool((obuf[prev.nbytes:] == 0xAA).all())
    return out.cpu().numpy().view(odt).copy()


def test_golden_requantize(ctx):
    cases, get = load_golden()
    n = 0
    for c in cases:
        if c["kind"] != "requantize" or c["numel"] == 0:
            continue
        ctx.set_stochastic_threshold(c["tau"] if c["round_mode"] else None)
        got = gpu_requantize(ctx, get(c["name"], "x"), c["dt"], c["quant_dtype"], c["scale"], c["zp"], c["round_mode"], c["op"], get(c["name"], "prev"))
        assert same_floats(got, get(c["name"], "ref")), c
        n += 1
    ctx.set_stochastic_threshold(None)
    assert n > 250


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("qd", [4, 3, 2], ids=["u8", "u4", "u2"])
def test_requantize_random_and_reference_tolerances(ctx, O, dt, qd):
    """Bit-exact vs the oracle, plus the reference's own round-trip test (test/requant.cpp:19-63: params from data,
    fused requant with SET and ADD, tolerance 0.1 / 0.2 / 0.7 for uint8 / uint4 / uint2)."""
    rng = np.random.default_rng(40 + 10 * dt + qd)
    tol = {4: 0.1, 3: 0.2, 2: 0.7}[qd]
    for n in (1, 1000, 4096, 4097, 1_000_003):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        xin = x if dt == 0 else O.f32_to_bf16(x)
        scale, zp = O.compute_quant_params(xin, dt, qd)
        for rm, tau in ((0, 0.0), (1, 0.41)):
            ctx.set_stochastic_threshold(tau if rm else None)
            for op in (0, 1):
                prev = rng.uniform(-1, 1, n).astype(np.float32)
                prev = prev if dt == 0 else O.f32_to_bf16(prev)
                got = gpu_requantize(ctx, xin, dt, qd, scale, zp, rm, op, prev)
                want = O.requantize(xin, dt, qd, scale, zp, rm, tau, op, out=prev.copy())
                assert same_floats(got, want), (n, rm, op)
                if dt == 0 and rm == 0 and n > 1:
                    err = np.abs(got - (prev if op else 0) - x)
                    assert err.max() <= tol, (n, op, err.max())
            if dt == 0:   # in place (out aliases in)
                got = gpu_requantize(ctx, xin, dt, qd, scale, zp, rm, 0, np.zeros(n, np.float32), in_place=True)
                assert same_floats(got, O.requantize(xin, dt, qd, scale, zp, rm, tau, 0))
    ctx.set_stochastic_threshold(None)


def test_requantize_torch_api(O):
    import piquant
    import torch

    x = torch.empty(300_001, device="cuda").uniform_(-1, 1)
    scale, zp = piquant.torch.compute_quant_params(x, dtype=torch.quint4x2)
    y = piquant.torch.quantize_dequantize(x, scale=scale, zero_point=zp, quant_dtype=torch.quint4x2)
    q = piquant.torch.quantize(x, scale=scale, zero_point=zp, dtype=torch.quint4x2)
    z = piquant.torch.dequantize(q, scale=scale, zero_point=zp, dtype=torch.float32)
    assert float((y - z).abs().max()) <= 1e-6      # same values as the two-pass route on ordinary data
    assert np.array_equal(y.cpu().numpy(), O.requantize(x.cpu().numpy(), 0, 3, scale, zp))


# ---------------------------------------------------------------------------------------------------
# compute_quant_params
# ---------------------------------------------------------------------------------------------------
def test_minmax_scan_ignores_nans_like_the_oracle(ctx, O):
    """NaNs are skipped by the HIP scan wherever they sit (v_min/v_max return the other operand): the position-independent reading of
    the reference's out-of-contract behaviour that tests/test_oracle_vs_ref.py pins; a tensor of NaNs only scans to the identities."""
    import piquant
    import torch

    rng = np.random.default_rng(33)
    for n in (37, 64, 1000, 4099, 1_000_003):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        x[n // 3], x[n // 2] = -5.0, 7.0
        x[[0, n - 1, n // 5]] = np.nan
        for dt, host in ((piquant.DataType.F32, x), (piquant.DataType.BF16, O.f32_to_bf16(x))):
            keep, ptr = to_device(host)
            keys = torch.empty(2, dtype=torch.int32, device="cuda")
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.set_blocking(False)
            ctx.minmax_keys_ptr(ptr, dt, n, keys.data_ptr(), True)
            torch.cuda.synchronize()
            k = keys.cpu().numpy()
            assert piquant.decode_minmax_keys(int(k[0]), int(k[1])) == O.minmax(host, O.F32 if dt == piquant.DataType.F32 else O.BF16) == (-5.0, 7.0)
    nans = torch.full((1000,), float("nan"), device="cuda")
    keys = torch.empty(2, dtype=torch.int32, device="cuda")
    ctx.minmax_keys_ptr(nans.data_ptr(), piquant.DataType.F32, 1000, keys.data_ptr(), True)
    torch.cuda.synchronize()
    k = keys.cpu().numpy()
    lo, hi = piquant.decode_minmax_keys(int(k[0]), int(k[1]))
    assert lo == np.float32(3.4028235e38) and hi == -np.float32(3.4028235e38)


def test_compute_quant_params_matches_oracle(ctx, O):
    import piquant
    import torch

    rng = np.random.default_rng(21)
    for n in (1, 2, 7, 64, 1023, 1024, 4097, 1_000_003, 5_000_000):
        x = rng.normal(size=n).astype(np.float32)
        for pos_lo, pos_hi in ((0, n - 1), (n - 1, 0), (n // 2, n // 3)):
            y = x.copy()
            y[pos_lo] = -11.0
            if pos_hi != pos_lo:
                y[pos_hi] = 13.0
            yd = torch.from_numpy(y).cuda()
            yb = O.f32_to_bf16(y)
            ybd = torch.from_numpy(yb.view(np.int16)).cuda().view(torch.bfloat16)
            for tdt, odt in ((torch.quint8, 4), (torch.quint4x2, 3), (torch.quint2x4, 2)):
                assert piquant.torch.compute_quant_params(yd, dtype=tdt) == O.compute_quant_params(y, 0, odt), (n, pos_lo)
                assert piquant.torch.compute_quant_params(ybd, dtype=tdt) == O.compute_quant_params(yb, 1, odt), (n, pos_lo)
    # degenerate range -> (1.0, mid)   (reference src/piquant.cpp:249-252, test/quant.cpp:198-217)
    const = torch.full((1000,), 42.0, device="cuda")
    assert [piquant.torch.compute_quant_params(const, dtype=d) for d in (torch.quint8, torch.quint4x2, torch.quint2x4)] == [(1.0, 127), (1.0, 7), (1.0, 1)]
    # misaligned view
    base = torch.from_numpy(rng.normal(size=10_001).astype(np.float32)).cuda()
    assert piquant.torch.compute_quant_params(base[1:], dtype=torch.quint8) == O.compute_quant_params(base[1:].cpu().numpy(), 0, 4)
    # extremes of the float range through the synchronous call: infinities (the reference returns (inf, 0): inf passes its `scale >= 0` assertion,
    # src/piquant.cpp:373), +-FLT_MAX (the range only fits in the epilogue's doubles), denormals only, zeros of both signs only
    for vals in ([np.inf], [-np.inf], [np.inf, -np.inf], [3.4028235e38, -3.4028235e38], [3.4028235e38], [-3.4028235e38]):
        y = rng.normal(size=70_001).astype(np.float32)
        y[rng.choice(y.size, len(vals), replace=False)] = vals
        yb = O.f32_to_bf16(y)                       # FLT_MAX rounds to inf in bf16: one more infinity case
        for tdt, odt in ((torch.quint8, 4), (torch.quint4x2, 3), (torch.quint2x4, 2)):
            assert piquant.torch.compute_quant_params(torch.from_numpy(y).cuda(), dtype=tdt) == O.compute_quant_params(y, 0, odt), (vals, odt)
            assert piquant.torch.compute_quant_params(torch.from_numpy(yb.view(np.int16)).cuda().view(torch.bfloat16), dtype=tdt) == O.compute_quant_params(yb, 1, odt), (vals, odt)
    for y in ((rng.uniform(-1, 1, 5000) * 1e-41).astype(np.float32), np.where(rng.uniform(size=5000) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)):
        for tdt, odt in ((torch.quint8, 4), (torch.quint4x2, 3), (torch.quint2x4, 2)):
            assert piquant.torch.compute_quant_params(torch.from_numpy(y).cuda(), dtype=tdt) == O.compute_quant_params(y, 0, odt), odt


def test_compute_quant_params_back_to_back(O):
    """The result travels through a pinned host mailbox tagged with a sequence number and the scan alternates between
    two slot buffers: hammer it with alternating tensors, dtypes and streams -- every answer must be the tensor's own."""
    import piquant
    import torch

    rng = np.random.default_rng(8)
    tensors = []
    for i in range(6):
        x = (rng.normal(size=200_000 + 1000 * i) * (i + 1)).astype(np.float32)
        tensors.append((torch.from_numpy(x).cuda(), O.compute_quant_params(x, 0, 4), O.compute_quant_params(x, 0, 3)))
    side = torch.cuda.Stream()
    for it in range(300):
        t, want8, want4 = tensors[it % len(tensors)]
        if it % 3 == 2:
            with torch.cuda.stream(side):
                got = piquant.torch.compute_quant_params(t, dtype=torch.quint8)
        else:
            got = piquant.torch.compute_quant_params(t, dtype=torch.quint8 if it % 2 else torch.quint4x2)
            want8 = want8 if it % 2 else want4
        assert got == want8, it


def test_device_resident_params_match_the_host_epilogue(O):
    """piquant_hip_compute_quant_params_device: the double-precision epilogue runs in a one-wave kernel; scale, 1/scale and
    zero point must be bit-identical to the host path (and to the oracle) on ordinary, degenerate and extreme ranges."""
    import struct

    import piquant
    import torch

    rng = np.random.default_rng(31)
    cases = [rng.normal(size=n).astype(np.float32) * s for n in (1, 2, 1000, 70_001) for s in (1.0, 1e-3, 1e4, 1e-30, 1e30)]
    cases += [np.full(1000, 42.0, np.float32), np.array([2.0, 6.0], np.float32), np.array([-6.0, -2.0], np.float32),
              np.array([-1.0, 1.0], np.float32), np.linspace(-1, 3, 1001).astype(np.float32), np.array([0.0, 1e-45], np.float32),
              np.array([-3.4e38, 3.4e38], np.float32)]
    for x in cases:
        xd = torch.from_numpy(x).cuda()
        for tdt, odt in ((torch.quint8, 4), (torch.quint4x2, 3), (torch.quint2x4, 2)):
            rec = piquant.torch.compute_quant_params_device(xd, dtype=tdt)
            scale, inv, zp = struct.unpack("<ffq", rec.cpu().numpy().tobytes())
            want = O.compute_quant_params(x, 0, odt)
            host = piquant.torch.compute_quant_params(xd, dtype=tdt) if want[0] >= 0 and not np.isnan(want[0]) else want
            assert (np.float32(scale).tobytes(), zp) == (np.float32(want[0]).tobytes(), want[1]) == (np.float32(host[0]).tobytes(), host[1]), (x[:3], tdt)
            with np.errstate(divide="ignore", over="ignore"):
                assert np.float32(inv).tobytes() == (np.float32(1.0) / np.float32(want[0])).tobytes()
            assert piquant.torch.params_to_host(rec) == (scale, zp)


def test_dynamic_pipeline_equals_the_two_step_path_and_is_graph_capturable(O):
    import piquant
    import torch

    rng = np.random.default_rng(32)
    n = 3_000_001
    for dt_name, tdt, odt, qd in (("f32", torch.quint8, 4, 4), ("bf16", torch.quint4x2, 3, 3), ("f32", torch.quint2x4, 2, 2)):
        x = rng.uniform(-2, 3, n).astype(np.float32)
        xin = x if dt_name == "f32" else O.f32_to_bf16(x)
        xd = torch.from_numpy(xin).cuda() if dt_name == "f32" else torch.from_numpy(xin.view(np.int16)).cuda().view(torch.bfloat16)
        fdt = torch.float32 if dt_name == "f32" else torch.bfloat16
        q, rec = piquant.torch.quantize_dynamic(xd, dtype=tdt)
        scale, zp = piquant.torch.params_to_host(rec)
        assert (scale, zp) == O.compute_quant_params(xin, 0 if dt_name == "f32" else 1, odt)
        want_q = O.quantize(xin, 0 if dt_name == "f32" else 1, qd, scale, zp)
        assert np.array_equal(piquant.torch.packed_bytes(q).cpu().numpy(), want_q)
        acc = torch.ones(n, dtype=fdt, device="cuda")
        piquant.torch.dequantize_dynamic(q, rec, dtype=fdt, reduce_op="add", out=acc)
        ones = np.ones(n, np.float32) if dt_name == "f32" else O.f32_to_bf16(np.ones(n, np.float32))
        want_acc = O.dequantize(want_q, qd, 0 if dt_name == "f32" else 1, n, scale, zp, 1, out=ones)
        got_acc = acc.cpu().numpy() if dt_name == "f32" else acc.view(torch.int16).cpu().numpy().view(np.uint16)
        assert same_floats(got_acc, want_acc)

    # whole dynamic pipeline in one hipGraph: new data -> replay -> parameters, bytes and reconstruction follow, no host sync inside
    x = torch.zeros(n, device="cuda")
    q = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(16, dtype=torch.uint8, device="cuda")
    y = torch.zeros(n, device="cuda")
    c = piquant.Context()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        piquant.torch.quantize_dynamic(x, dtype=torch.uint8, ctx=c, out=q, params=rec)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            piquant.torch.quantize_dynamic(x, dtype=torch.uint8, ctx=c, out=q, params=rec)
            piquant.torch.dequantize_dynamic(q, rec, dtype=torch.float32, ctx=c, out=y)
    for k in (3.0, 0.25, 1.0, 0.5):     # the range shrinks and grows between replays: a replay must not see the previous one's extremes
        data = (rng.normal(size=n) * k).astype(np.float32)
        x.copy_(torch.from_numpy(data))
        g.replay()
        torch.cuda.synchronize()
        scale, zp = piquant.torch.params_to_host(rec)
        assert (scale, zp) == O.compute_quant_params(data, 0, 4)
        wq = O.quantize(data, 0, 4, scale, zp)
        assert np.array_equal(q.cpu().numpy(), wq)
        assert same_floats(y.cpu().numpy(), O.dequantize(wq, 4, 0, n, scale, zp))


def test_one_context_on_two_forked_streams_inside_one_capture(O):
    """Round-2 advisor finding: inside capture the context's own serialisation is skipped, so two fused / scan launches of ONE context
    captured on parallel branches of a graph (two side streams forked inside the capture) shared the barrier and scan state concurrently
    and could mix the keys of different tensors.  Now the second launch is made a graph successor of the first (event edge inside the
    capture): both tensors get their own parameters and bytes on every replay, fused and unfused."""
    import piquant
    import torch

    rng = np.random.default_rng(91)
    n = 5_000_000
    for fusion in (True, False):
        c = piquant.Context()
        c.set_barrier_timeout_us(50_000)   # "no hand-over" below means "launches were ordered", not "no block ever waited 1 ms on a busy box"
        c.set_fusion(fusion)
        xa, xb = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        qa, qb = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        ra, rb = torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.uint8, device="cuda")
        main, side = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(main):
            piquant.torch.quantize_dynamic(xa, dtype=torch.uint8, ctx=c, out=qa, params=ra)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(main):
            with torch.cuda.graph(g, stream=main):
                side.wait_stream(main)                      # fork: `side` joins the capture
                piquant.torch.quantize_dynamic(xa, dtype=torch.uint8, ctx=c, out=qa, params=ra)
                with torch.cuda.stream(side):
                    piquant.torch.quantize_dynamic(xb, dtype=torch.uint8, ctx=c, out=qb, params=rb)
                main.wait_stream(side)                      # join
        for ka, kb in ((1.0, 40.0), (25.0, 0.5), (3.0, 3.0)):
            da = (rng.normal(size=n) * ka).astype(np.float32)
            db = (rng.normal(size=n) * kb + 2.0).astype(np.float32)
            xa.copy_(torch.from_numpy(da))
            xb.copy_(torch.from_numpy(db))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for data, q, rec in ((da, qa, ra), (db, qb, rb)):
                scale, zp = piquant.torch.params_to_host(rec)
                assert (scale, zp) == O.compute_quant_params(data, 0, 4), (fusion, ka, kb)
                assert np.array_equal(q.cpu().numpy(), O.quantize(data, 0, 4, scale, zp))
        assert c.barrier_bailouts() == 0


def test_fused_nodes_of_one_context_replayed_many_times_keep_their_generation(O):
    """Round-3 advisor finding: the fused kernel picks one of two barrier buffers by the parity of a generation word that the previous fused
    launch of the context bumped.  Fused nodes of one context in one hipGraph, each a successor of the one before (a forked side stream
    included: round 4 broke that edge for a day by forgetting the capturing stream whenever the binding switched streams, and the two nodes
    ran side by side), are the hard case -- nothing but the dispatch's own acquire stands between the bump and the read -- so the graph is
    replayed a few hundred times with the extremes of both tensors moved around on every replay; a node that read a stale parity, or shared
    the barrier state with its sibling, loses a block's extremes: wrong parameters, caught here."""
    import piquant
    import torch

    n = 3_000_000
    c = piquant.Context()
    c.set_barrier_timeout_us(50_000)   # "no hand-over" below means "launches were ordered", not "no block ever waited 1 ms on a busy box"
    xa, xb = torch.empty(n, device="cuda").uniform_(-1, 1), torch.empty(n, device="cuda").uniform_(-1, 1)
    qa, qb = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    ra, rb = torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.uint8, device="cuda")
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(main):
        piquant.torch.quantize_dynamic(xa, dtype=torch.uint8, ctx=c, out=qa, params=ra)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(main):
        with torch.cuda.graph(g, stream=main):
            side.wait_stream(main)
            piquant.torch.quantize_dynamic(xa, dtype=torch.uint8, ctx=c, out=qa, params=ra)
            with torch.cuda.stream(side):
                piquant.torch.quantize_dynamic(xb, dtype=torch.uint8, ctx=c, out=qb, params=rb)
            main.wait_stream(side)
            piquant.torch.quantize_dynamic(xb, dtype=torch.uint8, ctx=c, out=qb, params=rb)      # a third node: parity flips between replays too
    rng = np.random.default_rng(5)
    for it in range(300):
        # the extremes are single planted elements whose place and value change per replay: the block that holds them changes too
        ia, ib = int(rng.integers(0, n)), int(rng.integers(0, n))
        ja, jb = int(rng.integers(0, n)), int(rng.integers(0, n))
        va, vb = float(rng.uniform(2, 50)), float(rng.uniform(2, 50))
        xa[ia], xa[ja] = va, -va * 0.5
        xb[ib], xb[jb] = vb * 0.75, -vb
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if ia != ja:
            assert piquant.torch.params_to_host(ra) == piquant.quant_params_from_minmax(float(np.float32(-va * 0.5)), float(np.float32(va)), piquant.DataType.UINT8), it
        if ib != jb:
            assert piquant.torch.params_to_host(rb) == piquant.quant_params_from_minmax(float(np.float32(-vb)), float(np.float32(vb * 0.75)), piquant.DataType.UINT8), it
        xa[ia], xa[ja], xb[ib], xb[jb] = 0.5, -0.5, 0.5, -0.5      # back inside (-1, 1)
    assert c.barrier_bailouts() == 0


def test_stream_can_be_destroyed_after_it_has_been_replaced(ctx, O):
    """A caller's stream handed to set_stream may be destroyed once the context has moved to another stream: no scan or fused launch that
    follows may touch the old handle (round-2 advisor finding: the fused-launch order and the scan kept it)."""
    import piquant
    import torch

    rng = np.random.default_rng(92)
    x = rng.uniform(-1, 1, 2_000_000).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    c = piquant.Context()
    for _ in range(3):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            q, rec = piquant.torch.quantize_dynamic(xd, dtype=torch.uint8, ctx=c)
            sp = piquant.torch.compute_quant_params(xd, dtype=torch.quint8, ctx=c)
        c.reset_stream()
        del s                                   # torch returns pooled streams, so also force real handle churn below
        torch.cuda.synchronize()
        assert piquant.torch.params_to_host(rec) == sp == O.compute_quant_params(x, 0, 4)
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")
    for _ in range(3):
        h = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(h)) == 0
        c.set_stream(h.value)
        c.set_blocking(False)
        out = torch.empty(x.size, dtype=torch.uint8, device="cuda")
        recb = torch.zeros(16, dtype=torch.uint8, device="cuda")
        c.quantize_dynamic_ptr(xd.data_ptr(), piquant.DataType.F32, out.data_ptr(), piquant.DataType.UINT8, x.size, recb.data_ptr(), piquant.RoundMode.NEAREST, _device_ptrs=True)
        c.reset_stream()                        # the context lets go of the handle ...
        assert hip.hipStreamSynchronize(h) == 0
        assert hip.hipStreamDestroy(h) == 0     # ... so it may die
        out2 = torch.empty(x.size, dtype=torch.uint8, device="cuda")
        c.quantize_dynamic_ptr(xd.data_ptr(), piquant.DataType.F32, out2.data_ptr(), piquant.DataType.UINT8, x.size, recb.data_ptr(), piquant.RoundMode.NEAREST, _device_ptrs=True)
        c.set_blocking(True)
        s_, z_ = c.compute_quant_params_ptr_float32(xd.data_ptr(), piquant.DataType.UINT8, x.size, _device_ptrs=True)
        torch.cuda.synchronize()
        assert (s_, z_) == O.compute_quant_params(x, 0, 4) and torch.equal(out, out2)


def test_scans_on_two_streams_of_one_context_do_not_overlap(O):
    """Scans of one context share one state buffer.  A long scan on stream A followed at once by a scan of other data on stream B: the context
    records an event behind the first when it leaves A and B waits for it -- no host wait, and both results right (keys of the two tensors never mix)."""
    import piquant
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=g)
    big[123] = -3.0
    big[-7] = 2.5
    small = torch.empty(100_003, dtype=torch.float32, device="cuda").uniform_(10.0, 20.0, generator=g)
    lo_s, hi_s = float(small.min()), float(small.max())
    c = piquant.Context()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ka, kb = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.set_blocking(False)
    for _ in range(5):
        c.set_stream(a.cuda_stream)
        c.minmax_keys_ptr(big.data_ptr(), piquant.DataType.F32, big.numel(), ka.data_ptr(), init=True, _device_ptrs=True)
        c.set_stream(b.cuda_stream)
        c.minmax_keys_ptr(small.data_ptr(), piquant.DataType.F32, small.numel(), kb.data_ptr(), init=True, _device_ptrs=True)
        torch.cuda.synchronize()
        assert piquant.decode_minmax_keys(int(ka[0]), int(ka[1])) == (-3.0, 2.5)
        assert piquant.decode_minmax_keys(int(kb[0]), int(kb[1])) == (lo_s, hi_s)


def test_minmax_keys_accumulate_across_calls(ctx, O):
    """init=0 folds further scans into the same keys: the building block of the multi-GPU reduction."""
    import piquant
    import torch

    rng = np.random.default_rng(4)
    parts = [rng.normal(size=n).astype(np.float32) for n in (1000, 77, 123_456)]
    keys = torch.empty(2, dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    keep = []
    for i, p in enumerate(parts):
        t = torch.from_numpy(p).cuda()
        keep.append(t)
        ctx.minmax_keys_ptr(t.data_ptr(), piquant.DataType.F32, t.numel(), keys.data_ptr(), init=(i == 0))
    k = keys.cpu()
    assert piquant.decode_minmax_keys(int(k[0]), int(k[1])) == O.minmax(np.concatenate(parts), 0)


# ---------------------------------------------------------------------------------------------------
# API semantics
# ---------------------------------------------------------------------------------------------------
def test_blocking_default_and_stream_ordering(O):
    """A fresh context behaves like the reference: the call returns when the result is complete."""
    import piquant
    import torch

    c = piquant.Context()
    x = np.random.default_rng(3).uniform(-1, 1, 3_000_000).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros(x.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.quantize_ptr(xd.data_ptr(), piquant.DataType.F32, out.data_ptr(), piquant.DataType.UINT8, x.size, 0.0078431377, 127, piquant.RoundMode.NEAREST)
    # no torch-side synchronisation: the blocking context already waited on its own stream
    got = out.cpu().numpy()
    assert np.array_equal(got, O.quantize(x, 0, 4, 0.0078431377, 127))
    # stream-ordered mode on a side stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = xd * 2.0
        q = piquant.torch.quantize(y, scale=0.0157, zero_point=127, dtype=torch.uint8, ctx=c)
        back = piquant.torch.dequantize(q, scale=0.0157, zero_point=127, dtype=torch.float32, ctx=c)
    s.synchronize()
    assert np.array_equal(q.cpu().numpy(), O.quantize((x * np.float32(2.0)), 0, 4, 0.0157, 127))
    assert float((back - y).abs().max()) <= 0.0157 * 0.5 + 1e-6


def test_default_stream_ordering_without_explicit_sync(O):
    """PyTorch's default stream is HIP's legacy NULL stream (cuda_stream == 0): work enqueued through piquant.torch
    must be ordered behind the tensor's producer and ahead of its consumer with no synchronize() in between."""
    import piquant
    import torch

    n = 8_000_000
    base = torch.empty(n, device="cuda").uniform_(-1, 1)
    ref_in = (base * 0.5 + 0.25).cpu().numpy()
    torch.cuda.synchronize()
    for _ in range(3):
        x = base
        for _ in range(40):          # a long producer chain on the default stream
            x = x * 1.0
        x = x * 0.5 + 0.25
        q = piquant.torch.quantize(x, scale=0.0078431377, zero_point=64, dtype=torch.uint8)
        keys_scale = piquant.torch.compute_quant_params(x, dtype=torch.quint8)
        got = q.cpu().numpy()        # consumer on the default stream, no explicit sync
        assert np.array_equal(got, O.quantize(ref_in, 0, 4, 0.0078431377, 64))
        assert keys_scale == O.compute_quant_params(ref_in, 0, 4)


def test_calls_are_capturable_in_a_hip_graph(O):
    """Stream-ordered calls on device pointers enqueue kernels and nothing else (no allocation, no synchronisation), so a
    quantize -> dequantize(ADD) -> requant chain can be captured once into a hipGraph and replayed on new data."""
    import piquant
    import torch

    n = 2_000_003
    x = torch.zeros(n, device="cuda")
    q = torch.zeros(n, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(n, device="cuda")
    y = torch.zeros(n, device="cuda")
    c = piquant.Context()
    scale, zp = 0.0078431377, 128
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        piquant.torch.quantize(x, scale=scale, zero_point=zp, dtype=torch.uint8, ctx=c, out=q)     # warm-up outside capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            piquant.torch.quantize(x, scale=scale, zero_point=zp, dtype=torch.uint8, ctx=c, out=q)
            piquant.torch.dequantize(q, scale=scale, zero_point=zp, dtype=torch.float32, reduce_op="add", ctx=c, out=acc)
            piquant.torch.quantize_dequantize(x, scale=scale, zero_point=zp, quant_dtype=torch.quint4x2, ctx=c, out=y)
    rng = np.random.default_rng(12)
    want_acc = np.zeros(n, dtype=np.float32)
    for _ in range(3):
        data = rng.uniform(-1, 1, n).astype(np.float32)
        x.copy_(torch.from_numpy(data))
        g.replay()
        torch.cuda.synchronize()
        wq = O.quantize(data, 0, 4, scale, zp)
        want_acc = O.dequantize(wq, 4, 0, n, scale, zp, 1, out=want_acc)
        assert np.array_equal(q.cpu().numpy(), wq)
        assert same_floats(acc.cpu().numpy(), want_acc)
        assert same_floats(y.cpu().numpy(), O.requantize(data, 0, 3, scale, zp))


def test_empty_inputs_are_no_ops(ctx):
    import piquant

    ctx.quantize_ptr(0, piquant.DataType.F32, 0, piquant.DataType.UINT4, 0, 1.0, 0, piquant.RoundMode.NEAREST)
    ctx.dequantize_ptr(0, piquant.DataType.UINT2, 0, piquant.DataType.BF16, 0, 1.0, 0, piquant.ReduceOp.ADD)


@pytest.mark.parametrize("snippet,needle", [
    ("C.piquant_quantize(ctx, p, 4, p, 4, 16, 1.0, 0, 0)", "must be a dequantized type"),
    ("C.piquant_quantize(ctx, p, 0, p, 1, 16, 1.0, 0, 0)", "must be a quantized type"),
    ("C.piquant_dequantize(ctx, p, 0, p, 0, 16, 1.0, 0, 0)", "must be a quantized type"),
    ("C.piquant_dequantize(ctx, p, 3, p, 4, 16, 1.0, 0, 0)", "must be a dequantized type"),
])
def test_contract_violations_abort_like_the_reference(snippet, needle):
    """reference src/piquant.cpp:88-98,288-289,321-322: message on stderr, then abort()."""
    code = textwrap.dedent(f"""
        import sys; sys.path.insert(0, {str(os.path.join(os.path.dirname(__file__), '..', 'pi-quant_amd'))!r})
        import torch, piquant
        from piquant._bootstrap import C_LIB as C
        t = torch.zeros(64, device='cuda'); p = t.data_ptr()
        ctx = C.piquant_context_create(1)
        {snippet}
        print('survived')
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == -6, (r.returncode, r.stderr[-500:])   # SIGABRT
    assert needle in r.stderr and "survived" not in r.stdout


def test_reference_layout_of_a_multi_thread_reference_context(ctx, O):
    """VERDICT r01 "missing 4": a reference context with T pool threads splits a call into T partitions (src/piquant.cpp:145-157), each with
    its own scalar head (fp32 -> uint8) and tail, so the corner inputs land on different formulas than with one thread.
    `set_reference_layout(True, threads=T)` reproduces that; the oracle's threaded reference form is pinned to the reference kernels run
    per partition (tests/test_oracle_vs_ref.py).  Data is salted with the values on which the formulas differ."""
    rng = np.random.default_rng(78)
    try:
        for threads in (2, 3, 7):
            ctx.set_reference_layout(True, threads=threads)
            for n in (5, 64, 1000, 4099, 70_001):
                x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
                x[rng.choice(n, max(1, n // 3))] = np.float32(0.49999997)
                x[rng.choice(n, max(1, n // 5))] = np.float32(-0.49999997)
                x[rng.choice(n, max(1, n // 7))] = np.float32(8388609.0)     # odd and >= 2^23
                xb = O.f32_to_bf16(x)
                differs = 0
                for dt_in, xin in ((O.F32, x), (O.BF16, xb)):
                    for dt_out in (O.UINT8, O.UINT4, O.UINT2):
                        for off in ((0, 5) if (dt_in, dt_out) == (O.F32, O.UINT8) else (0,)):
                            nbytes = O.packed_numel(n, dt_out)
                            wbuf = np.zeros(nbytes + 32, dtype=np.uint8)
                            base = (-wbuf.ctypes.data) % 16
                            want = O.quantize(xin, dt_in, dt_out, 1.0, 1, form=O.FORM_REFERENCE, threads=threads, out=wbuf[base + off: base + off + nbytes])
                            got = gpu_quantize(ctx, xin, dt_in, dt_out, 1.0, 1, offset_out=off)
                            assert np.array_equal(got, want), (threads, n, dt_in, dt_out, off)
                            differs += int(not np.array_equal(want, O.quantize(xin, dt_in, dt_out, 1.0, 1, form=O.FORM_REFERENCE)))
                # dequantize: tails of the partitions (bf16 ADD double rounding, the uint2 -> fp32 ADD tail that stores)
                for dt_q in (O.UINT8, O.UINT4, O.UINT2):
                    q = rng.integers(0, 256, O.packed_numel(n, dt_q), dtype=np.uint8)
                    for dt_f, prev in ((O.F32, rng.uniform(-3, 3, n).astype(np.float32)), (O.BF16, O.f32_to_bf16(rng.uniform(-3, 3, n).astype(np.float32)))):
                        for op in (0, 1):
                            want = O.dequantize(q, dt_q, dt_f, n, 0.3, 2, op, form=O.FORM_REFERENCE, threads=threads, out=prev.copy())
                            got = gpu_dequantize(ctx, q, dt_q, dt_f, n, 0.3, 2, op, prev=prev.copy())
                            assert same_floats(got, want), (threads, n, dt_q, dt_f, op)
                if n >= 1000:
                    assert differs > 0, "partitioning never moved a corner input onto another formula: nothing was tested"
    finally:
        ctx.set_reference_layout(False, threads=1)


# ---------------------------------------------------------------------------------------------------
# reference-layout mode: scalar head/tail formulas at the reference's positions -> equals golden `ref` byte for byte
# ---------------------------------------------------------------------------------------------------
def test_reference_layout_matches_golden_ref(ctx):
    cases, get = load_golden()
    ctx.set_reference_layout(True, threads=1)
    try:
        nq = nd = differing = 0
        for c in cases:
            if c["kind"] == "quantize":
                ctx.set_stochastic_threshold(c["tau"] if c["round_mode"] else None)
                got = gpu_quantize(ctx, get(c["name"], "x"), c["dt_in"], c["dt_out"], c["scale"], c["zp"], c["round_mode"])
                assert np.array_equal(got, get(c["name"], "ref")), c
                differing += int(not np.array_equal(get(c["name"], "ref"), get(c["name"], "uniform")))
                nq += 1
            elif c["kind"] == "dequantize":
                got = gpu_dequantize(ctx, get(c["name"], "q"), c["dt_in"], c["dt_out"], c["numel"], c["scale"], c["zp"], c["op"],
                                     prev=get(c["name"], "prev"))
                assert same_floats(got, get(c["name"], "ref")), c
                differing += int(not same_floats(get(c["name"], "ref"), get(c["name"], "uniform")))
                nd += 1
        assert nq > 500 and nd > 400
        assert differing > 20       # the mode is exercised: these cases differ between the two forms
    finally:
        ctx.set_stochastic_threshold(None)
        ctx.set_reference_layout(False)


def test_reference_layout_head_and_host_chunks(ctx, O):
    """fp32 -> uint8 with a misaligned output pointer (scalar head, kernels_specialized.inl:52), device and host buffers; and a
    host call longer than one staging chunk whose tail sits in the last chunk."""
    rng = np.random.default_rng(77)
    ctx.set_reference_layout(True, threads=1)
    try:
        for n in (1, 7, 15, 16, 64, 100, 1000, 4097, 70_001):
            x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
            x[rng.choice(n, max(1, n // 3))] = np.float32(0.49999997) * np.float32(0.01)   # p = 0.49999997 up to rounding
            x[rng.choice(n, max(1, n // 5))] = np.float32(-0.49999997)
            for off in (0, 1, 5, 15):
                for scale, zp in ((1.0, 3), (0.01, 0)):
                    want_buf = np.zeros(n + 16 + off, dtype=np.uint8)
                    base = (-want_buf.ctypes.data) % 16
                    want = O.quantize(x, O.F32, O.UINT8, scale, zp, form=O.FORM_REFERENCE, out=want_buf[base + off: base + off + n])
                    got = gpu_quantize(ctx, x, O.F32, O.UINT8, scale, zp, offset_out=off)
                    assert np.array_equal(got, want), (n, off, scale)
        # host pointers: alignment of the HOST output pointer decides the head
        import piquant
        n = (1 << 24) + 1000 + 37
        x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
        x[-37:] = np.float32(0.49999997)
        x[:20] = np.float32(0.49999997)
        for off, path in ((0, "stage"), (3, "stage"), (0, "auto"), (3, "auto")):      # auto: the companion library serves reference-layout mode too (round 5)
            buf = np.zeros(n + 32, dtype=np.uint8)
            base = (-buf.ctypes.data) % 16
            out = buf[base + off: base + off + n]
            ctx.reset_stream()
            ctx.set_blocking(True)
            ctx.set_host_path(path)
            ctx.quantize_ptr(x.ctypes.data, piquant.DataType.F32, out.ctypes.data, piquant.DataType.UINT8, n, 1.0, 0, piquant.RoundMode.NEAREST)
            wbuf = np.zeros(n + 32, dtype=np.uint8)
            wbase = (-wbuf.ctypes.data) % 16
            want = O.quantize(x, O.F32, O.UINT8, 1.0, 0, form=O.FORM_REFERENCE, out=wbuf[wbase + off: wbase + off + n])
            assert np.array_equal(out, want), off
            if off == 0:
                assert out[-1] == 0 and out[0] == 1     # tail of 13: the scalar formula rounds 0.49999997 down; no head, body rounds up
            else:
                assert out[0] == 0 and out[-1] == 1     # head of 13 scalar elements, and (n - 13) % 64 == 0: no tail
    finally:
        ctx.set_host_path("auto")
        ctx.set_reference_layout(False)
    # with the mode off every position rounds it up, like the SIMD body
    got = gpu_quantize(ctx, np.full(37, 0.49999997, dtype=np.float32), O.F32, O.UINT8, 1.0, 0)
    assert (got == 1).all()


# ---------------------------------------------------------------------------------------------------
# compute_quant_params + quantize as one launch, tensor resident on chip (piquant_hip_quantize_dynamic, fused_kernels.hpp)
# ---------------------------------------------------------------------------------------------------
def gpu_quantize_dynamic(ctx, x, dt_in, dt_out, round_mode=0, offset_in=0):
    """-> (packed bytes, (scale, zero_point)) through the C ABI, with guard bytes around the output checked."""
    import struct

    import piquant
    import torch

    n = x.size
    nbytes = piquant.DataType(dt_out).packed_nbytes(n)
    xin, pin = to_device(x, offset_in)
    obuf = torch.full((nbytes + 128,), 0xAA, dtype=torch.uint8, device="cuda")
    out = obuf[64: 64 + nbytes]
    rec = torch.zeros(16, dtype=torch.uint8, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_dynamic_ptr(pin if n else 0, piquant.DataType(dt_in), out.data_ptr() if n else 0, piquant.DataType(dt_out), n, rec.data_ptr(),
                             piquant.RoundMode(round_mode))
    torch.cuda.synchronize()
    assert bool((obuf[:64] == 0xAA).all()) and bool((obuf[64 + nbytes:] == 0xAA).all()), "kernel wrote outside the output"
    scale, _inv, zp = struct.unpack("<ffq", rec.cpu().numpy().tobytes())
    return out.cpu().numpy(), (scale, zp)


def _dynamic_cases(rng, n):
    base = rng.uniform(-2, 3, n).astype(np.float32)
    yield "uniform", base
    with_nan = base.copy()
    with_nan[rng.choice(n, max(1, n // 50))] = np.nan
    with_nan[rng.choice(n, max(1, n // 70))] = -np.nan
    if not np.isnan(with_nan).all():
        yield "nan", with_nan
    yield "constant", np.full(n, 42.0, np.float32)
    yield "far from zero", (np.float32(1e12) + rng.uniform(0, 1e6, n)).astype(np.float32)     # x/scale beyond 2^31: every step hits the x86 indefinite
    yield "all negative", rng.uniform(-6, -2, n).astype(np.float32)
    yield "huge range", (rng.normal(size=n) * 1e30).astype(np.float32)
    # an infinity in the data: the reference's epilogue returns (inf, 0) -- inf passes its `scale >= 0` assertion (src/piquant.cpp:373) -- and
    # quantizing with it is legal (1/scale = 0: every finite product is 0, inf * 0 is NaN -> the x86 indefinite -> 0)
    for name, vals in (("plus inf", [np.inf]), ("minus inf", [-np.inf]), ("both inf", [np.inf, -np.inf])):
        with_inf = base.copy()
        with_inf[rng.choice(n, min(n, len(vals)), replace=False)] = vals[: min(n, len(vals))]
        yield name, with_inf
    full = base.copy()                                   # +-FLT_MAX: the range only fits in the epilogue's doubles; uint2's 1/scale is a denormal
    full[rng.choice(n, min(n, 2), replace=False)] = [3.4028235e38, -3.4028235e38][: min(n, 2)]
    yield "whole float range", full
    yield "denormals only", (rng.uniform(-1, 1, n) * 1e-41).astype(np.float32)      # a denormal scale: 1/scale overflows to inf, every product is +-inf or NaN
    yield "tiny range", (np.float32(1e-30) * rng.uniform(-1, 1, n)).astype(np.float32)


def test_fused_dynamic_quantize_matches_oracle_and_unfused_path(O):
    import piquant

    rng = np.random.default_rng(2024)
    fused, plain = piquant.Context(), piquant.Context()
    plain.set_fusion(False)
    checked = 0
    for n in (1, 2, 3, 5, 63, 64, 65, 1000, 4097, 262_144 * 4, 262_144 * 4 + 5, 1_000_003):
        for dt_in in (0, 1):
            for dt_out in (4, 3, 2):
                for name, x in _dynamic_cases(rng, n):
                    if n > 5000 and name not in ("uniform", "nan", "far from zero"):
                        continue
                    xin = x if dt_in == 0 else O.f32_to_bf16(x)
                    # the scan ignores NaNs (v_min/v_max return the other operand); the reference leaves them unspecified
                    finite = xin[~np.isnan(x)] if name == "nan" else xin
                    want_p = O.compute_quant_params(finite, dt_in, dt_out)
                    if np.isnan(want_p[0]) or want_p[0] < 0:
                        continue          # the reference aborts on such a scale (src/piquant.cpp:373); nothing to compare
                    want = O.quantize(xin, dt_in, dt_out, want_p[0], want_p[1])
                    got, got_p = gpu_quantize_dynamic(fused, xin, dt_in, dt_out)
                    assert (np.float32(got_p[0]).tobytes(), got_p[1]) == (np.float32(want_p[0]).tobytes(), want_p[1]), (n, dt_in, dt_out, name)
                    assert np.array_equal(got, want), (n, dt_in, dt_out, name)
                    got3, got3_p = gpu_quantize_dynamic(plain, xin, dt_in, dt_out)
                    assert got3_p == got_p and np.array_equal(got3, got), (n, dt_in, dt_out, name)
                    checked += 1
    assert checked > 300


def test_fused_dynamic_quantize_stochastic_modes(O):
    import piquant

    rng = np.random.default_rng(2025)
    c = piquant.Context()
    for n in (7, 1000, 300_001):
        x = rng.uniform(-2, 3, n).astype(np.float32)
        for dt_in in (0, 1):
            xin = x if dt_in == 0 else O.f32_to_bf16(x)
            for dt_out in (4, 3, 2):
                scale, zp = O.compute_quant_params(xin, dt_in, dt_out)
                c.set_stochastic_per_element(False)
                c.set_stochastic_threshold(0.3125)
                got, p = gpu_quantize_dynamic(c, xin, dt_in, dt_out, 1)
                assert p == (scale, zp) and np.array_equal(got, O.quantize(xin, dt_in, dt_out, scale, zp, 1, 0.3125)), (n, dt_in, dt_out)
                c.set_stochastic_threshold(None)
                c.set_stochastic_per_element(True, seed=99, index_base=(1 << 32) - 1000)
                got, p = gpu_quantize_dynamic(c, xin, dt_in, dt_out, 1)
                assert p == (scale, zp) and np.array_equal(got, O.quantize_per_element(xin, dt_in, dt_out, scale, zp, 99, (1 << 32) - 1000)), (n, dt_in, dt_out)


def test_fused_dynamic_quantize_capacity_boundary_headline_size_and_misalignment(O):
    """The largest tensor the chip holds (27 rounds x 1024 threads x 16 B per CU), one vector more and 1.5x that (part of every
    block's share streamed twice), the largest size the fused kernel takes (64 rounds) and one vector more (two launches), the
    BASELINE size, a misaligned input (fallback), and the stochastic / per-element modes over a streamed remainder: all equal
    the oracle."""
    import piquant
    import torch

    c = piquant.Context()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fits = 27 * 1024 * cus * 4
    rng = np.random.default_rng(5)
    limit = 64 * 1024 * cus * 4
    for n, off in ((fits, 0), (fits + 4, 0), (fits + 3, 0), (fits * 3 // 2 + 7, 0), (limit, 0), (limit + 4, 0), (N1, 0), (100_003, 4)):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        x[n // 3] = 1.5
        x[n - 5] = -1.25                      # the minimum sits in the streamed part of the last block's share
        scale, zp = O.compute_quant_params(x, 0, 4)
        got, p = gpu_quantize_dynamic(c, x, 0, 4, offset_in=off)
        assert p == (scale, zp), (n, off)
        assert np.array_equal(got, O.quantize(x, 0, 4, scale, zp)), (n, off)
    # other modes and dtypes over a streamed remainder
    n = fits + fits // 3 + 11
    x = rng.uniform(-2, 3, n).astype(np.float32)
    xb = O.f32_to_bf16(rng.uniform(-2, 3, 2 * n).astype(np.float32))
    c.set_stochastic_threshold(0.4375)
    scale, zp = O.compute_quant_params(x, 0, 3)
    got, p = gpu_quantize_dynamic(c, x, 0, 3, 1)
    assert p == (scale, zp) and np.array_equal(got, O.quantize(x, 0, 3, scale, zp, 1, 0.4375))
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(True, seed=5, index_base=123)
    got, p = gpu_quantize_dynamic(c, x, 0, 4, 1)
    scale, zp = O.compute_quant_params(x, 0, 4)
    assert p == (scale, zp) and np.array_equal(got, O.quantize_per_element(x, 0, 4, scale, zp, 5, 123))
    c.set_stochastic_per_element(False)
    scale, zp = O.compute_quant_params(xb, 1, 3)
    got, p = gpu_quantize_dynamic(c, xb, 1, 3)
    assert p == (scale, zp) and np.array_equal(got, O.quantize(xb, 1, 3, scale, zp))


def test_fused_dynamic_quantize_from_two_streams_and_contexts(O):
    """Fused launches carry a grid barrier; launches issued on different streams are ordered behind one another by the library.
    Interleave two contexts on two streams without synchronising in between and check every result."""
    import piquant
    import torch

    rng = np.random.default_rng(77)
    n = 2_000_003
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [piquant.Context(), piquant.Context()]
    xs = [rng.uniform(-1 - i, 2 + i, n).astype(np.float32) for i in range(6)]
    xd = [torch.from_numpy(x).cuda() for x in xs]
    outs = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in xs]
    recs = [torch.zeros(16, dtype=torch.uint8, device="cuda") for _ in xs]
    torch.cuda.synchronize()
    for rep in range(20):
        for i in range(len(xs)):
            with torch.cuda.stream(streams[i % 2]):
                piquant.torch.quantize_dynamic(xd[i], dtype=torch.uint8, ctx=ctxs[i % 2], out=outs[i], params=recs[i])
    torch.cuda.synchronize()
    for i, x in enumerate(xs):
        scale, zp = O.compute_quant_params(x, 0, 4)
        assert piquant.torch.params_to_host(recs[i]) == (scale, zp)
        assert np.array_equal(outs[i].cpu().numpy(), O.quantize(x, 0, 4, scale, zp))


def test_dequantize_sum_equals_sequential_adds(O):
    """piquant_hip_dequantize_sum: K quantized inputs with their own device parameter records summed in one pass == the K
    dequantize calls in order (and == the oracle), for every dtype pair, SET and ADD, ragged sizes, 1..17 inputs (one launch takes
    16) and a misaligned accumulator."""
    import piquant
    import piquant.torch as pt
    import torch

    rng = np.random.default_rng(404)
    tq = {4: torch.quint8, 3: torch.quint4x2, 2: torch.quint2x4}
    for n in (1, 7, 1000, 4099, 300_001):
        for dt_q in (4, 3, 2):
            for f_name, fdt, dt_f in (("f32", torch.float32, 0), ("bf16", torch.bfloat16, 1)):
                for K in (1, 3, 17) if n == 4099 else (1, 3):
                    xs = [rng.uniform(-1 - i, 2 + 0.5 * i, n).astype(np.float32) for i in range(K)]
                    qs, recs, hp = [], [], []
                    for x in xs:
                        q, rec = pt.quantize_dynamic(torch.from_numpy(x).cuda(), dtype=tq[dt_q])
                        qs.append(pt.packed_bytes(q))
                        recs.append(rec)
                        hp.append(pt.params_to_host(rec))
                    prev = rng.uniform(-3, 3, n).astype(np.float32)
                    prev_in = prev if dt_f == 0 else O.f32_to_bf16(prev)
                    for op in ("set", "add"):
                        # oracle: the calls one after the other
                        want = prev_in.copy()
                        for i in range(K):
                            want = O.dequantize(qs[i].cpu().numpy(), dt_q, dt_f, n, hp[i][0], hp[i][1], 1 if (op == "add" or i > 0) else 0, out=want)
                        for off in (0, 1) if n in (1000, 300_001) else (0,):
                            buf = torch.zeros(n + 8 if dt_f == 0 else n + 16, dtype=fdt, device="cuda")
                            acc = buf[off: off + n]
                            src = torch.from_numpy(prev_in).cuda() if dt_f == 0 else torch.from_numpy(prev_in.view(np.int16)).cuda().view(torch.bfloat16)
                            acc.copy_(src)
                            qs_in = qs
                            if off:   # packed inputs that start on odd bytes as well: with an element-aligned accumulator the vector path takes all of it
                                qs_in = []
                                for i, q in enumerate(qs):
                                    holder = torch.zeros(q.numel() + 16, dtype=torch.uint8, device="cuda")
                                    holder[1 + 2 * (i % 3): 1 + 2 * (i % 3) + q.numel()].copy_(q)
                                    qs_in.append(holder[1 + 2 * (i % 3): 1 + 2 * (i % 3) + q.numel()])
                            pt.dequantize_sum(qs_in, recs, dtype=fdt, reduce_op=op, out=acc, quant_dtype=tq[dt_q], shape=(n,))
                            got = acc.cpu().numpy() if dt_f == 0 else acc.view(torch.int16).cpu().numpy().view(np.uint16)
                            assert same_floats(got, want), (n, dt_q, f_name, K, op, off)
                            assert bool((buf[:off] == 0).all()) and bool((buf[off + n:] == 0).all())


def test_batched_dynamic_quantize_and_dequantize_equal_single_calls(O):
    """quantize_dynamic_batch / dequantize_dynamic_batch: up to 16 independent tensors per launch, each with its own parameters --
    every output and record must equal the single-tensor calls (and the oracle); ragged and empty tensors, a misaligned one (drops the
    whole group to single calls), more than 16 tensors, a tensor too large for its sub-grid, stochastic mode."""
    import piquant
    import piquant.torch as pt
    import torch

    rng = np.random.default_rng(909)
    ctx = piquant.Context()
    tq = {4: torch.quint8, 3: torch.quint4x2, 2: torch.quint2x4}
    size_sets = [
        [3_407_872] * 7,                                  # the chunks of an 8-way all-reduce of the BASELINE tensor
        [1, 7, 1000, 4099, 65_536, 300_001, 5],
        [2000 + 17 * i for i in range(19)],               # more than one launch's worth
        [5_000_000, 100, 5_000_000],                      # 15 rounds per block of a third of a 256-CU chip: one launch (a batch is refused from 65 rounds on, kFusedMaxRounds: tests/test_gpu_dynamic_wire_edges.py)
    ]
    for sizes in size_sets:
        for dt_f, fdt in ((0, torch.float32), (1, torch.bfloat16)):
            for dt_q in (4, 3) if sizes[0] > 1_000_000 else (4, 3, 2):
                for rm, tau in ((0, 0.0), (1, 0.625)):
                    if rm and dt_q == 2:
                        continue
                    xs = [rng.uniform(-1 - 0.1 * i, 2 + 0.2 * i, n).astype(np.float32) for i, n in enumerate(sizes)]
                    xin = [x if dt_f == 0 else O.f32_to_bf16(x) for x in xs]
                    xd = [torch.from_numpy(x).cuda() if dt_f == 0 else torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) for x in xin]
                    ctx.set_stochastic_threshold(tau if rm else None)
                    qs, recs = pt.quantize_dynamic_batch(xd, dtype=tq[dt_q], round_mode="stochastic" if rm else "nearest", ctx=ctx)
                    torch.cuda.synchronize()
                    for i, x in enumerate(xin):
                        scale, zp = O.compute_quant_params(x, dt_f, dt_q)
                        assert pt.params_to_host(recs[i]) == (scale, zp), (sizes, i)
                        assert np.array_equal(pt.packed_bytes(qs[i]).cpu().numpy(), O.quantize(x, dt_f, dt_q, scale, zp, rm, tau)), (sizes, dt_f, dt_q, rm, i)
                    # and back, SET then ADD, in one launch per 16
                    back = pt.dequantize_dynamic_batch(qs, recs, dtype=fdt, ctx=ctx)
                    accs = [torch.ones_like(b) for b in back]
                    pt.dequantize_dynamic_batch(qs, recs, dtype=fdt, reduce_op="add", outs=accs, ctx=ctx)
                    for i, x in enumerate(xin):
                        scale, zp = pt.params_to_host(recs[i])
                        qb = pt.packed_bytes(qs[i]).cpu().numpy()
                        want = O.dequantize(qb, dt_q, dt_f, x.size, scale, zp)
                        ones = np.ones(x.size, np.float32) if dt_f == 0 else O.f32_to_bf16(np.ones(x.size, np.float32))
                        want_acc = O.dequantize(qb, dt_q, dt_f, x.size, scale, zp, 1, out=ones)
                        got = back[i].cpu().numpy() if dt_f == 0 else back[i].view(torch.int16).cpu().numpy().view(np.uint16)
                        got_acc = accs[i].cpu().numpy() if dt_f == 0 else accs[i].view(torch.int16).cpu().numpy().view(np.uint16)
                        assert same_floats(got, want) and same_floats(got_acc, want_acc), (sizes, dt_f, dt_q, i)
    ctx.set_stochastic_threshold(None)
    # an empty tensor and a misaligned one inside a batch
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1000, 0, 3000)]
    big = torch.zeros(3004, device="cuda")
    xd = [torch.from_numpy(xs[0]).cuda(), torch.empty(0, device="cuda"), big[1:3001]]
    xd[2].copy_(torch.from_numpy(xs[2]))
    qs, recs = pt.quantize_dynamic_batch(xd, dtype=torch.quint8, ctx=ctx)
    for i in (0, 2):
        scale, zp = O.compute_quant_params(xs[i], 0, 4)
        assert pt.params_to_host(recs[i]) == (scale, zp)
        assert np.array_equal(pt.packed_bytes(qs[i]).cpu().numpy(), O.quantize(xs[i], 0, 4, scale, zp))
    assert pt.params_to_host(recs[1]) == (1.0, 127)   # nothing scanned: the degenerate record, never a negative scale (include/piquant_hip.h)
    # batched dequantize into slices that are only element-aligned, from packed inputs on odd bytes: still the vector path, same floats
    for dt_q in (4, 3, 2):
        for dt_f, fdt in ((0, torch.float32), (1, torch.bfloat16)):
            xs = [rng.uniform(-2, 1, n).astype(np.float32) for n in (300_001, 4099, 70_000)]
            xd = [torch.from_numpy(x).cuda() for x in xs]
            qs, recs = pt.quantize_dynamic_batch(xd, dtype=tq[dt_q], ctx=ctx)
            qb = [pt.packed_bytes(q) for q in qs]
            odd = []
            for i, q in enumerate(qb):
                holder = torch.zeros(q.numel() + 8, dtype=torch.uint8, device="cuda")
                holder[1 + i: 1 + i + q.numel()].copy_(q)
                odd.append(holder[1 + i: 1 + i + q.numel()])
            bufs = [torch.full((x.size + 8,), 1.0, dtype=fdt, device="cuda") for x in xs]
            outs = [b[1 + i: 1 + i + x.size] for i, (b, x) in enumerate(zip(bufs, xs))]
            pt.dequantize_dynamic_batch(odd, recs, dtype=fdt, reduce_op="add", outs=outs, quant_dtype=tq[dt_q], shapes=[(x.size,) for x in xs], ctx=ctx)
            for i, x in enumerate(xs):
                scale, zp = pt.params_to_host(recs[i])
                ones = np.ones(x.size, np.float32) if dt_f == 0 else O.f32_to_bf16(np.ones(x.size, np.float32))
                want = O.dequantize(qb[i].cpu().numpy(), dt_q, dt_f, x.size, scale, zp, 1, out=ones)
                got = outs[i].cpu().numpy() if dt_f == 0 else outs[i].view(torch.int16).cpu().numpy().view(np.uint16)
                assert same_floats(got, want), (dt_q, dt_f, i)
                edge = bufs[i].float()
                assert bool((edge[: 1 + i] == 1).all()) and bool((edge[1 + i + x.size:] == 1).all())


def test_reduce_quantize_dynamic_equals_sum_then_quantize(O):
    """piquant_hip_reduce_quantize_dynamic: quantize(acc + sum of dequantized inputs) with parameters from the sum, in one launch that
    keeps the sum on chip.  Bytes and record must equal dequantize_sum followed by quantize_dynamic (and the oracle) for every dtype
    pair, rounding mode, 1..7 terms; ragged / oversized tensors take the two-step form and must agree as well."""
    import piquant
    import piquant.torch as pt
    import torch

    rng = np.random.default_rng(1312)
    ctx = piquant.Context()
    tq = {4: torch.quint8, 3: torch.quint4x2, 2: torch.quint2x4}
    checked = 0
    for n in (8, 4096, 70_000, 3_407_872, 3_407_875, 24_000_000):
        for dt_f, fdt in ((0, torch.float32), (1, torch.bfloat16)):
            for dt_q in (4, 3, 2):
                if n > 5_000_000 and (dt_q != 4 or dt_f != 0):
                    continue
                for K in (1, 7) if n >= 3_000_000 else (1, 3):
                    for rm, tau in ((0, 0.0), (1, 0.28125)):
                        if rm and (dt_q == 2 or n > 5_000_000):
                            continue
                        own = rng.uniform(-2, 2, n).astype(np.float32)
                        own_in = own if dt_f == 0 else O.f32_to_bf16(own)
                        terms = [rng.uniform(-1 - i, 1 + 0.5 * i, n).astype(np.float32) for i in range(K)]
                        qs, recs, want_acc = [], [], own_in.copy()
                        for t in terms:
                            q, rec = pt.quantize_dynamic(torch.from_numpy(t).cuda(), dtype=tq[dt_q], ctx=ctx)
                            qs.append(pt.packed_bytes(q))
                            recs.append(rec)
                            s_k, z_k = pt.params_to_host(rec)
                            want_acc = O.dequantize(qs[-1].cpu().numpy(), dt_q, dt_f, n, s_k, z_k, 1, out=want_acc)
                        want_p = O.compute_quant_params(want_acc, dt_f, dt_q)
                        want_q = O.quantize(want_acc, dt_f, dt_q, want_p[0], want_p[1], rm, tau)
                        acc = torch.from_numpy(own_in).cuda() if dt_f == 0 else torch.from_numpy(own_in.view(np.int16)).cuda().view(torch.bfloat16)
                        ctx.set_stochastic_threshold(tau if rm else None)
                        out, rec = pt.reduce_quantize_dynamic(acc, qs, recs, dtype=tq[dt_q], round_mode="stochastic" if rm else "nearest", ctx=ctx)
                        assert pt.params_to_host(rec) == want_p, (n, dt_f, dt_q, K, rm)
                        assert np.array_equal(pt.packed_bytes(out).cpu().numpy(), want_q), (n, dt_f, dt_q, K, rm)
                        checked += 1
    ctx.set_stochastic_threshold(None)
    assert checked > 60


def test_independent_calls_mode_same_bytes_and_later_work_waits(ctx, O):
    """piquant_hip_set_independent_calls (round 5): quantize / dequantize launches without the barrier bit of their dispatch packets -- consecutive
    calls overlap at their edges.  The caller's promise (no call depends on work still in flight) holds here: distinct tensors.  Every call's bytes
    equal the oracle's, work enqueued BEHIND the calls (a torch reduction over all outputs, a device-to-host copy) sees all of them complete, and
    with the mode off again a dependent chain (quantize -> dequantize of the same buffer) is ordered as always."""
    import piquant
    import torch

    c = piquant.Context()
    rng = np.random.default_rng(2025)
    xs = [rng.uniform(-2, 2, n).astype(np.float32) for n in (3_000_001, 27_264_000 // 4, 4096, 1_000_003, 5_000_000, 77)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = [torch.from_numpy(x).cuda() for x in xs]
        qd = [torch.zeros(x.size, dtype=torch.uint8, device="cuda") for x in xs]
        q4 = [torch.zeros((x.size + 1) // 2, dtype=torch.uint8, device="cuda") for x in xs]
        back = [torch.zeros(x.size, dtype=torch.float32, device="cuda") for x in xs]
        torch.cuda.synchronize()          # the inputs are complete: nothing the calls below depend on is in flight
        with c.independent_calls():
            for rep in range(3):
                for x, q, p4 in zip(xd, qd, q4):
                    piquant.torch.quantize(x, scale=0.0157, zero_point=128, dtype=torch.uint8, ctx=c, out=q)
                    piquant.torch.quantize(x, scale=0.27, zero_point=7, dtype=torch.quint4x2, ctx=c, out=p4)
            total = sum(int(q.sum(dtype=torch.int64)) for q in qd)      # torch kernels behind the any-order launches: they wait for all of them
        for q, b in zip(qd, back):        # dependent on the quantize calls above: issued with the mode off, ordered as always
            piquant.torch.dequantize(q, scale=0.0157, zero_point=128, dtype=torch.float32, ctx=c, out=b)
    torch.cuda.synchronize()
    want_total = 0
    for x, q, p4, b in zip(xs, qd, q4, back):
        want = O.quantize(x, 0, 4, 0.0157, 128)
        assert np.array_equal(q.cpu().numpy(), want)
        assert np.array_equal(p4.cpu().numpy(), O.quantize(x, 0, 3, 0.27, 7))
        assert same_floats(b.cpu().numpy(), O.dequantize(want, 4, 0, x.size, 0.0157, 128))
        want_total += int(want.astype(np.int64).sum())
    assert total == want_total


# ---------------------------------------------------------------------------------------------------
# degenerate parameters: the reference validates dtypes and sizes only (src/piquant.cpp:286-295, 319-327) -- ANY float is a legal scale
# ---------------------------------------------------------------------------------------------------
# 0 and -0 (1/scale = +-inf: every product is +-inf or NaN), +-inf (1/scale = 0), NaN, negative scales, denormal scales (1/scale overflows to inf),
# scales whose reciprocal is denormal (3e38, 8.6e37, FLT_MAX), the smallest normal, 2^-127 and the smallest denormal
DEGENERATE_SCALES = [0.0, -0.0, np.inf, -np.inf, np.nan, -0.05, -1.0, 1e-40, -1e-40, 3e38, -3e38, 1.1754944e-38, 3.4028235e38, 1e-45, 2.0 ** -126, 2.0 ** -127, 8.6e37]


@pytest.mark.parametrize("dt_in", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("dt_out", [4, 3, 2], ids=["u8", "u4", "u2"])
def test_quantize_with_degenerate_scales(ctx, O, dt_in, dt_out):
    """Every such scale through every quantizer, both rounding modes, sizes that take the vector tiles and the ragged ends, data with zeros of both
    signs, NaN, infinities, a denormal and a huge value: bytes equal the oracle's -- which equals the reference's own AVX-512 kernels on exactly
    these parameters (tests/test_oracle_vs_ref.py::test_degenerate_scales_against_reference_kernels, where oracle/_ref is built)."""
    rng = np.random.default_rng(4100 + 10 * dt_in + dt_out)
    for n in (1, 65, 4099, 70_001):
        x = rng.uniform(-3, 3, n).astype(np.float32)
        if n > 20:
            x[[1, 3, 5, 7, 9, 11, 13, 15, 17]] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e38, 3.3e38, -3.3e38]   # the last two: products of about +-1.1 with a DENORMAL 1/scale
        xin = x if dt_in == 0 else O.f32_to_bf16(x)
        for scale in DEGENERATE_SCALES:
            for zp in (0, 3, 200, -7):
                for rm, tau in ((0, 0.0), (1, 0.37)):
                    ctx.set_stochastic_threshold(tau if rm else None)
                    got = gpu_quantize(ctx, xin, dt_in, dt_out, float(scale), zp, rm)
                    want = O.quantize(xin, dt_in, dt_out, float(scale), zp, rm, tau, form=O.FORM_UNIFORM)
                    assert np.array_equal(got, want), (n, scale, zp, rm, np.nonzero(got != want)[0][:5], got[:8], want[:8])
    ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("dt_q", [4, 3, 2], ids=["u8", "u4", "u2"])
@pytest.mark.parametrize("dt_f", [0, 1], ids=["f32", "bf16"])
def test_dequantize_with_degenerate_scales_and_nonfinite_accumulators(ctx, O, dt_q, dt_f):
    """The same scales through every dequantizer, SET and ADD, with NaN, +-inf and a value next to FLT_MAX sitting in the accumulator.  Float results
    are compared bit for bit except that any NaN equals any NaN (payloads and signs of NaNs are outside the contract: the reference's own AVX-512F
    body and its scalar tail already disagree about them -- 0x7fc1 against 0x7fc0 for the bf16 image of the default NaN, kernels_specialized.inl:14-33
    against piquant.hpp:86-90)."""
    rng = np.random.default_rng(4200 + 10 * dt_q + dt_f)
    for n in (1, 65, 4099, 70_001):
        q = rng.integers(0, 256, O.packed_numel(n, dt_q)).astype(np.uint8)
        prev = rng.uniform(-5, 5, n).astype(np.float32)
        if n > 20:
            prev[[2, 4, 6, 8]] = [np.nan, np.inf, -np.inf, 3e38]
        prev = prev if dt_f == 0 else O.f32_to_bf16(prev)
        for scale in DEGENERATE_SCALES:
            for zp in (0, 3, 200, -7):
                for op in (0, 1):
                    got = gpu_dequantize(ctx, q, dt_q, dt_f, n, float(scale), zp, op, prev=prev)
                    want = O.dequantize(q, dt_q, dt_f, n, float(scale), zp, op, form=O.FORM_UNIFORM, out=prev.copy())
                    assert same_floats(got, want), (n, scale, zp, op)


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_requantize_with_degenerate_scales(ctx, O, dt):
    rng = np.random.default_rng(4300 + dt)
    n = 4099
    x = rng.uniform(-3, 3, n).astype(np.float32)
    x[[1, 3, 5, 7, 9, 11, 13, 15, 17]] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e38, 3.3e38, -3.3e38]   # the last two: products of about +-1.1 with a DENORMAL 1/scale
    xin = x if dt == 0 else O.f32_to_bf16(x)
    prev = rng.uniform(-5, 5, n).astype(np.float32)
    prev = prev if dt == 0 else O.f32_to_bf16(prev)
    for qd in (4, 3, 2):
        for scale in DEGENERATE_SCALES:
            for zp in (0, 3, -7):
                for rm, tau in ((0, 0.0), (1, 0.37)):
                    ctx.set_stochastic_threshold(tau if rm else None)
                    for op in (0, 1):
                        got = gpu_requantize(ctx, xin, dt, qd, float(scale), zp, rm, op, prev)
                        want = O.requantize(xin, dt, qd, float(scale), zp, rm, tau, op, out=prev.copy())
                        assert same_floats(got, want), (qd, scale, zp, rm, op)
    ctx.set_stochastic_threshold(None)


def test_reference_layout_with_degenerate_scales(ctx, O):
    """The same degenerate scales in reference-layout mode: the scalar heads and tails of a one- and a three-thread reference context take the
    reference's scalar formulas (std::round, the (q - zp) * scale form of the bf16 tails) on +-inf / NaN / denormal reciprocals too."""
    rng = np.random.default_rng(4400)
    try:
        for threads in (1, 3):
            ctx.set_reference_layout(True, threads=threads)
            for n in (65, 4099):
                x = rng.uniform(-3, 3, n).astype(np.float32)
                x[[1, 3, 5, 7, 9, 11, 13, 15, 17]] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e38, 3.3e38, -3.3e38]
                x[-3:] = [0.49999997, 3.3e38, np.nan]                           # in the last partition's scalar tail
                for scale in DEGENERATE_SCALES:
                    for zp in (3, -7):
                        for dt_in, xin in ((O.F32, x), (O.BF16, O.f32_to_bf16(x))):
                            for dt_out in (O.UINT8, O.UINT4, O.UINT2):
                                for rm, tau in ((0, 0.0), (1, 0.37)):
                                    ctx.set_stochastic_threshold(tau if rm else None)
                                    nbytes = O.packed_numel(n, dt_out)
                                    wbuf = np.zeros(nbytes + 32, dtype=np.uint8)
                                    base = (-wbuf.ctypes.data) % 16
                                    want = O.quantize(xin, dt_in, dt_out, float(scale), zp, rm, tau, form=O.FORM_REFERENCE, threads=threads, out=wbuf[base: base + nbytes])
                                    got = gpu_quantize(ctx, xin, dt_in, dt_out, float(scale), zp, rm)
                                    assert np.array_equal(got, want), (threads, n, scale, zp, dt_in, dt_out, rm, np.nonzero(got != want)[0][:5])
                        for dt_q in (O.UINT8, O.UINT4, O.UINT2):
                            q = rng.integers(0, 256, O.packed_numel(n, dt_q), dtype=np.uint8)
                            for dt_f in (O.F32, O.BF16):
                                prev = rng.uniform(-3, 3, n).astype(np.float32)
                                prev[[2, 4, n - 1]] = [np.nan, np.inf, -np.inf]
                                prev = prev if dt_f == O.F32 else O.f32_to_bf16(prev)
                                for op in (0, 1):
                                    want = O.dequantize(q, dt_q, dt_f, n, float(scale), zp, op, form=O.FORM_REFERENCE, threads=threads, out=prev.copy())
                                    got = gpu_dequantize(ctx, q, dt_q, dt_f, n, float(scale), zp, op, prev=prev.copy())
                                    assert same_floats(got, want), (threads, n, scale, zp, dt_q, dt_f, op)
    finally:
        ctx.set_reference_layout(False, threads=1)
        ctx.set_stochastic_threshold(None)


def test_reference_layout_partitions_at_full_size(ctx, O):
    """Round 5: reference-layout mode with scalar positions inside the tensor (partitions of a T-thread reference context, a misaligned output) no
    longer takes the element-by-element kernels (124-213 us at numel 27 264 000): the vector kernels run in the uniform form and patch kernels rewrite
    the partitions' heads and tails (quantize_ref_patch_kernel, dequantize_ref_patch_kernel).  255 and 3 partitions of the BASELINE tensor, salted with
    the values on which the reference's formulas differ -- also exactly at the partition boundaries -- against the oracle's threaded reference form;
    stream-ordered, blocking in every wait mode, and with the calls declared independent."""
    import piquant
    import torch

    rng = np.random.default_rng(255)
    n = N1
    x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
    x[rng.choice(n, n // 50)] = np.float32(0.49999997)
    x[rng.choice(n, n // 60)] = np.float32(-0.49999997)
    x[rng.choice(n, n // 70)] = np.float32(8388609.0)
    q8 = rng.integers(0, 256, n, dtype=np.uint8)
    prev = rng.uniform(-3, 3, n).astype(np.float32)
    try:
        for threads in (255, 3):
            edges = np.unique(np.clip(np.concatenate([(n * np.arange(1, threads) // threads)[:, None] + np.arange(-70, 20)[None, :]]).ravel(), 0, n - 1))
            x[edges] = rng.choice(np.array([0.49999997, -0.49999997, 8388609.0, 0.3], np.float32), edges.size)
            xb = O.f32_to_bf16(x)
            ctx.set_reference_layout(True, threads=threads)
            for dt_in, xin, dt_out, off in ((O.F32, x, O.UINT8, 0), (O.F32, x, O.UINT8, 5), (O.BF16, xb, O.UINT4, 0), (O.BF16, xb, O.UINT2, 0)):
                nbytes = O.packed_numel(n, dt_out)
                wbuf = np.zeros(nbytes + 32, dtype=np.uint8)
                base = (-wbuf.ctypes.data) % 16
                want = O.quantize(xin, dt_in, dt_out, 1.0, 1, form=O.FORM_REFERENCE, threads=threads, out=wbuf[base + off: base + off + nbytes])
                got = gpu_quantize(ctx, xin, dt_in, dt_out, 1.0, 1, offset_out=off)
                assert np.array_equal(got, want), (threads, dt_in, dt_out, off, np.nonzero(got != want)[0][:8])
                if dt_in == O.F32 and threads == 255:      # (bf16 has no value on which the nearest formulas differ: 0.49999997 and 8388609 are not bf16 numbers;
                    #  three partitions of 27 264 000 elements are whole SIMD blocks: no tails, and heads only in front of a misaligned output)
                    assert not np.array_equal(want, O.quantize(xin, dt_in, dt_out, 1.0, 1, form=O.FORM_UNIFORM)), "the salt never met a scalar position"
            for dt_q, dt_f, op in ((O.UINT4, O.BF16, 0), (O.UINT4, O.BF16, 1), (O.UINT8, O.BF16, 1), (O.UINT2, O.BF16, 1), (O.UINT2, O.F32, 1), (O.UINT8, O.F32, 1)):
                q = q8[: O.packed_numel(n, dt_q)]
                pv = prev if dt_f == O.F32 else O.f32_to_bf16(prev)
                want = O.dequantize(q, dt_q, dt_f, n, 0.3, 2, op, form=O.FORM_REFERENCE, threads=threads, out=pv.copy())
                got = gpu_dequantize(ctx, q, dt_q, dt_f, n, 0.3, 2, op, prev=pv.copy())
                assert same_floats(got, want), (threads, dt_q, dt_f, op)
        # the same call as a blocking call in every wait mode (the patch kernel carries the completion signal, not the vector kernel in front of it),
        # and as an independent call (only the first launch of the sequence may go out of order)
        ctx.set_reference_layout(True, threads=7)
        m = 3_000_001
        xs = x[:m].copy()
        wbuf = np.zeros(m + 32, dtype=np.uint8)
        base = (-wbuf.ctypes.data) % 16
        want = O.quantize(xs, O.F32, O.UINT8, 1.0, 1, form=O.FORM_REFERENCE, threads=7, out=wbuf[base: base + m]).copy()
        xd = torch.from_numpy(xs).cuda()
        for mode in ('sync', 'write32', 'kernel', 'event'):
            out = torch.zeros(m, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.reset_stream()
            ctx.set_blocking(True)
            ctx.set_blocking_wait(mode)
            ctx.quantize_ptr(xd.data_ptr(), piquant.DataType.F32, out.data_ptr(), piquant.DataType.UINT8, m, 1.0, 1, piquant.RoundMode.NEAREST)
            host = torch.empty(m, dtype=torch.uint8).pin_memory()
            host.copy_(out, non_blocking=True)          # on another stream than the call's: correct only if the call really completed
            torch.cuda.synchronize()
            assert np.array_equal(host.numpy(), want), mode
        ctx.set_blocking_wait('kernel')
        ctx.set_blocking(False)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            outs = [torch.zeros(m, dtype=torch.uint8, device="cuda") for _ in range(6)]
            torch.cuda.synchronize()
            with ctx.independent_calls():
                for o in outs:
                    ctx.quantize_ptr(xd.data_ptr(), piquant.DataType.F32, o.data_ptr(), piquant.DataType.UINT8, m, 1.0, 1, piquant.RoundMode.NEAREST)
        torch.cuda.synchronize()
        for o in outs:
            assert np.array_equal(o.cpu().numpy(), want)
    finally:
        ctx.set_blocking_wait('kernel')
        ctx.set_blocking(False)
        ctx.set_reference_layout(False, threads=1)


def test_reference_layout_from_the_environment_takes_the_contexts_own_thread_count(O):
    """PIQUANT_HIP_REFERENCE_LAYOUT=1 at context creation: an UNCHANGED binding -- piquant_context_create(num_threads) and the six calls, nothing else --
    gets byte for byte what the reference's context of the same num_threads writes (its partitions' scalar heads and tails, src/piquant.cpp:145-157)."""
    code = textwrap.dedent(f"""
        import sys, numpy as np
        sys.path.insert(0, {str(os.path.join(os.path.dirname(__file__), '..', 'pi-quant_amd'))!r}); sys.path.insert(0, {str(os.path.join(os.path.dirname(__file__), '..'))!r})
        import torch, oracle as O
        from piquant._bootstrap import C_LIB as C
        rng = np.random.default_rng(31)
        n = 1_000_003
        x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
        x[rng.choice(n, n // 3)] = np.float32(0.49999997)
        x[rng.choice(n, n // 5)] = np.float32(8388609.0)
        xd = torch.from_numpy(x).cuda()
        for threads in (1, 5, 31):
            ctx = C.piquant_context_create(threads)
            out = torch.zeros(n, dtype=torch.uint8, device='cuda')
            C.piquant_quantize(ctx, xd.data_ptr(), 0, out.data_ptr(), 4, n, 1.0, 1, 0)        # blocking, as the reference's calls are
            wbuf = np.zeros(n + 32, dtype=np.uint8); base = (-wbuf.ctypes.data) % 16
            want = O.quantize(x, O.F32, O.UINT8, 1.0, 1, form=O.FORM_REFERENCE, threads=threads, out=wbuf[base: base + n])
            assert np.array_equal(out.cpu().numpy(), want), threads
            assert not np.array_equal(want, O.quantize(x, O.F32, O.UINT8, 1.0, 1, form=O.FORM_UNIFORM))
            # host tensors, the reference's own calling convention: served by the companion library (or staged), same bytes; the head by the HOST pointer
            hbuf = np.zeros(n + 32, dtype=np.uint8); hb = (-hbuf.ctypes.data) % 16
            for off in (0, 7):
                hout = hbuf[hb + off: hb + off + n]
                C.piquant_quantize(ctx, x.ctypes.data, 0, hout.ctypes.data, 4, n, 1.0, 1, 0)
                want = O.quantize(x, O.F32, O.UINT8, 1.0, 1, form=O.FORM_REFERENCE, threads=threads, out=wbuf[base + off: base + off + n])
                assert np.array_equal(hout, want), (threads, off)
            xb = O.f32_to_bf16(x); h4 = np.zeros((n + 1) // 2, dtype=np.uint8)
            C.piquant_quantize(ctx, xb.ctypes.data, 1, h4.ctypes.data, 3, n, 0.2, 7, 0)
            assert np.array_equal(h4, O.quantize(xb, O.BF16, O.UINT4, 0.2, 7, form=O.FORM_REFERENCE, threads=threads)), threads
            acc = O.f32_to_bf16(rng.uniform(-3, 3, n).astype(np.float32)); want = O.dequantize(h4, O.UINT4, O.BF16, n, 0.3, 2, 1, form=O.FORM_REFERENCE, threads=threads, out=acc.copy())
            C.piquant_dequantize(ctx, h4.ctypes.data, 3, acc.ctypes.data, 1, n, 0.3, 2, 1)
            assert np.array_equal(acc, want), threads
            C.piquant_context_destroy(ctx)
        print('layout ok')
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PIQUANT_HIP_REFERENCE_LAYOUT="1"))
    assert r.returncode == 0 and "layout ok" in r.stdout, r.stderr[-2000:]


def test_reference_layout_partitions_across_staged_host_chunks(ctx, O):
    """A host call longer than one staging chunk (2^24 elements) in reference-layout mode for a 7- and a 100-thread reference context: every chunk is its
    own vector launch + patch launch over a WINDOW of the call, and a partition's head or tail may sit in either chunk (or straddle the cut) -- the
    patch kernels clip their ranges to the window (quantize_ref_patch_kernel, dequantize_ref_patch_kernel).  fp32 -> uint8 with a misaligned host
    output (heads), bf16 -> uint4, uint4 -> bf16 ADD."""
    import piquant

    rng = np.random.default_rng(79)
    n = (1 << 24) + (1 << 22) + 1000 + 37
    x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
    x[rng.choice(n, n // 40)] = np.float32(0.49999997)
    x[rng.choice(n, n // 50)] = np.float32(8388609.0)
    xb = O.f32_to_bf16(x)
    q4 = rng.integers(0, 256, O.packed_numel(n, O.UINT4), dtype=np.uint8)
    prev = O.f32_to_bf16(rng.uniform(-3, 3, n).astype(np.float32))
    try:
        ctx.reset_stream()
        ctx.set_blocking(True)
        ctx.set_host_path("stage")
        for threads in (7, 100):
            ctx.set_reference_layout(True, threads=threads)
            for off in (0, 3):
                buf = np.zeros(n + 32, dtype=np.uint8)
                base = (-buf.ctypes.data) % 16
                out = buf[base + off: base + off + n]
                ctx.quantize_ptr(x.ctypes.data, piquant.DataType.F32, out.ctypes.data, piquant.DataType.UINT8, n, 1.0, 0, piquant.RoundMode.NEAREST)
                wbuf = np.zeros(n + 32, dtype=np.uint8)
                wbase = (-wbuf.ctypes.data) % 16
                want = O.quantize(x, O.F32, O.UINT8, 1.0, 0, form=O.FORM_REFERENCE, threads=threads, out=wbuf[wbase + off: wbase + off + n])
                assert np.array_equal(out, want), (threads, off, np.nonzero(out != want)[0][:8])
                assert not np.array_equal(want, O.quantize(x, O.F32, O.UINT8, 1.0, 0, form=O.FORM_UNIFORM))
            out4 = np.zeros(O.packed_numel(n, O.UINT4), dtype=np.uint8)
            ctx.quantize_ptr(xb.ctypes.data, piquant.DataType.BF16, out4.ctypes.data, piquant.DataType.UINT4, n, 0.2, 7, piquant.RoundMode.NEAREST)
            assert np.array_equal(out4, O.quantize(xb, O.BF16, O.UINT4, 0.2, 7, form=O.FORM_REFERENCE, threads=threads)), threads
            acc = prev.copy()
            ctx.dequantize_ptr(q4.ctypes.data, piquant.DataType.UINT4, acc.ctypes.data, piquant.DataType.BF16, n, 0.3, 2, piquant.ReduceOp.ADD)
            assert same_floats(acc, O.dequantize(q4, O.UINT4, O.BF16, n, 0.3, 2, 1, form=O.FORM_REFERENCE, threads=threads, out=prev.copy())), threads
    finally:
        ctx.set_host_path("auto")
        ctx.set_reference_layout(False, threads=1)
        ctx.set_blocking(False)


def test_reference_layout_partitions_inside_a_hip_graph(O):
    """Reference-layout mode for a 5-thread reference context captured into a hipGraph: quantize is two kernel nodes (vector + patch), dequantize SET to bf16
    likewise, and dequantize ADD to bf16 -- whose fast flow takes stream-ordered scratch memory -- falls back to the element-by-element kernel inside a
    capture.  Replayed on new data: the oracle's threaded reference form every time."""
    import piquant
    import torch

    n, threads = 1_000_003, 5
    x = torch.zeros(n, device="cuda")
    q = torch.zeros(n, dtype=torch.uint8, device="cuda")
    q4 = torch.zeros((n + 1) // 2, dtype=torch.uint8, device="cuda")
    y = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    acc = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    c = piquant.Context()
    c.set_reference_layout(True, threads=threads)
    s = torch.cuda.Stream()
    c.set_stream(s.cuda_stream)
    c.set_blocking(False)
    F32, BF16, U8, U4 = piquant.DataType.F32, piquant.DataType.BF16, piquant.DataType.UINT8, piquant.DataType.UINT4

    def calls():
        c.quantize_ptr(x.data_ptr(), F32, q.data_ptr(), U8, n, 1.0, 1, piquant.RoundMode.NEAREST, _device_ptrs=True)
        c.dequantize_ptr(q4.data_ptr(), U4, y.data_ptr(), BF16, n, 0.3, 2, piquant.ReduceOp.SET, _device_ptrs=True)
        c.dequantize_ptr(q4.data_ptr(), U4, acc.data_ptr(), BF16, n, 0.3, 2, piquant.ReduceOp.ADD, _device_ptrs=True)

    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        calls()                                   # warm-up outside capture (also: the ADD flow's memory pool exists)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            calls()
    rng = np.random.default_rng(14)
    for _ in range(3):
        data = rng.uniform(-1.2, 1.2, n).astype(np.float32)
        data[rng.choice(n, n // 3)] = np.float32(0.49999997)
        packed = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8)
        prev = O.f32_to_bf16(rng.uniform(-3, 3, n).astype(np.float32))
        x.copy_(torch.from_numpy(data))
        q4.copy_(torch.from_numpy(packed))
        acc.copy_(torch.from_numpy(prev.view(np.int16)).view(torch.bfloat16))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        wbuf = np.zeros(n + 32, dtype=np.uint8)
        base = (-wbuf.ctypes.data) % 16
        want = O.quantize(data, O.F32, O.UINT8, 1.0, 1, form=O.FORM_REFERENCE, threads=threads, out=wbuf[base: base + n])
        assert np.array_equal(q.cpu().numpy(), want)
        assert not np.array_equal(want, O.quantize(data, O.F32, O.UINT8, 1.0, 1))
        assert same_floats(y.view(torch.int16).cpu().numpy().view(np.uint16), O.dequantize(packed, O.UINT4, O.BF16, n, 0.3, 2, 0, form=O.FORM_REFERENCE, threads=threads))
        assert same_floats(acc.view(torch.int16).cpu().numpy().view(np.uint16),
                           O.dequantize(packed, O.UINT4, O.BF16, n, 0.3, 2, 1, form=O.FORM_REFERENCE, threads=threads, out=prev.copy()))
