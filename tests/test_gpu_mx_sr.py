"""piquant_hip_quantize_mx_sr / _sr_batch on the device against tests/mx_sr_model.py, bit for bit, with guard bytes around every buffer (the buffers
of test_gpu_mx.py).  Every element's input is built from its OWN threshold t: the float whose floor(f * 2^24) is the smallest achievable value
>= 2^24 - t (it goes up), or the next achievable one below (it stays) -- a wrong index, a wrong alignment of the hash word or a word shared between
elements flips codes.  The only slack is the definition's: the two NaN bytes of E4M3 compare as one."""
import numpy as np
import pytest

import mx_sr_model as S
from test_gpu_mx import Buf, as_input, canon_codes, ctx  # noqa: F401  (ctx: the fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLOATS = ["float32", "bfloat16"]
NUMELS = [1, 31, 33, 1025, 2047, 2049, 6181]       # a wave's tile is 2048 elements (1024: float32 -> FP8); 6181: three tiles and a ragged end
SEED, BASE = 0x9E3779B97F4A7C15, 2 ** 32 - 1000     # the hash key switches at element 1000, inside the first tile
MBITS = {S.FP4: 1, S.FP8: 3, S.E2M3: 3, S.E3M2: 2}
EMIN = {S.FP4: 0, S.FP8: -6, S.E2M3: 0, S.E3M2: -2}


def near_threshold_inputs(n, fmt, dt, base=BASE):
    """float32 values (bfloat16-representable for dt bfloat16) of n elements at the global indices base + i.  Blocks cycle through maxima in the
    format's denormal range (float32 denormals, s = 0), below emax, at emax, on / just above / far above the top mantissa at middle and large
    exponents, then one block each with -0, NaN, +inf and -inf in it; the other elements sit in binades from the block's down into the format's
    denormal range, their discarded bits placed at the element's threshold as the module docstring says."""
    rng = np.random.default_rng(n * 8 + len(fmt))
    P, mb, emin, emax, topm = (23 if dt == "float32" else 7), MBITS[fmt], EMIN[fmt], S.EMAX[fmt], S.TOP_MANT[fmt]
    gran = 1 << (23 - P)
    nb = -(-n // S.BLOCK)
    need = np.resize(2 ** 24 - S.thresholds(SEED, base, n), nb * S.BLOCK).reshape(nb, S.BLOCK)
    down = rng.integers(0, 2, (nb, S.BLOCK))                        # 0: the smallest value that goes up; 1: the next one below
    kinds = [(0, 0), (emax - 1, 0x7FFFFF & -gran), (emax, 0), (emax + 5, topm), (emax + 5, topm + gran), (127, 0x7FFFFF & -gran), (200, topm + gran),
             (254, topm), (254, 0x7FFFFF & -gran)]
    bits = np.zeros((nb, S.BLOCK), np.int64)
    for b in range(nb):
        E, M = kinds[b % len(kinds)]
        if E == 0:                                                      # v = Mx * 2^-22: Mx = kept << r | discarded, kept < 2^mb keeps v below 2^emin
            r = 22 + emin - mb
            disc = np.clip(((need[b] + (1 << (24 - r)) - 1) >> (24 - r)) - down[b], 0, (1 << r) - 1)
            mx = ((rng.integers(0, 1 << mb, S.BLOCK) << r | disc) + gran - 1) & -gran
            bits[b] = np.where(mx < 1 << (r + mb), mx, 0)
            continue
        s = max(E - emax, 0) + (E >= emax and M > topm)
        low = max(emin - mb - 1, 1 - s)                                 # scaled binades below the maximum's (its own where there is none: the
        k = rng.integers(low, max(E - s, low + 1), S.BLOCK)             # maximum's mantissa is then all ones), down to half the smallest step
        r = P - mb + np.maximum(emin - k, 0)                            # discarded bits of the significand (the implicit one included past P)
        disc = np.clip(((need[b] + (1 << (24 - r)) - 1) >> (24 - r)) - down[b], np.where(r > P, 1 << P, 0), np.minimum(1 << r, 2 << P) - 1)
        kept = (1 << np.maximum(P - r, 0)) + rng.integers(0, 1 << 30, S.BLOCK) % (1 << np.maximum(P - r, 0))
        sig = np.where(r > P, disc, kept << np.minimum(r, P) | disc)
        bits[b] = (k + s) << 23 | (sig - (1 << P)) << (23 - P)
        bits[b, rng.integers(0, S.BLOCK)] = E << 23 | M                 # the block's maximum
    bits |= rng.integers(0, 2, bits.shape) << 31
    x = bits.astype(np.uint32).view(np.float32)
    for b, special in zip(range(len(kinds), nb, len(kinds) + 1), np.array([-0.0, np.nan, np.inf, -np.inf], np.float32)):
        x[b, 5] = special
    return x.ravel()[:n].copy()


def device_quantize_sr(ctx, held, dt, fmt, base, off=(0, 0, 0)):
    import piquant
    import piquant.torch as T

    n, esize = held.size, held.itemsize
    nc, ns = T.mx_nbytes(n, fmt)
    x, codes, scales = Buf(n * esize, off[0] * esize, held), Buf(nc, off[1]), Buf(ns, off[2])
    ctx.set_stream(0)
    ctx.quantize_mx_sr_ptr(x.view.data_ptr(), piquant.DataType.F32 if dt == "float32" else piquant.DataType.BF16, codes.view.data_ptr(),
                           scales.view.data_ptr(), n, T.MX_FORMATS[fmt], SEED, base, _device_ptrs=True)
    torch.cuda.synchronize()
    x.bytes()
    return codes.bytes(), scales.bytes()


def canon(raw, fmt):
    return canon_codes(raw, fmt) if fmt == S.FP8 else raw


def check(ctx, wide, held, dt, fmt, base, off):
    raw, scales = device_quantize_sr(ctx, held, dt, fmt, base, off)
    want, want_scales = S.quantize(wide, fmt, SEED, base)
    assert np.array_equal(scales, want_scales)
    bad = np.flatnonzero(canon(raw, fmt) != canon(S.pack(want, fmt), fmt))
    assert bad.size == 0, (bad[:8], raw[bad[:8]], S.pack(want, fmt)[bad[:8]])
    return raw, scales


@pytest.mark.parametrize("n", NUMELS)
@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_against_the_model_aligned_and_one_element_off(ctx, fmt, dt, n):
    held, wide = as_input(near_threshold_inputs(n, fmt, dt), dt)
    streamed = check(ctx, wide, held, dt, fmt, BASE, (0, 0, 0))
    guarded = check(ctx, wide, held, dt, fmt, BASE, (1, 1, 1))          # the guarded kernels: the same bytes
    assert all(np.array_equal(a, b) for a, b in zip(streamed, guarded))


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_two_halves_with_their_offsets_are_the_whole_call(ctx, fmt, dt):
    n, cut = 6181, 97 * S.BLOCK
    held, wide = as_input(near_threshold_inputs(n, fmt, dt), dt)
    whole = check(ctx, wide, held, dt, fmt, BASE, (0, 0, 0))
    first, second = device_quantize_sr(ctx, held[:cut], dt, fmt, BASE), device_quantize_sr(ctx, held[cut:], dt, fmt, BASE + cut)
    assert all(np.array_equal(np.concatenate([a, b]), w) for a, b, w in zip(first, second, whole))


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("fmt", [S.FP4, S.FP8])
def test_batch_members_are_the_single_calls(ctx, fmt, dt):
    import piquant.torch as T

    tdt = torch.float32 if dt == "float32" else torch.bfloat16
    sizes, bases = [4096 + 2049, 0, 2047], [BASE, 7, 2 ** 63 + 5]
    wides = [as_input(near_threshold_inputs(n, fmt, dt, b), dt)[1] for n, b in zip(sizes, bases)]
    outs = T.quantize_mx_batch([torch.from_numpy(w).cuda().to(tdt) for w in wides], format=fmt, round_mode="stochastic", seed=SEED, index_bases=bases)
    for w, b, (codes, scales) in zip(wides, bases, outs):
        want, want_scales = S.quantize(w, fmt, SEED, b)
        assert np.array_equal(scales.cpu().numpy(), want_scales)
        assert np.array_equal(canon(codes.cpu().numpy(), fmt), canon(S.pack(want, fmt), fmt))


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_graph_replays_give_the_eager_bytes(ctx, fmt):
    import piquant.torch as T

    n = 6181
    inputs = [torch.from_numpy(near_threshold_inputs(n, fmt, "float32", b)).cuda() for b in (BASE, BASE + 1)]
    x = inputs[0].clone()
    kw = dict(format=fmt, round_mode="stochastic", seed=SEED, index_base=BASE)
    T.quantize_mx(x, **kw)                                             # eager warm-up (context, code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gc, gs = T.quantize_mx(x, **kw)
    for fresh in (inputs[1], inputs[0], inputs[1]):
        x.copy_(fresh)
        gc.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        want_c, want_s = T.quantize_mx(fresh, **kw)
        assert torch.equal(gc, want_c) and torch.equal(gs, want_s)
