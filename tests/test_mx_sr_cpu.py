"""The stochastic MX definition (tests/mx_sr_model.py) on blocks worked out by hand, its unbiasedness, and the argument rules of
piquant.torch.quantize_mx(round_mode=...) / quantize_mx_batch -- no GPU."""
import numpy as np
import pytest

import mx_sr_model as S

torch = pytest.importorskip("torch")

SEED = 12345
HALF = {S.FP4: (1.25, 2), S.FP8: (1.0625, 56), S.E2M3: (1.0625, 8), S.E3M2: (1.125, 12)}   # midway between code k and k + 1: (value, k)


def block(first, rest=0.0):
    b = np.full(S.BLOCK, rest, np.float32)
    b[0] = first
    return b


def bits(field, mantissa):
    return np.array([field << 23 | mantissa], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_headroom_bump_on_and_just_off_the_top_mantissa(fmt):
    emax, topm, mags = S.EMAX[fmt], S.TOP_MANT[fmt], S.magnitudes(fmt)
    cases = [(127 + emax, topm, 127), (127 + emax, topm + 1, 128), (130 + emax, topm, 130), (130 + emax, topm + 1, 131), (254, topm, 254 - emax),
             (254, topm + 1, 255 - emax), (emax, topm, 0), (emax, topm + 1, 1), (emax - 1, 0x7FFFFF, 0), (0, 0x7FFFFF, 0), (255, 0, 255 - emax)]
    for field, mantissa, s in cases:
        assert S.scale_bytes(block(bits(field, mantissa)), fmt)[0] == s, (field, hex(mantissa))
    # just above the top the element lands between top / 2 and the next code up under the bumped scale: it never clips
    half = int(np.flatnonzero(mags == mags[-1] / 2)[0])
    for base in range(8):
        codes, scales = S.quantize(block(bits(127 + emax, topm + 1)), fmt, SEED, base)
        assert scales[0] == 128 and codes[0] in (half, half + 1)


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_half_way_goes_both_ways_and_representable_values_stay(fmt):
    v, k = HALF[fmt]
    t = S.thresholds(SEED, 0, 64)
    up, stay = int(np.flatnonzero(t >= 2 ** 23)[0]), int(np.flatnonzero(t < 2 ** 23)[0])
    b = block(2.0 ** S.EMAX[fmt], -v)                                    # amax 2^emax: s = 127, the scaled domain is the input's
    for g, want in ((up, k + 1), (stay, k)):
        codes, scales = S.quantize(b, fmt, SEED, g - 1)                  # element 1 sits at global index g
        assert scales[0] == 127 and codes[1] == want | S.SIGN[fmt]
    mags = S.magnitudes(fmt)
    pick = np.linspace(0, mags.size - 1, S.BLOCK).astype(int)            # 32 codes from 0 to the top: none moves under any index
    for base in (0, 77, 2 ** 40):
        codes, scales = S.quantize((mags[pick] * np.where(pick % 2, -1, 1)).astype(np.float32), fmt, SEED, base)
        assert scales[0] == 127 and np.array_equal(codes, pick | np.where(pick % 2, S.SIGN[fmt], 0))


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_zeros_nan_and_infinity_encode_as_in_the_nearest_call(fmt):
    b = block(4.0)
    b[1:5] = [-0.0, np.nan, 0.0, -1e-30]                                 # -1e-30 is far below half a step: never up
    codes, scales = S.quantize(b, fmt, SEED)
    assert scales[0] == 127 + 2 - S.EMAX[fmt] and list(codes[1:5]) == [S.SIGN[fmt], S.NAN_CODE[fmt], 0, S.SIGN[fmt]]
    b[0], b[5] = np.inf, -np.inf
    codes, scales = S.quantize(b, fmt, SEED)
    top = S.magnitudes(fmt).size - 1
    assert scales[0] == 255 - S.EMAX[fmt] and codes[0] == top and codes[5] == top | S.SIGN[fmt] and codes[2] == S.NAN_CODE[fmt]
    codes, scales = S.quantize(np.full(S.BLOCK, np.nan, np.float32), fmt, SEED)
    assert scales[0] == 0 and (codes == S.NAN_CODE[fmt]).all()


@pytest.mark.parametrize("v", [0.3, 1.3, 2.9])
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_the_mean_over_4096_indices_is_unbiased(fmt, v):
    """One fixed v next to a block maximum of 4 (s = 127 + 2 - emax) at 4096 consecutive global indices: the mean dequantized value is v within 4
    standard errors of the Bernoulli mean between its two neighbours lo and hi."""
    v = np.float32(v)
    b = np.tile(block(4.0, v), 4096 // (S.BLOCK - 1) + 1)
    codes, scales = S.quantize(b, fmt, SEED, 10 ** 12)
    d = S.dequantize(codes, scales, fmt).astype(np.float64).reshape(-1, S.BLOCK)[:, 1:].ravel()[:4096]
    lo, hi = d.min(), d.max()
    assert lo <= v <= hi and set(np.unique(d)) <= {lo, hi}
    p = 0.0 if hi == lo else (float(v) - lo) / (hi - lo)
    assert abs(d.mean() - float(v)) <= 4 * (hi - lo) * np.sqrt(p * (1 - p) / 4096)


def test_argument_rules():
    import piquant.torch as T

    x = torch.zeros(64)
    with pytest.raises(ValueError, match="seed= belongs to round_mode='stochastic'"):
        T.quantize_mx(x, seed=1)
    with pytest.raises(ValueError, match="needs seed="):
        T.quantize_mx(x, round_mode="stochastic")
    with pytest.raises(ValueError, match="round_mode must be"):
        T.quantize_mx(x, round_mode="up")
    with pytest.raises(ValueError, match="index_base must be an int"):
        T.quantize_mx(x, round_mode="stochastic", seed=1, index_base=-1)
    with pytest.raises(ValueError, match="seed= belongs to round_mode='stochastic'"):
        T.quantize_mx_batch([x], seed=1)
    with pytest.raises(ValueError, match="one int per tensor"):
        T.quantize_mx_batch([x, x], round_mode="stochastic", seed=1, index_bases=[0])
    with pytest.raises(ValueError, match=r"index_bases\[1\] must be an int"):
        T.quantize_mx_batch([x, x], round_mode="stochastic", seed=1, index_bases=[0, -5])
    with pytest.raises(ValueError, match="FP6 is served by"):
        T.quantize_mx_batch([x], format="fp6_e2m3", round_mode="stochastic", seed=1)
    with pytest.raises(ValueError, match="ROCm device tensor"):       # the rounding arguments are in order: only the device is missing
        T.quantize_mx(x, round_mode="stochastic", seed=-1, index_base=2 ** 64 - 1)
