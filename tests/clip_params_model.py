"""CPU model of the histogram clip search for per-tensor parameters (include/piquant_hip.h, "HISTOGRAM CLIP SEARCH"): numpy and the oracle's epilogue alone.

(lo, hi) is the float32 min / max, NaNs ignored.  Counts: t = fl32(fl32(x - lo) * fl32(8192 / fl32(hi - lo))), bin = int(min(max(t, 0), 8191)), a NaN t
giving 0, NaN elements not counted.  Candidate k < steps shrinks both extremes by r_k = 1 - k / 64 in float32 and takes the ordinary epilogue; its
error is the binary64 adjacent-pair tree sum over the bins of c_j * (m_j - d_j)^2, m_j the bin centre and d_j its nearest round trip; the smallest
error wins under strict `<`.  `Rules` holds the definition's decisions one by one, so that a test can swap exactly one of them for a wrong variant
and show that a committed case notices (tests/test_clip_params_cpu.py).
"""
from dataclasses import dataclass
from typing import Callable

import numpy as np

import oracle as O

BINS = 8192
MAX_STEPS = 63
QMAX = {O.UINT2: 3, O.UINT4: 15, O.UINT8: 255}


def as_f32(x, dt_in):
    return O.bf16_to_f32(x) if dt_in == O.BF16 else np.ascontiguousarray(x, dtype=np.float32)


def tree_sum(t: np.ndarray) -> np.float64:
    """float64[8192] -> the sum by adjacent pairs (tests/clip_model.py's tree_sum, in binary64)."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        while t.size > 1:
            t = t[0::2] + t[1::2]
    return t[0]


def sequential_sum(t: np.ndarray) -> np.float64:
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in np.asarray(t, dtype=np.float64):
            s = s + v
    return s


@dataclass
class Rules:
    bin_of: Callable = np.trunc                      # t (clamped to [0, 8191]) -> bin; WRONG: np.rint
    clamp_top: bool = True                           # WRONG: t == 8192 (x == hi) lands in a bin 8192 that is dropped
    count_nans: bool = False                         # WRONG: NaN elements counted (their NaN t gives bin 0)
    centre_dtype: type = np.float64                  # WRONG: np.float32 centres
    round_half: float = 0.5                          # WRONG: 0.0, floor(t) for floor(t + 0.5)
    reduce: Callable = tree_sum                      # WRONG: sequential_sum
    less: Callable = np.less                         # WRONG: np.less_equal
    zero_empty: bool = True                          # WRONG: an empty bin adds 0 * e^2 (NaN where e is not finite)
    zp_in_d: bool = True                             # WRONG: d = u * s


DEFINITION = Rules()


FLT_MAX = np.float32(3.402823466e+38)


def minmax(x, dt_in):
    """float32 (lo, hi) as the scan folds them: from the identities (+FLT_MAX, -FLT_MAX), NaNs ignored -- nothing scanned leaves max < min."""
    xf = as_f32(x, dt_in)
    xf = xf[~np.isnan(xf)]
    if xf.size == 0:
        return FLT_MAX, -FLT_MAX
    return np.float32(min(xf.min(), FLT_MAX)), np.float32(max(xf.max(), -FLT_MAX))


def histogram(x, dt_in, lo, hi, rules: Rules = DEFINITION) -> np.ndarray:
    """uint64[8192] counts of x against (lo, hi); all zero when not hi > lo."""
    c = np.zeros(BINS, dtype=np.uint64)
    lo, hi = np.float32(lo), np.float32(hi)
    if not hi > lo:
        return c
    xf = as_f32(x, dt_in)
    if not rules.count_nans:
        xf = xf[~np.isnan(xf)]
    with np.errstate(all="ignore"):
        wf = np.float32(hi - lo)
        inv = np.float32(np.float32(BINS) / wf)
        t = ((xf - lo).astype(np.float32) * inv).astype(np.float32)
    t = np.where(np.isnan(t), np.float32(0.0), t)
    t = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(BINS - 1 if rules.clamp_top else BINS))
    b = rules.bin_of(t).astype(np.int64)
    b = b[b < BINS]
    return np.bincount(b, minlength=BINS).astype(np.uint64)


def epilogue(lo, hi, qd):
    """the ordinary epilogue as the device runs it: a range with not hi > lo (constant, or nothing scanned: max < min) gets (1.0, qmax >> 1)"""
    if not np.float32(hi) > np.float32(lo):
        return 1.0, QMAX[qd] >> 1
    return O.quant_params_from_minmax(float(lo), float(hi), qd)


def candidate(lo, hi, k, qd):
    """-> (evaluated, scale, zero point) of candidate k"""
    r = np.float32(1.0) - np.float32(k) / np.float32(64.0)
    with np.errstate(all="ignore"):
        lo_k, hi_k = np.float32(np.float32(lo) * r), np.float32(np.float32(hi) * r)
    s, z = epilogue(lo_k, hi_k, qd)
    return bool(k == 0 or hi_k > lo_k), np.float32(s), int(z)


def candidate_error(c, lo, hi, s, z, qd, rules: Rules = DEFINITION) -> np.float64:
    with np.errstate(all="ignore"):
        j = np.arange(BINS, dtype=np.float64) + 0.5
        if rules.centre_dtype is np.float32:
            W = np.float32((np.float32(hi) - np.float32(lo)) / np.float32(BINS))
            m = (np.float32(lo) + (j.astype(np.float32) * W).astype(np.float32)).astype(np.float32).astype(np.float64)
        else:
            W = (np.float64(hi) - np.float64(lo)) / np.float64(BINS)
            m = np.float64(lo) + j * W
        sd, zd = np.float64(s), np.float64(z)
        u = np.floor(m / sd + rules.round_half) + zd
        u = np.where(np.isnan(u), 0.0, np.minimum(np.maximum(u, 0.0), np.float64(QMAX[qd])))
        d = ((u - zd) if rules.zp_in_d else u) * sd
        e = m - d
        term = c.astype(np.float64) * (e * e)
        if rules.zero_empty:
            term = np.where(c == 0, np.float64(0.0), term)
        return np.float64(rules.reduce(term))


def search(lo, hi, c, qd, steps, rules: Rules = DEFINITION):
    """-> (scale float32, zero point, choice, errors float64[63] with NaN where a candidate was not evaluated) from a range and its counts;
    nothing scanned: the identities, max < min."""
    assert isinstance(steps, int) and 1 <= steps <= MAX_STEPS
    errors = np.full(MAX_STEPS, np.nan, dtype=np.float64)
    s0, z0 = epilogue(lo, hi, qd)
    best = (np.float32(s0), int(z0), 0)
    if steps == 1 or not np.float32(hi) > np.float32(lo):
        return best + (errors,)
    e_best = None
    for k in range(steps):
        ok, s, z = candidate(lo, hi, k, qd)
        if not ok:
            continue
        E = candidate_error(c, lo, hi, s, z, qd, rules)
        if np.isnan(E):
            E = np.float64(np.nan)   # one NaN pattern (0x7ff8000000000000), whatever produced it
        errors[k] = E
        with np.errstate(invalid="ignore"):
            if k == 0:
                e_best = E
            elif rules.less(E, e_best):
                e_best, best = E, (s, z, k)
    return best + (errors,)


def compute_quant_params_clipped(x, dt_in, qd, steps=63, rules: Rules = DEFINITION):
    """-> (scale, zero point, choice, errors, counts): the one-call form"""
    lo, hi = minmax(x, dt_in)
    c = histogram(x, dt_in, lo, hi, rules)
    return search(lo, hi, c, qd, steps, rules) + (c,)


def record_bytes(scale, zp) -> bytes:
    """the 16 bytes of piquant_hip_params_t {scale, fl32(1 / scale), zero point}"""
    import struct

    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.float32(scale)
    return struct.pack("<ffq", float(np.float32(scale)), float(inv), int(zp))


def assert_tie(lo, hi, c, qd, steps, ks):
    """The candidates `ks` tie exactly at the minimum of the errors (so the case cannot silently stop being a tie)."""
    E = search(lo, hi, c, qd, steps)[3]
    assert all(E[k] == E[ks[0]] for k in ks) and E[ks[0]] == np.nanmin(E), f"no tie of candidates {ks} at the minimum any more: E = {E[:steps]}"


def round_trip_mse(x, dt_in, qd, scale, zp) -> float:
    """true round-trip MSE: the oracle's nearest quantize and float32 dequantize, NaN elements left out (float64 accumulation: a report)"""
    xf = as_f32(x, dt_in)
    q = O.quantize(x, dt_in, qd, float(scale), int(zp))
    d = O.dequantize(q, qd, O.F32, x.size, float(scale), int(zp)).astype(np.float64)
    keep = ~np.isnan(xf)
    return float(np.mean((xf.astype(np.float64)[keep] - d[keep]) ** 2))


# ---- committed cases: (name, float32 values) -- tests/test_clip_params_cpu.py and tests/test_gpu_clip_params.py run all of them ----------------
DENORMAL = np.float32(1.401298464324817e-45)   # 2^-149
TIE_KS = (0, 1, 10)   # candidates of edge case "tie" with hi_k = fl32(3 * 2^-149 * r_k) = 3 * 2^-149: the same (scale, zero point), the same error


def edge_tensors():
    rng = np.random.default_rng(7)
    g = rng.standard_normal(3000).astype(np.float32)
    with_nans = g.copy()
    with_nans[::7] = np.nan
    infs = g.copy()
    infs[5], infs[77] = np.inf, -np.inf
    wide = g.copy()
    wide[0], wide[1] = np.float32(-3e38), np.float32(3e38)
    edges = np.concatenate([np.arange(0, 8193, dtype=np.float32), np.arange(0, 8193, 64, dtype=np.float32)])
    one_bin = np.full(2000, 0.5, dtype=np.float32)
    one_bin[0], one_bin[-1] = -1.0, 3.0
    zeros = np.array([0.0, -0.0] * 50 + [1.0, -1.0, 0.25], dtype=np.float32)
    return [
        ("constant", np.full(777, 1.5, dtype=np.float32)),
        ("all_nan", np.full(300, np.nan, dtype=np.float32)),
        ("nans_among_values", with_nans),
        ("infs_present", infs),
        ("range_overflows", wide),
        ("denormal_range", np.array([0.0] * 40 + [float(DENORMAL)] * 3 + [float(DENORMAL * 2)] * 5 + [float(DENORMAL * 5)] * 9, dtype=np.float32)),
        ("bin_edges_and_top", edges),
        ("one_bin", one_bin),
        ("signed_zeros", zeros),
        ("plus_inf_only", np.array([1.0, 2.5, np.inf, 3.0, np.inf, -0.5] * 20, dtype=np.float32)),      # lo finite, hi = +inf
        ("minus_inf_only", np.array([1.0, -np.inf, 2.5, 3.0, -0.5] * 20, dtype=np.float32)),            # lo = -inf, hi finite
        ("tie", np.array([0.0] * 11 + [float(DENORMAL * 3)] * 6, dtype=np.float32)),
    ]


def as_input(v: np.ndarray, dt_in):
    """float32 values -> the input array of type dt_in (bfloat16: rounded, so the case is what the widened tensor holds)"""
    return O.f32_to_bf16(v) if dt_in == O.BF16 else np.ascontiguousarray(v, dtype=np.float32)


def mse_ratio_table(n=1 << 20, steps=63, seed=0):
    """Round-trip MSE with the search over MSE with min/max, and the estimate's E / n over the true MSE: the table of DESIGN.md (python tests/clip_params_model.py)."""
    rng = np.random.default_rng(seed)
    spiked = rng.standard_normal(n).astype(np.float32)
    spiked[::65536] = 50.0
    data = {"N(0,1)": rng.standard_normal(n).astype(np.float32), "Laplace": rng.laplace(size=n).astype(np.float32), "N(0,1) + 50 sigma every 65 536": spiked}
    rows = []
    for name, x in data.items():
        for qd, wire in ((O.UINT8, "uint8"), (O.UINT4, "uint4"), (O.UINT2, "uint2")):
            s, z, k, E, _ = compute_quant_params_clipped(x, O.F32, qd, steps)
            s0, z0 = O.compute_quant_params(x, O.F32, qd)
            with_search = round_trip_mse(x, O.F32, qd, s, z)
            rows.append((name, wire, k, with_search / round_trip_mse(x, O.F32, qd, s0, z0), E[k] / n / with_search))
    return rows


if __name__ == "__main__":
    O.build(with_ref=None)
    print("| data | wire | chosen k | MSE searched / MSE min-max | estimate / true |\n|---|---|---|---|---|")
    for name, wire, k, ratio, est in mse_ratio_table():
        print(f"| {name} | {wire} | {k} | {ratio:.3f} | {est:.3f} |")
