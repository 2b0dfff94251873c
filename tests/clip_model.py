"""CPU model of the per-group clip search (piquant_hip_quantize_grouped_clipped), made of tests/grouped_model.py and the oracle alone.

For every FULL group with hi > lo (float32 min / max, NaNs ignored), candidate k < steps shrinks both extremes towards zero, lo_k = fl32(lo r_k),
hi_k = fl32(hi r_k) with r_k = 1 - k / 16, and takes the ordinary epilogue on them; its error E_k is the float32 sum, by the adjacent-pair tree,
of fl32(fl32(xf - d)^2) over the group, d the float32 dequantize of the NEAREST quantize with (scale_k, zp_k), +0 for a NaN element; the smallest
E_k wins under strict float32 `<` (ties and NaNs keep the smaller k).  The output is quantize_grouped with the chosen parameters given, in the
call's rounding mode.  Everything is float32 numpy arithmetic; the tree is formed by repeated s[0::2] + s[1::2].

`Rules` holds the definition's decisions one by one, so that a test can swap exactly one of them for a wrong variant and show that a committed
case notices (tests/test_grouped_clip_cpu.py).
"""
from dataclasses import dataclass
from typing import Callable

import numpy as np

import grouped_model as GM
import oracle as O

MAX_STEPS = 12


def tree_sum(s: np.ndarray, e: np.ndarray = None) -> np.ndarray:
    """float32[ng, G] -> float32[ng]: adjacent pairs until one value per row is left."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def shrink_towards_zero(lo: np.float32, hi: np.float32, r: np.float32):
    return np.float32(lo * r), np.float32(hi * r)


@dataclass
class Rules:
    reduce: Callable = tree_sum                      # (s, e) -> E
    less: Callable = np.less                         # E_k (less) E_best
    zero_nan: bool = True                            # an element whose xf is NaN adds +0
    dequant_in_input_type: bool = False              # WRONG: d rounded to bfloat16 for a bfloat16 x
    search_ragged: bool = False                      # WRONG: the ragged last group searched too
    shrink: Callable = shrink_towards_zero           # (lo, hi, r_k) -> (lo_k, hi_k)
    eval_with_call_mode: bool = False                # WRONG: candidates judged in the call's rounding mode


DEFINITION = Rules()


def search(x, dt_in, qd, G, steps, rules: Rules = DEFINITION, round_mode=O.NEAREST, threshold=0.0):
    """-> (scales float32[ng], zero points uint8[ng], choices uint8[ng], E float32[steps, ng] with NaN where a candidate was not evaluated)."""
    assert isinstance(steps, int) and 1 <= steps <= MAX_STEPS
    xf = GM.as_f32(x, dt_in)
    n = x.size
    ng = (n + G - 1) // G
    lo, hi = GM.group_minmax(xf, G)
    s0, z0 = GM.group_params_all(xf, G, qd)                       # candidate 0: quantize_grouped's parameters
    scales, zps = s0.copy(), z0.copy()
    choices = np.zeros(ng, dtype=np.uint8)
    errors = np.full((steps, ng), np.nan, dtype=np.float32)
    if steps == 1:
        return scales, zps, choices, errors
    nsearch = ng if rules.search_ragged else n // G               # groups that can be searched at all
    searched = np.zeros(ng, dtype=bool)
    searched[:nsearch] = hi[:nsearch] > lo[:nsearch]
    best_e = np.zeros(ng, dtype=np.float32)
    mode, thr = (round_mode, threshold) if rules.eval_with_call_mode else (O.NEAREST, 0.0)
    pad = np.full(ng * G, np.nan, dtype=np.float32)               # a searched ragged group (a wrong variant) is padded with NaNs: +0 each
    pad[:n] = xf
    for k in range(steps):
        r = np.float32(1.0) - np.float32(k) / np.float32(16.0)
        sk, zk = s0.copy(), z0.copy()
        ok = np.zeros(ng, dtype=bool)
        for g in np.flatnonzero(searched):
            with np.errstate(all='ignore'):
                lo_k, hi_k = rules.shrink(lo[g], hi[g], r)
            if k == 0:
                ok[g] = True                                      # exactly quantize_grouped's pair, already in sk / zk
            elif hi_k > lo_k:
                ok[g] = True
                sk[g], zk[g] = O.quant_params_from_minmax(float(lo_k), float(hi_k), qd)
        q, _, _ = GM.quantize_grouped(x, dt_in, qd, G, mode, thr, params=(sk, zk))
        if rules.dequant_in_input_type and dt_in == O.BF16:
            d = O.bf16_to_f32(GM.dequantize_grouped(q, qd, O.BF16, n, G, sk, zk))
        else:
            d = GM.dequantize_grouped(q, qd, O.F32, n, G, sk, zk)
        dp = np.zeros(ng * G, dtype=np.float32)
        dp[:n] = d
        with np.errstate(all='ignore'):
            e = (pad - dp).astype(np.float32)
            s = (e * e).astype(np.float32)
        if rules.zero_nan:
            s[np.isnan(pad)] = np.float32(0.0)
            e = np.where(np.isnan(pad), np.float32(0.0), e)
        with np.errstate(all='ignore'):
            E = np.asarray(rules.reduce(s.reshape(ng, G), e.reshape(ng, G)), dtype=np.float32)
        errors[k, ok] = E[ok]
        with np.errstate(invalid='ignore'):
            wins = ok & (np.full(ng, k == 0) | rules.less(E, best_e))
        best_e[wins] = E[wins]
        choices[wins] = k
        scales[wins] = sk[wins]
        zps[wins] = zk[wins]
    return scales, zps, choices, errors


def quantize_grouped_clipped(x, dt_in, qd, G, steps=9, round_mode=O.NEAREST, threshold=0.0, rules: Rules = DEFINITION):
    """-> (packed bytes, scales, zero points, choices): quantize_grouped with the chosen parameters given, in the call's rounding mode."""
    scales, zps, choices, _ = search(x, dt_in, qd, G, steps, rules, round_mode, threshold)
    q, _, _ = GM.quantize_grouped(x, dt_in, qd, G, round_mode, threshold, params=(scales, zps))
    return q, scales, zps, choices


def assert_tie(x, dt_in, qd, G, steps, group, ks):
    """The candidates `ks` of `group` tie exactly at the minimum of the group's errors (so the case cannot silently stop being a tie)."""
    E = search(x, dt_in, qd, G, steps)[3][:, group]
    assert all(E[k] == E[ks[0]] for k in ks) and E[ks[0]] == np.nanmin(E), f"no tie of candidates {ks} at the minimum any more: E = {E}"


def assert_crosses_short_step_line(x, dt_in, qd, G, steps, group):
    """The short step's bound, fl32(max(|lo|, |hi|) * fl32(1 / scale_k)) < 10^9 on the group's unclipped extremes, holds for candidate 0 and fails
    for a later candidate of `group` (so the case cannot silently stop crossing)."""
    xf = GM.as_f32(x, dt_in)[group * G:(group + 1) * G]
    lo, hi = np.fmin.reduce(xf), np.fmax.reduce(xf)
    ratios = []
    for k in range(steps):
        r = np.float32(1.0) - np.float32(k) / np.float32(16.0)
        scale, _ = O.quant_params_from_minmax(float(np.float32(lo * r)), float(np.float32(hi * r)), qd)
        ratios.append(np.float32(max(abs(lo), abs(hi))) * (np.float32(1.0) / np.float32(scale)))
    assert ratios[0] < np.float32(1.0e9) and max(ratios[1:]) >= np.float32(1.0e9), f"the candidates do not cross the line any more: {ratios}"


def round_trip_mse(x, dt_in, qd, G, q, scales, zps) -> float:
    """Mean squared error of dequantize_grouped(q) in float32 against the widened x, NaN elements left out (float64 accumulation: a report)."""
    xf = GM.as_f32(x, dt_in).astype(np.float64)
    d = GM.dequantize_grouped(q, qd, O.F32, x.size, G, scales, zps).astype(np.float64)
    keep = ~np.isnan(xf)
    return float(np.mean((xf[keep] - d[keep]) ** 2))


def mse_ratio_table(n=1 << 16, steps=9, seed=0):
    """Round-trip MSE with the search over MSE without it, in the project's arithmetic: the table of DESIGN.md, "Per-group clip search" (python tests/clip_model.py)."""
    rng = np.random.default_rng(seed)
    data = {"N(0,1)": rng.standard_normal(n).astype(np.float32), "Laplace": rng.laplace(size=n).astype(np.float32)}
    rows = []
    for name, x in data.items():
        for qd, wire in ((O.UINT2, "uint2"), (O.UINT4, "uint4"), (O.UINT8, "uint8")):
            ratios = []
            for G in (32, 128, 1024):
                q0, s0, z0 = GM.quantize_grouped(x, O.F32, qd, G)
                q1, s1, z1, _ = quantize_grouped_clipped(x, O.F32, qd, G, steps)
                ratios.append(round_trip_mse(x, O.F32, qd, G, q1, s1, z1) / round_trip_mse(x, O.F32, qd, G, q0, s0, z0))
            rows.append((name, wire, ratios))
    return rows


if __name__ == "__main__":
    O.build(with_ref=None)
    print("| data | wire | G = 32 | G = 128 | G = 1024 |\n|---|---|---|---|---|")
    for name, wire, ratios in mse_ratio_table():
        print(f"| {name} | {wire} | " + " | ".join(f"{r:.2f}" for r in ratios) + " |")
