"""The per-group clip search on the CPU: properties of the model (tests/clip_model.py) on the committed cases (tests/clip_cases.py), and the proof
that the cases can tell the definition from ten plausible wrong implementations -- each changes the bytes, the parameters or the choices of at
least one case, so a kernel that has one of these faults fails the bit-for-bit GPU tests (tests/test_gpu_grouped_clip.py)."""
import functools

import numpy as np
import pytest

import clip_cases as CC
import clip_model as M
import grouped_model as GM
import oracle as O

CASES = CC.variant_cases()
CASE_IDS = [c[0] for c in CASES]
STOCH = (O.STOCHASTIC, 0.3)   # the rounding mode of a stochastic call with its threshold pinned


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


@functools.lru_cache(maxsize=None)
def definition(i, mode=O.NEAREST, thr=0.0):
    name, dt_in, qd, G, steps, v = CASES[i]
    x = CC.as_input(v, dt_in)
    q, s, z, c = M.quantize_grouped_clipped(x, dt_in, qd, G, steps, mode, thr)
    return x, q, s, z, c


def same(a, b):
    return all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8)) for u, w in zip(a, b))


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_one_step_is_quantize_grouped(i):
    name, dt_in, qd, G, steps, v = CASES[i]
    x = CC.as_input(v, dt_in)
    q, s, z, c = M.quantize_grouped_clipped(x, dt_in, qd, G, 1)
    assert same((q, s, z), GM.quantize_grouped(x, dt_in, qd, G)) and not c.any()


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_best_error_is_at_most_the_unclipped_and_the_output_is_quantize_grouped_with_the_choice(i):
    name, dt_in, qd, G, steps, v = CASES[i]
    x, q, s, z, c = definition(i)
    _, _, c2, E = M.search(x, dt_in, qd, G, steps)
    assert np.array_equal(c, c2)
    for g in range(c.size):
        if c[g]:
            assert E[c[g], g] < E[0, g]                               # a later candidate wins only by being strictly better
            assert not np.any(E[: c[g], g] <= E[c[g], g])             # ... than every candidate before it (NaN compares false)
    s0, z0 = GM.group_params_all(GM.as_f32(x, dt_in), G, qd)
    keep = c == 0
    assert same((s[keep], z[keep]), (s0[keep], z0[keep]))             # candidate 0 is exactly quantize_grouped's pair
    for mode, thr in ((O.NEAREST, 0.0), STOCH):
        _, qm, sm, zm, cm = definition(i, mode, thr)
        assert same((sm, zm, cm), (s, z, c))                          # the search does not depend on the call's mode
        assert same((qm,), (GM.quantize_grouped(x, dt_in, qd, G, mode, thr, params=(s, z))[0],))


def test_choices_spread_and_the_search_pays():
    for i, (name, dt_in, qd, G, steps, v) in enumerate(CASES):
        if not name.startswith("gauss"):
            continue
        x, q, s, z, c = definition(i)
        assert np.unique(c).size >= (3 if qd == O.UINT2 else 2), (name, np.bincount(c))
        q0, s0, z0 = GM.quantize_grouped(x, dt_in, qd, G)
        assert M.round_trip_mse(x, dt_in, qd, G, q, s, z) < M.round_trip_mse(x, dt_in, qd, G, q0, s0, z0)


def test_the_constructed_grid_groups_spread_on_every_wire():
    """also where Gaussian data cannot: uint8, and uint4 at small group sizes"""
    for dt_in, qd in CC.PAIRS:
        for G in CC.GROUP_SIZES:
            c = M.search(CC.as_input(CC.grid_tensor(G, qd), dt_in), dt_in, qd, G, 9)[2]
            assert np.unique(c).size >= CC.grid_min_choices(qd, G), (dt_in, qd, G, c)
            assert c[-1] == 0


def test_the_short_step_line_is_crossed():
    g = [n for n, _ in CC.EDGE_GROUPS].index("short_long_line_uint8")
    for steps in (9, 12):   # float32 -> uint8 only: clip_cases.py says why no other pair has such a group
        M.assert_crosses_short_step_line(CC.as_input(CC.edge_tensor(), O.F32), O.F32, O.UINT8, 32, steps, g)


def test_groups_that_are_not_searched():
    names = [n for n, _ in CC.EDGE_GROUPS]
    for dt_in, qd in CC.PAIRS:
        x = CC.as_input(CC.edge_tensor(), dt_in)
        q, s, z, c = M.quantize_grouped_clipped(x, dt_in, qd, 32, 12)
        for n in ("all_nan", "constant", "signed_zeros", "plus_inf", "minus_inf"):
            assert c[names.index(n)] == 0, n
        assert c[-1] == 0 and c.size == len(names) + 1               # the ragged last group, spike and all
        assert qd != O.UINT2 or np.unique(c).size >= 3


def test_the_tie_is_a_tie_and_keeps_the_smaller_k():
    g = [n for n, _ in CC.EDGE_GROUPS].index("tie")
    for dt_in in (O.F32, O.BF16):
        x = CC.as_input(CC.edge_tensor(), dt_in)
        M.assert_tie(x, dt_in, O.UINT2, 32, 9, g, CC.TIE_KS)
        assert M.search(x, dt_in, O.UINT2, 32, 9)[2][g] == min(CC.TIE_KS)


def test_chunk_elems_restates_the_tile():
    from extremum_positions import GroupedTile

    for dt_in, qd in CC.PAIRS:
        for G in CC.GROUP_SIZES:
            assert CC.chunk_elems(dt_in, qd, G) == GroupedTile(G, CC.ESIZE[dt_in], CC.BITS[qd]).chunk


# ---- the wrong variants ------------------------------------------------------------------------------------------------------------------
def sequential_sum(s, e):
    return np.cumsum(s, axis=1, dtype=np.float32)[:, -1]


def contracted_first_level(s, e):
    """s[2j] + e[2j+1]^2 as one fma: the product of the odd element is not rounded before the add"""
    first = (s[:, 0::2].astype(np.float64) + e[:, 1::2].astype(np.float64) ** 2).astype(np.float32)
    return M.tree_sum(first)


def float64_sum(s, e):
    return s.astype(np.float64).sum(axis=1).astype(np.float32)


def rows_before_lanes(epv):
    """a lane's rows folded first (what the min / max fold does), then the lanes: another order whenever a group has more than 64 vectors"""
    def reduce(s, e):
        ng, G = s.shape
        v = G // epv
        if v <= 64:
            return M.tree_sum(s)
        lanes = M.tree_sum(s.reshape(-1, epv)).reshape(ng, v // 64, 64)
        rows = lanes[:, 0, :].copy()
        for r in range(1, v // 64):
            rows = rows + lanes[:, r, :]
        return M.tree_sum(rows)
    return reduce


def about_the_centre(lo, hi, r):
    c = (lo + hi) * np.float32(0.5)
    h = (hi - lo) * np.float32(0.5) * r
    return np.float32(c - h), np.float32(c + h)


def variants(dt_in):
    return {
        "a sequential sum": M.Rules(reduce=sequential_sum),
        "an fma-contracted e * e + acc": M.Rules(reduce=contracted_first_level),
        "float64 accumulation": M.Rules(reduce=float64_sum),
        "rows folded before lanes": M.Rules(reduce=rows_before_lanes(16 // CC.ESIZE[dt_in])),
        "<= instead of <": M.Rules(less=np.less_equal),
        "NaN elements not zeroed": M.Rules(zero_nan=False),
        "a bfloat16 dequantize for bfloat16 inputs": M.Rules(dequant_in_input_type=True),
        "a searched ragged group": M.Rules(search_ragged=True),
        "r_k applied to hi - lo about the centre": M.Rules(shrink=about_the_centre),
        "candidates judged with the call's stochastic threshold": M.Rules(eval_with_call_mode=True),
    }


@pytest.mark.parametrize("variant", list(variants(O.F32)))
def test_every_wrong_variant_changes_a_committed_case(variant):
    mode, thr = STOCH if "stochastic" in variant else (O.NEAREST, 0.0)
    noticed = []
    for i, (name, dt_in, qd, G, steps, v) in enumerate(CASES):
        x, q, s, z, c = definition(i, mode, thr)
        wrong = M.quantize_grouped_clipped(x, dt_in, qd, G, steps, mode, thr, rules=variants(dt_in)[variant])
        if not same(wrong, (q, s, z, c)):
            noticed.append(name)
    assert noticed, f"no committed case tells the definition from {variant}"
