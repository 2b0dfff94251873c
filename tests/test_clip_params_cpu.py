"""CPU: the model of the histogram clip search for per-tensor parameters (tests/clip_params_model.py) on the committed cases, and the proof that
each decision of the definition is pinned by them: a model with exactly one wrong rule must change the result -- counts, error words, choice or
record -- of at least one case.

One rule cannot be pinned by any input, and the test of it says why instead of pretending: "an empty bin adds exactly +0".  With a finite range
every centre m_j, every d and so every e is finite, e * e <= 4.7e77 does not overflow binary64, and 0 * (e * e) is +0 already.  With an infinite
range the scale is +inf and the epilogue's zero point is 0 (lo finite, hi = +inf: z = round(-lo / inf) = 0; lo = -inf: -lo / s is inf / inf, a NaN
that the clamp sends to 0), so for a POPULATED bin too u = 0 (m / inf is 0 or NaN, floor(0 + 0.5) = 0) and d = (0 - 0) * inf is NaN: e is NaN in
every bin, populated or empty, and E_k is NaN under either rule.  The cases "plus_inf_only" and "minus_inf_only" pin that half, "range_overflows"
the finite half.  The rule stays in the definition because it spares the kernel the multiplication, not because a result depends on it.

The true round trip: on 2^20 N(0,1) float32 elements the oracle's nearest quantize / dequantize with the chosen parameters loses less than with
min/max on uint8, uint4 and uint2.  Measured ratios (python tests/clip_params_model.py): 0.864 / 0.375 / 0.226.
"""
import dataclasses

import numpy as np
import pytest

import clip_params_model as M
import oracle as O

WIRES = (O.UINT8, O.UINT4, O.UINT2)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def cases():
    """(name, dt_in, qd, steps, float32 values): the edge tensors on every wire and a seeded Gaussian"""
    out = []
    for name, v in M.edge_tensors():
        for qd in WIRES:
            out.append((f"{name}-{qd}", O.F32, qd, 63, v))
        out.append((f"{name}-bf16", O.BF16, O.UINT4, 63, v))
    g = np.random.default_rng(5).standard_normal(20_000).astype(np.float32)
    for qd in WIRES:
        out.append((f"gaussian-{qd}", O.F32, qd, 63, g))
    out.append(("gaussian-bf16", O.BF16, O.UINT2, 17, g))
    return out


CASES = cases()


def result(case, rules=M.DEFINITION):
    _, dt_in, qd, steps, v = case
    s, z, k, E, c = M.compute_quant_params_clipped(M.as_input(v, dt_in), dt_in, qd, steps, rules)
    return M.record_bytes(s, z), k, E.view(np.uint64).tobytes(), c.tobytes()


@pytest.fixture(scope="module")
def definition_results():
    return [result(c) for c in CASES]   # computed once, shared


def test_the_model_on_the_committed_cases(definition_results):
    by_name = {c[0]: (c, r) for c, r in zip(CASES, definition_results)}
    for name in ("constant", "all_nan"):
        for qd in WIRES:
            case, (rec, k, E, c) = by_name[f"{name}-{qd}"]
            assert (rec, k) == (M.record_bytes(1.0, M.QMAX[qd] >> 1), 0)
            assert np.isnan(np.frombuffer(E, dtype=np.float64)).all() and not np.frombuffer(c, dtype=np.uint64).any()
    for case, (rec, k, E, c) in zip(CASES, definition_results):
        _, dt_in, qd, steps, v = case
        x = M.as_input(v, dt_in)
        lo, hi = M.minmax(x, dt_in)
        counts, errors = np.frombuffer(c, dtype=np.uint64), np.frombuffer(E, dtype=np.float64)
        if hi > lo:
            assert counts.sum() == np.count_nonzero(~np.isnan(M.as_f32(x, dt_in)))          # every non-NaN element in exactly one bin
        assert 0 <= k < steps and np.isnan(errors[steps:]).all()
        assert not (errors[k] > errors[0]) or np.isnan(errors[0])
        s0, z0 = M.epilogue(lo, hi, qd)
        if k == 0:
            assert rec == M.record_bytes(s0, z0)                                            # candidate 0 is the plain call's pair
        assert result((case[0], dt_in, qd, 1, v))[:2] == (M.record_bytes(s0, z0), 0)       # steps == 1
    # the top clamp: every integer 0 .. 8192 on a bin edge, hi itself in bin 8191
    c = np.frombuffer(by_name[f"bin_edges_and_top-{O.UINT2}"][1][3], dtype=np.uint64)
    assert c[8191] == 3 and c[0] == 2 and c[64] == 2 and c[1] == 1 and c.sum() == 8193 + 129
    # everything but the two extremes in one bin
    c = np.frombuffer(by_name[f"one_bin-{O.UINT2}"][1][3], dtype=np.uint64)
    assert sorted(c[c > 0].tolist()) == [1, 1, 1998]
    # the tie keeps the smallest k; candidates whose shrunk range is empty are not evaluated
    x = M.as_input(dict(M.edge_tensors())["tie"], O.F32)
    lo, hi = M.minmax(x, O.F32)
    M.assert_tie(lo, hi, M.histogram(x, O.F32, lo, hi), O.UINT2, 63, M.TIE_KS)
    rec, k, E, _ = by_name[f"tie-{O.UINT2}"][1]
    assert k == 0 and np.isnan(np.frombuffer(E, dtype=np.float64)[54:]).all()


VARIANTS = {
    "bin_by_rounding": dict(bin_of=np.rint),
    "no_clamp_at_bin_8191": dict(clamp_top=False),
    "nans_counted": dict(count_nans=True),
    "float32_centres": dict(centre_dtype=np.float32),
    "floor_t_for_floor_t_plus_half": dict(round_half=0.0),
    "sequential_sum_for_the_tree": dict(reduce=M.sequential_sum),
    "less_equal_for_less": dict(less=np.less_equal),
    "zero_point_left_out_of_d": dict(zp_in_d=False),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_a_wrong_variant_changes_a_committed_case(definition_results, name):
    rules = dataclasses.replace(M.DEFINITION, **VARIANTS[name])
    changed = [c[0] for c, want in zip(CASES, definition_results) if result(c, rules) != want]
    assert changed, f"no committed case notices the variant {name}"


def test_empty_bins_not_forced_to_zero_cannot_change_any_result(definition_results):
    """the ninth variant: see the module docstring for why no input can show it; here, that none of the committed cases does -- the infinite ranges
    among them included -- and that on a finite range every e is finite"""
    rules = dataclasses.replace(M.DEFINITION, zero_empty=False)
    assert [result(c, rules) for c in CASES] == definition_results
    for name in ("plus_inf_only", "minus_inf_only"):   # the infinite half: scale +inf, zero point 0, every evaluated E_k NaN whatever the counts
        x = M.as_input(dict(M.edge_tensors())[name], O.F32)
        lo, hi = M.minmax(x, O.F32)
        assert np.isinf(lo) != np.isinf(hi)
        for qd in WIRES:
            ok, s, z = M.candidate(lo, hi, 0, qd)
            assert ok and np.isinf(s) and z == 0
            for counts in (M.histogram(x, O.F32, lo, hi), np.ones(M.BINS, dtype=np.uint64)):
                assert np.isnan(M.candidate_error(counts, lo, hi, s, z, qd, rules)) and np.isnan(M.candidate_error(counts, lo, hi, s, z, qd))
    x = M.as_input(dict(M.edge_tensors())["range_overflows"], O.F32)
    lo, hi = M.minmax(x, O.F32)
    for k in (0, 31, 62):
        _, s, z = M.candidate(lo, hi, k, O.UINT2)
        ones = np.ones(M.BINS, dtype=np.uint64)
        assert np.isfinite(M.candidate_error(ones, lo, hi, s, z, O.UINT2, dataclasses.replace(M.DEFINITION, reduce=lambda t: t.max())))


def test_the_true_round_trip_improves_on_a_gaussian():
    x = np.random.default_rng(0).standard_normal(1 << 20).astype(np.float32)
    for qd, wire in zip(WIRES, ("uint8", "uint4", "uint2")):
        s, z, k, E, _ = M.compute_quant_params_clipped(x, O.F32, qd, 63)
        s0, z0 = O.compute_quant_params(x, O.F32, qd)
        with_search, without = M.round_trip_mse(x, O.F32, qd, s, z), M.round_trip_mse(x, O.F32, qd, s0, z0)
        print(f"\nhistogram clip search, N(0,1), 2^20, {wire}: k = {k}, round-trip MSE {with_search:.6g} / {without:.6g} = {with_search / without:.3f}, "
              f"estimate / true = {E[k] / x.size / with_search:.4f}")
        assert with_search < without
