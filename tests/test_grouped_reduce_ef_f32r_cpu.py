"""CPU: the inputs of tests/reduce_ef_f32r_cases.py discriminate.  The fused reduce of a bfloat16 accumulator with a float32 residual must round
the running sum to bfloat16 after EVERY term; a kernel that kept it in float32 and rounded once would pass any test whose inputs never land on a
tie.  So: on the hand-built tie inputs the model that sums in float32 differs from the definition (tests/grouped_ef_f32r_sim.py:
reduce_ef_f32r_step) for every wire type, the ties are the ties the docstring claims, and swapping two terms changes the result."""
import numpy as np
import pytest

import oracle as O
from grouped_ef_f32r_sim import reduce_ef_f32r_step
from reduce_ef_f32r_cases import ACC_CYCLE, TIE_ORDERS, add_terms, differs, float32_sum_variant, reduce_ef_f32r_model, tie_case

QDS = [O.UINT8, O.UINT4, O.UINT2]
G, N = 128, 3 * 128 + 65


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def _values(bits):
    return O.bf16_to_f32(bits)


@pytest.mark.parametrize("qd", QDS)
def test_the_hand_built_terms_are_the_ties_they_claim(qd):
    acc, _, t = tie_case(qd, G, N)
    cyc = np.array(ACC_CYCLE, dtype=np.float32)[np.arange(N) % len(ACC_CYCLE)]
    one, odd = cyc == 1.0, cyc == 1.0078125
    assert one.any() and odd.any()
    for name, units in (("A", 1), ("B", 1), ("C", 2)):
        d = _values(add_terms(np.zeros(N, dtype=np.uint16), [t[name]], qd, G))
        assert np.array_equal(d, np.full(N, units * 2.0 ** -8, dtype=np.float32)), name
    after_a = _values(add_terms(acc, [t["A"]], qd, G))
    assert np.all(after_a[one] == 1.0), "1.0 + 2^-8 is a tie that rounds to even: down"
    assert np.all(after_a[odd] == 1.015625), "1.0078125 + 2^-8 is a tie that rounds to even: up"
    after_ab = _values(add_terms(acc, [t["A"], t["B"]], qd, G))
    assert np.all(after_ab[one] == 1.0), "two terms of 2^-8, each rounded: 1.0 twice (a float32 running sum gives 1.0078125)"
    ac, ca = _values(add_terms(acc, [t["A"], t["C"]], qd, G)), _values(add_terms(acc, [t["C"], t["A"]], qd, G))
    assert np.all(ac[one] == 1.0078125) and np.all(ca[one] == 1.015625), "the order of the terms shows"


@pytest.mark.parametrize("qd", QDS)
def test_a_float32_running_sum_differs_on_the_tie_inputs(qd):
    acc, r, t = tie_case(qd, G, N)
    for order in TIE_ORDERS:
        terms = [t[c] for c in order]
        want = reduce_ef_f32r_step(acc, r, terms, qd, G)[:4]
        mine = reduce_ef_f32r_model(acc, r, terms, qd, G)
        assert not differs(want, mine) and np.array_equal(want[1], mine[1]) and np.array_equal(want[2], mine[2]), "the test's model is the committed one"
        assert differs(want, float32_sum_variant(acc, r, terms, qd, G)), f"qd={qd} order={order}: summing in float32 gives the same bytes and residual"


@pytest.mark.parametrize("qd", QDS)
def test_swapping_two_terms_changes_the_result(qd):
    acc, r, t = tie_case(qd, G, N)
    assert differs(reduce_ef_f32r_step(acc, r, [t["A"], t["C"]], qd, G)[:4], reduce_ef_f32r_step(acc, r, [t["C"], t["A"]], qd, G)[:4])
