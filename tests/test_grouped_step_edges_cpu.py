"""CPU: conditions on the inputs of tests/test_gpu_grouped_step_edges.py (tests/grouped_edge_cases.py), asserted with the model alone, so that a
generator that drifts cannot hollow out the GPU tests -- and the mathematics of taking the short rounding step with per-group computed parameters:
on the bounded groups the numpy short steps of tests/test_short_step_model.py give the model's bytes.  The thresholds here (10 %, more than 0)
are conditions on inputs, not tolerances."""
import numpy as np
import pytest

import grouped_edge_cases as E
import oracle as O
from grouped_edge_cases import unpack
from grouped_model import group_minmax, group_params_all, quantize_grouped
from test_short_step_model import short_nearest, short_stochastic

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
TAUS = (0.0, 0.25, 0.375, 0.37499997, 0.5, 0.99999994)


def as_input(bits, dt_in):
    return bits.view(np.float32) if dt_in == O.F32 else bits


@pytest.fixture(scope="module", params=[(p, G) for p in PAIRS for G in (32, 128, 4096)], ids=lambda v: f"dt{v[0][0]}-q{v[0][1]}-G{v[1]}")
def case(request, oracle_mod):
    (dt_in, qd), G = request.param
    bits, lay = E.edge_tensor(dt_in, qd, G, seed=0)
    xf = E.values(bits)
    s, z = group_params_all(xf, G, qd)
    lo, hi = group_minmax(xf, G)
    return dt_in, qd, G, bits, lay, xf, s, z, E.bounded_by_product_rule(lo, hi, s)


def test_layout(case):
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    assert lay.chunk == E.chunk_elems(dt_in, qd, G) and lay.sections["S"][0] == 0 and lay.sections["T"][1] == lay.n == bits.size
    assert lay.n % 4 in (1, 3) and 0 < lay.n - lay.sections["T"][0] < lay.chunk and lay.n % G != 0
    assert len(lay.chunks_of("S")) == len(lay.chunks_of("L")) == E.STEP_CHUNKS >= 3
    assert len(lay.cls) == len(lay.section) == len(lay.origin) == s.size
    assert lay.n < 100_000


def test_a_tenth_of_the_short_step_section_sits_on_a_decision_edge(case):
    """an element is on a decision edge when the model's nearest code changes as the element moves by one ulp of the input type"""
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    b, e = lay.sections["S"]
    x = bits[b:e]
    ng = (e - b) // G
    params = (s[:ng], z[:ng])
    base = unpack(quantize_grouped(as_input(x, dt_in), dt_in, qd, G, params=params)[0], qd, e - b)
    finite = np.isfinite(xf[b:e]) & (xf[b:e] != 0)
    edge = np.zeros(e - b, dtype=bool)
    for step in (1, -1):
        moved = np.where(finite, (x.astype(np.int64) + step).astype(x.dtype), x)
        edge |= unpack(quantize_grouped(as_input(moved, dt_in), dt_in, qd, G, params=params)[0], qd, e - b) != base
    share = edge.mean()
    print(f"pair ({dt_in}, {qd}) G={G}: {100 * share:.1f} % of S on a decision edge")
    assert share >= 0.10


def test_exact_fractions_of_the_product(case):
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    b, e = lay.sections["S"]
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / s[: (e - b) // G]
        p = (xf[b:e] * np.repeat(inv, G)).astype(np.float32)
        frac = np.abs(p - np.trunc(p))
    for tau in (0.25, 0.375, 0.5):
        count = int((frac == np.float32(tau)).sum())
        print(f"pair ({dt_in}, {qd}) G={G}: {count} products ({100 * count / (e - b):.2f} %) with the fractional part {tau}")
        if dt_in == O.F32:
            assert count > 0, tau


def test_which_chunks_take_which_step(case):
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    for c in lay.chunks_of("S"):
        assert all(bounded[g] for g in c), [lay.describe(g) for g in c if not bounded[g]]
    for c in lay.chunks_of("L"):
        assert any(not bounded[g] for g in c), f"no unbounded group in the chunk of {lay.describe(c[0])}"
        assert lay.NG == 1 or any(bounded[g] for g in c)
    for g in lay.groups_of("L"):
        if lay.origin[g] < 0:
            assert lay.cls[g] == "zeros" or not bounded[g], lay.describe(g)
    qmax = E.QMAX[qd]
    assert (z == 0).any() and (z == qmax).any() and ((z > 0) & (z < qmax)).any()
    assert set(E.bounded_classes(dt_in, qd)) <= {lay.cls[g] for g in lay.groups_of("S")}
    assert set(E.unbounded_classes(dt_in, qd)) <= {lay.cls[g] for g in lay.groups_of("L")}


def test_line_groups_sit_on_the_line(case):
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    if (dt_in, qd) != (O.F32, O.UINT8):
        return
    lo, hi = group_minmax(xf, G)
    line = np.float32(1.0e9)
    seen = set()
    for g, name in enumerate(lay.cls):
        if name.startswith("line_") and lay.bounds(g)[1] - lay.bounds(g)[0] == G:
            prod = np.float32(max(abs(lo[g]), abs(hi[g])) * (np.float32(1.0) / s[g]))
            want = (np.nextafter(line, np.float32(0)),) if name == "line_below" else (line, np.nextafter(line, np.float32(np.inf)))
            assert prod in want, (lay.describe(g), prod)
            seen.add(name)
    assert seen == {"line_below", "line_above"}


def test_copies_are_bit_identical(case):
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    copies = {"L": 0, "T": 0}
    for g in list(lay.groups_of("L")) + list(lay.groups_of("T")):
        o = lay.origin[g]
        if o < 0:
            continue
        b, e = lay.bounds(g)
        assert np.array_equal(bits[b:e], bits[o * G: o * G + (e - b)]), lay.describe(g)
        copies[lay.section[g]] += 1
    assert copies["L"] >= E.STEP_CHUNKS * (lay.NG - 1) - E.STEP_CHUNKS and copies["T"] == len(lay.groups_of("T")) >= 1
    assert copies["L"] > 0 or lay.NG == 1


def test_short_steps_give_the_models_bytes_on_the_bounded_groups(case):
    """quantize_vec_short with each group's own computed parameters, in numpy float32, against the model"""
    dt_in, qd, G, bits, lay, xf, s, z, bounded = case
    generic = dt_in == O.F32 and qd == O.UINT2   # the one nearest pair with the generic std::round step
    for g in lay.groups_of("S"):
        b, e = lay.bounds(g)
        x = as_input(bits[b:e], dt_in)
        with np.errstate(all="ignore"):
            inv = np.float32(1.0) / s[g]
        want = O.quantize(x, dt_in, qd, float(s[g]), int(z[g]))
        assert np.array_equal(short_nearest(xf[b:e], inv, int(z[g]), qd, generic=generic), want), lay.describe(g)
        for tau in TAUS:
            want = O.quantize(x, dt_in, qd, float(s[g]), int(z[g]), O.STOCHASTIC, tau)
            assert np.array_equal(short_stochastic(xf[b:e], inv, int(z[g]), qd, tau), want), (lay.describe(g), tau)
