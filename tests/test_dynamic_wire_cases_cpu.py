"""CPU: the inputs of tests/dynamic_wire_cases.py have teeth.  Each wrong variant of the per-chunk wire's device calls below is a small numpy model
over the oracle; for each one at least one named case gives bytes, a record or floats that differ from the right model's
(tests/dynamic_wire_model.py), so a kernel or host path with that fault fails tests/test_gpu_dynamic_wire_edges.py.  Also a condition on the
inputs: no case's expected scale is NaN or negative (the reference aborts on such a scale: nothing would define the expected bytes)."""
import numpy as np
import pytest

import dynamic_wire_cases as C
import dynamic_wire_model as M
import oracle as O
from helpers import same_floats

M32 = (1 << 32) - 1
ELEMENT = M.per_element(C.SEED, C.INDEX_BASE)


def right(case, dt_f, dt_q, round=M.NEAREST):
    return M.reduce_quantize(O, case.acc, case.terms, case.records, dt_q, dt_f, round)


def differs(a, b):
    """(bytes, record, ...) results differ in the bytes or in the record"""
    return not np.array_equal(a[0], b[0]) or not M.same_record(a[1], b[1])


def named(n, dt_f, dt_q, name):
    return next(c for c in C.sum_cases(n, dt_f, dt_q) if c.name == name)


def add_in_type(a, b, dt_f):
    """a + b rounded to dt_f"""
    if dt_f == O.F32:
        with np.errstate(invalid="ignore", over="ignore"):
            return a + b
    with np.errstate(invalid="ignore", over="ignore"):
        return O.f32_to_bf16(O.bf16_to_f32(a) + O.bf16_to_f32(b))


def quantized(y, dt_f, dt_q, params, round=M.NEAREST):
    return M.quantize(O, y, dt_f, dt_q, params[0], params[1], round), params


# ---- conditions on the inputs

@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_no_case_needs_a_nan_or_negative_scale_and_every_sum_differs_from_its_accumulator(oracle_mod, dt_f, dt_q):
    """every reduce case of the GPU file: expected scale >= 0 (or +inf); and the sum differs from acc in at least one bit pattern, or the GPU file
    could not tell the one-launch form (acc untouched) from the two-step form (acc holds the sum)"""
    seen = 0
    for n in C.SIZES:
        cases = list(C.sum_cases(n, dt_f, dt_q)) + [C.count_case(n, dt_f, dt_q, K) for K in C.REDUCE_COUNTS]
        cases += [C.padded(c, dt_q, K) for c in C.sum_cases(n, dt_f, dt_q) for K in (17, 33)]
        if dt_f == O.BF16:
            cases += [C.tie_case(n, dt_q, K) for K in (1, 2, 3)]
        for case in cases:
            _, (scale, zp), y = right(case, dt_f, dt_q)
            assert scale >= 0 and 0 <= zp <= M.QMAX[dt_q], (n, case.name, scale, zp)
            if case.terms and n > 1:   # one element: +inf + x is +inf; that size is ragged on every path, and the other cases tell there
                assert not np.array_equal(y.view(np.uint8), case.acc.view(np.uint8)), (n, case.name)
            seen += 1
    for case in C.hand_over_cases(dt_f, dt_q):
        assert right(case, dt_f, dt_q)[1][0] >= 0
    for name, acc, q, rec in C.record_cases(dt_f, dt_q):
        _, (scale, zp), _ = M.reduce_quantize(O, acc, [q], [rec], dt_q, dt_f, M.NEAREST)
        assert scale >= 0, name
    for count in C.BATCH_COUNTS:
        for _, (scale, zp) in M.quantize_batch(O, C.batch_members(count, dt_f), dt_f, dt_q, M.NEAREST):
            assert scale >= 0
    for n in (4096, 4099, 999):
        for name, x in C.edge_batch(n, dt_f):
            assert M.quantize_dynamic(O, x, dt_f, dt_q, M.NEAREST)[1][0] >= 0, (n, name)
    assert seen == 4 * (14 * 3 + len(C.REDUCE_COUNTS) + (3 if dt_f == O.BF16 else 0))


def test_the_named_sums_are_what_their_names_say(oracle_mod):
    for dt_f, dt_q in C.PAIRS:
        for n in C.SIZES:
            sums = {c.name: (C.as_f32(right(c, dt_f, dt_q)[2], dt_f), right(c, dt_f, dt_q)[1]) for c in C.sum_cases(n, dt_f, dt_q)}
            assert len(sums) == 14
            degenerate = (1.0, M.QMAX[dt_q] >> 1)
            y, p = sums["constant"]
            assert (y == M.QMAX[dt_q]).all() and p == degenerate
            y, p = sums["all nan"]
            assert np.isnan(y).all() and p == degenerate
            y, _ = sums["nan where inf meets -inf"]
            assert np.isnan(y).sum() == min(n, 3) and np.isfinite(y[~np.isnan(y)]).all()
            if n > 1:
                assert np.isposinf(sums["plus inf"][0]).sum() == 1 and not np.isneginf(sums["plus inf"][0]).any()
                assert np.isneginf(sums["minus inf"][0]).sum() == 1 and not np.isposinf(sums["minus inf"][0]).any()
                y, p = sums["both inf"]
                assert np.isposinf(y).sum() == np.isneginf(y).sum() == 1 and p[0] == np.inf
                y, _ = sums["plus and minus the largest finite value"]
                assert y.max() == C.BIG[dt_f] and y.min() == -C.BIG[dt_f]
            assert np.isposinf(sums["finite operands overflow"][0]).sum() == 1
            y, p = sums["denormals only"]
            assert (np.abs(y) < 2.0 ** -126).all() and (y != 0).any() and (p != degenerate or n == 1)
            y, _ = sums["far from zero"]
            assert y.min() >= 1e12
            assert sums["all negative"][0].max() < 0
            y, p = sums["exact cancellation"]
            assert (y == 0).all() and p == degenerate
            assert np.abs(sums["tiny range"][0]).max() < 1e-29


# ---- the wrong variants

@pytest.mark.parametrize("dt_q", C.QDS)
def test_01_bfloat16_sum_accumulated_in_float32_and_rounded_once(oracle_mod, dt_q):
    for K in (2, 3):
        case = C.tie_case(4096, dt_q, K)
        want = right(case, O.BF16, dt_q)
        y32 = M.dequantize_sum(O, case.terms, case.records, dt_q, O.F32, 4096, O.ADD, O.bf16_to_f32(case.acc))
        wrong = O.f32_to_bf16(y32)
        assert not same_floats(wrong, want[2]), "rounding after every term must differ from rounding once"
        if dt_q == O.UINT8:   # one code of uint4 or uint2 is 40 or 200 times the 2 or 4 that the sums differ by: there the floats tell (the two-step accumulator, dequantize_sum)
            assert differs(quantized(wrong, O.BF16, dt_q, M.sum_params(O, wrong, O.BF16, dt_q)), want), (K, dt_q)


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_02_03_terms_in_reverse_order_and_acc_added_last(oracle_mod, dt_f, dt_q):
    for n in C.SIZES:
        case = named(n, dt_f, dt_q, "order of the terms")
        want = right(case, dt_f, dt_q)
        assert differs(right(case._replace(terms=case.terms[::-1], records=case.records[::-1]), dt_f, dt_q), want), n
        last = add_in_type(M.dequantize_sum(O, case.terms, case.records, dt_q, dt_f, n, O.SET, None), case.acc, dt_f)
        assert differs(quantized(last, dt_f, dt_q, M.sum_params(O, last, dt_f, dt_q)), want), n


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_04_parameters_taken_from_acc_instead_of_the_sum(oracle_mod, dt_f, dt_q):
    for n in C.SIZES[:3]:   # one element is a constant tensor either way
        hit = 0
        for case in C.sum_cases(n, dt_f, dt_q):
            want = right(case, dt_f, dt_q)
            hit += differs(quantized(want[2], dt_f, dt_q, M.sum_params(O, case.acc, dt_f, dt_q)), want)
        assert hit >= 8, (n, hit)


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_05_06_nan_poisons_the_scan_or_an_all_nan_sum_keeps_the_armed_identities(oracle_mod, dt_f, dt_q):
    for n in C.SIZES[:3]:
        want = right(named(n, dt_f, dt_q, "nan where inf meets -inf"), dt_f, dt_q)
        assert not M.same_record(O.quant_params_from_minmax(np.nan, np.nan, dt_q), want[1])
    for n in C.SIZES:
        want = right(named(n, dt_f, dt_q, "all nan"), dt_f, dt_q)
        assert not M.same_record(O.quant_params_from_minmax(C.FLT_MAX, -C.FLT_MAX, dt_q), want[1])
        assert O.quant_params_from_minmax(C.FLT_MAX, -C.FLT_MAX, dt_q)[0] < 0


def concat_codes(parts, sizes, dt_q):
    """packed bytes of consecutive pieces -> packed bytes of the whole (every piece but the last a whole number of bytes)"""
    per = 8 // M.BITS[dt_q]
    assert all(s % per == 0 for s in sizes[:-1])
    return np.concatenate(parts)


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_07_batch_member_index_counted_across_the_batch(oracle_mod, dt_f, dt_q):
    for count in (16, 17, 33):
        xs = C.batch_members(count, dt_f)
        want = M.quantize_batch(O, xs, dt_f, dt_q, ELEMENT)
        begin, changed = 0, 0
        for x, (q, p) in zip(xs, want):
            wrong = M.quantize(O, x, dt_f, dt_q, p[0], p[1], M.per_element(C.SEED, C.INDEX_BASE + begin))
            if begin and x.size:
                changed += not np.array_equal(wrong, q)
            begin += x.size
        assert changed >= count // 2, (count, changed)   # members of 1, 7 or 8 elements can agree by chance


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_08_element_index_truncated_to_32_bits(oracle_mod, dt_f, dt_q):
    cut = (1 << 32) - C.INDEX_BASE
    for n in (4096, 4099):
        for case in (C.count_case(n, dt_f, dt_q, 1), named(n, dt_f, dt_q, "all negative")):
            q, p, y = right(case, dt_f, dt_q, ELEMENT)
            wrong = concat_codes([M.quantize(O, y[:cut], dt_f, dt_q, p[0], p[1], ELEMENT), M.quantize(O, y[cut:], dt_f, dt_q, p[0], p[1], M.per_element(C.SEED, 0))],
                                 [cut, n - cut], dt_q)
            assert wrong.size == q.size and np.array_equal(wrong[: cut * M.BITS[dt_q] // 8], q[: cut * M.BITS[dt_q] // 8]) and not np.array_equal(wrong, q), (n, case.name)
        xs = C.batch_members(16, dt_f)
        for x, (q, p) in zip(xs, M.quantize_batch(O, xs, dt_f, dt_q, ELEMENT)):
            if x.size >= cut + 1000:
                wrong = np.concatenate([q[: cut * M.BITS[dt_q] // 8], M.quantize(O, x[cut:], dt_f, dt_q, p[0], p[1], M.per_element(C.SEED, 0))])
                assert not np.array_equal(wrong, q)


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_09_reduce_index_counted_from_the_start_of_a_blocks_share(oracle_mod, dt_f, dt_q):
    begins = [b * C.EPV[dt_f] for b in C.fused_share_begins(C.HAND_OVER_VECS)]
    assert len(begins) == 4 and begins[1] == C.FUSED_BLOCK * C.EPV[dt_f]
    for case in C.hand_over_cases(dt_f, dt_q):
        q, p, y = right(case, dt_f, dt_q, ELEMENT)
        ends = begins[1:] + [y.size]
        wrong = concat_codes([M.quantize(O, y[b:e], dt_f, dt_q, p[0], p[1], ELEMENT) for b, e in zip(begins, ends)], [e - b for b, e in zip(begins, ends)], dt_q)
        assert wrong.size == q.size and not np.array_equal(wrong, q), case.name


def test_10_zero_point_read_as_int32(oracle_mod):
    """only uint2 -> float32 subtracts the zero point in 64 bits; everywhere else the reference narrows it, and so does the oracle"""
    hits = set()
    for dt_f, dt_q in C.PAIRS:
        for name, acc, q, rec in C.record_cases(dt_f, dt_q):
            scale, inv, zp = M.read_record(rec)
            narrow = ((zp & M32) ^ (1 << 31)) - (1 << 31)
            for op in (O.SET, O.ADD):
                want = M.dequantize_sum(O, [q], [rec], dt_q, dt_f, C.RECORD_N, op, acc)
                wrong = M.dequantize_sum(O, [q], [M.record(scale, narrow, inv)], dt_q, dt_f, C.RECORD_N, op, acc)
                if not same_floats(wrong, want):
                    hits.add((dt_f, dt_q, zp))
    assert {h[:2] for h in hits} == {(O.F32, O.UINT2)} and {h[2] for h in hits} == {1 << 31, (1 << 63) - 1, -(1 << 63)}, hits


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_11_12_reciprocal_used_as_scale_and_set_added_to_the_previous_contents(oracle_mod, dt_f, dt_q):
    for n in C.SIZES:
        for K in C.SUM_COUNTS:
            case = C.count_case(n, dt_f, dt_q, K)
            want = right(case, dt_f, dt_q)
            swapped = [M.record(M.read_record(r)[1], M.read_record(r)[2], M.read_record(r)[0]) for r in case.records]
            assert n == 1 or differs(right(case._replace(records=swapped), dt_f, dt_q), want), (n, K)   # one element: a constant sum either way, the floats below tell
            assert not same_floats(M.dequantize_sum(O, case.terms, swapped, dt_q, dt_f, n, O.SET, case.acc), M.dequantize_sum(O, case.terms, case.records, dt_q, dt_f, n, O.SET, case.acc))
            assert not same_floats(M.dequantize_sum(O, case.terms, case.records, dt_q, dt_f, n, O.ADD, case.acc), M.dequantize_sum(O, case.terms, case.records, dt_q, dt_f, n, O.SET, case.acc))


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS)
def test_13_denormal_sums_flushed_to_zero_before_the_scan(oracle_mod, dt_f, dt_q):
    for n in C.SIZES[:3]:   # one element is a constant tensor either way
        want = right(named(n, dt_f, dt_q, "denormals only"), dt_f, dt_q)
        flushed = C.as_type(np.where(np.abs(C.as_f32(want[2], dt_f)) < 2.0 ** -126, 0.0, C.as_f32(want[2], dt_f)), dt_f)
        assert not M.same_record(M.sum_params(O, flushed, dt_f, dt_q), want[1]), n
