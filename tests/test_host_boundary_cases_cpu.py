"""CPU: the cases of tests/host_boundary_cases.py have teeth.  The staging loop of csrc/capi.cpp is restated there over the oracle with one fault
switched on at a time; without a fault the restatement gives the whole-call model, and every fault changes the bytes, the floats or the parameters
of a case that tests/test_gpu_host_boundary.py runs -- so a library with that fault fails there.  One or two pairs per fault: an oracle call over
three chunks takes about a second."""
import re
from pathlib import Path

import numpy as np
import pytest

import host_boundary_cases as H
import oracle as O
from helpers import same_floats

C, N2, N3 = H.C, H.N2, H.N3


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def test_the_chunk_is_the_librarys():
    text = (Path(__file__).resolve().parent.parent / "pi-quant_amd" / "csrc" / "context.hpp").read_text()
    m = re.search(r"constexpr\s+size_t\s+kStageChunkElems\s*=\s*size_t\s*\{\s*1\s*\}\s*<<\s*(\d+)\s*;", text)
    assert m, "kStageChunkElems is no longer written as size_t{1} << k: restate it here and in tests/host_boundary_cases.py"
    assert 1 << int(m.group(1)) == C


def test_the_sizes_are_what_the_cases_need():
    assert C < N2 < 2 * C and 2 * C < N3 < 3 * C
    assert N2 % 2 == 1 and N2 % 4 == 3, "the ragged tail must end inside a packed byte of uint4 and of uint2"
    assert H.INDEX_BASE + C < 1 << 32 < H.INDEX_BASE + N2, "index 2^32 must fall into the second chunk"
    assert H.INDEX_BASE_BELOW + C < H.INDEX_BASE_BELOW + N2 - 1 < 1 << 32, "the second base keeps every index of the second chunk in 32 bits"
    for n in (N2, N3):
        p = H.seam_positions(n)
        assert len(set(p)) == 6 and max(p) == n - 1 and {C - 1, C, C + 1} <= set(p)
    assert {2 * C - 1, 2 * C} <= set(H.seam_positions(N3))
    chunk_of = lambda i: i // C
    pairs = H.scan_pairs(N3)
    assert {chunk_of(a) for a, _ in pairs} == {chunk_of(b) for _, b in pairs} == {0, 1, 2}, "each chunk must hold each extremum at least once"
    assert all(a != b for a, b in pairs)


def test_the_planted_values_are_there_and_every_chunk_differs():
    for dt_f, dt_q in ((O.F32, O.UINT8), (O.BF16, O.UINT4)):
        x = H.quant_input(N2, dt_f, dt_q)
        f = x if dt_f == O.F32 else O.bf16_to_f32(x)
        v = f[H.seam_positions(N2)]
        scale = H.QUANT_PARAMS[dt_q][0]
        assert v[0] / np.float32(scale) == 2.5 and np.isnan(v[1]) and v[2] == np.inf and v[3] == -np.inf
        assert v[4] == 0 and np.signbit(v[4]) and 0 < v[5] < 2.0 ** -126
        assert not np.array_equal(f[:4099], f[C: C + 4099])
    a = H.accumulator(N3, O.BF16)
    v = O.bf16_to_f32(a[H.seam_positions(N3)])
    assert np.isnan(v[0]) and v[1] == np.inf and v[2] == -np.inf and np.signbit(v[3]) and v[3] == 0 and np.isnan(v[4]) and v[5] == np.inf
    x = H.scan_input(N3, O.BF16, C - 1, 2 * C)
    assert O.minmax(x, O.BF16) == (H.SCAN_MIN, H.SCAN_MAX) and ((x & 0x7FFF) > 0x7F80).sum() > 30


# ---- without a fault, the restated loop is the whole call
def test_the_restated_loop_without_a_fault_is_the_whole_call():
    x = H.quant_input(N2, O.F32, O.UINT4)
    assert np.array_equal(H.staged_quantize(x, O.F32, O.UINT4, H.PER_ELEMENT), H.quantize_model(x, O.F32, O.UINT4, H.PER_ELEMENT))
    for device in ("in", "out"):
        assert np.array_equal(H.staged_quantize(x, O.F32, O.UINT4, H.STOCHASTIC, device=device), H.quantize_model(x, O.F32, O.UINT4, H.STOCHASTIC))
    q, acc = H.codes_input(N3, O.UINT4), H.accumulator(N3, O.BF16)
    assert same_floats(H.staged_dequantize(q, O.UINT4, O.BF16, N3, O.ADD, acc), H.dequantize_model(q, O.UINT4, O.BF16, N3, O.ADD, acc))
    x = H.scan_input(N3, O.F32, 2 * C, C - 1)
    assert H.staged_scan(x, O.F32, O.UINT8) == H.scan_model(x, O.F32, O.UINT8)


# ---- the faults
QUANT_FAULTS = [
    # fault, size, pair, rounding, device
    ("index_restarted", N2, (O.F32, O.UINT8), H.PER_ELEMENT, None),
    ("index_restarted", N2, (O.F32, O.UINT4), H.PER_ELEMENT, "out"),
    ("threshold_redrawn", N2, (O.F32, O.UINT4), H.STOCHASTIC, None),
    ("stale_slot", N3, (O.BF16, O.UINT2), H.NEAREST, None),
    ("tail_byte_dropped", N2, (O.F32, O.UINT4), H.NEAREST, None),
    ("tail_byte_dropped", N2, (O.BF16, O.UINT2), H.STOCHASTIC, None),
    ("seam_early", N2, (O.F32, O.UINT4), H.NEAREST, None),
    ("seam_late", N2, (O.F32, O.UINT2), H.PER_ELEMENT, None),
    ("device_offset_twice", N2, (O.F32, O.UINT4), H.NEAREST, "in"),
    ("device_offset_twice", N2, (O.F32, O.UINT4), H.NEAREST, "out"),
    ("device_offset_missing", N2, (O.F32, O.UINT4), H.NEAREST, "in"),
    ("device_offset_missing", N2, (O.F32, O.UINT4), H.PER_ELEMENT, "out"),
]


@pytest.mark.parametrize("fault,n,pair,rounding,device", QUANT_FAULTS, ids=[f"{f}-{H.NAME[p[0]]}-{H.NAME[p[1]]}-{r[0]}-{d}" for f, _, p, r, d in QUANT_FAULTS])
def test_a_faulty_quantize_loop_changes_the_bytes(fault, n, pair, rounding, device):
    x = H.quant_input(n, *pair)
    want = H.quantize_model(x, *pair, rounding)
    wrong = H.staged_quantize(x, *pair, rounding, fault=fault, device=device)
    assert wrong.size == want.size and not np.array_equal(wrong, want)
    first = int(np.flatnonzero(wrong != want)[0]) * H.PACK[pair[1]]
    if fault == "tail_byte_dropped":
        assert first >= n - H.PACK[pair[1]], "only the last byte tells"
    if fault in ("index_restarted", "threshold_redrawn"):
        assert first >= C, "the first chunk is right under these faults: only a call of more than one chunk tells"


DEQUANT_FAULTS = [
    # fault, size, form, device
    ("stale_slot", N3, (O.UINT4, O.BF16, O.ADD), None),
    ("acc_not_uploaded", N2, (O.UINT8, O.F32, O.ADD), None),
    ("acc_not_uploaded", N3, (O.UINT4, O.BF16, O.ADD), None),
    ("acc_from_offset_0", N2, (O.UINT8, O.F32, O.ADD), None),
    ("tail_byte_dropped", N2, (O.UINT2, O.F32, O.SET), None),
    ("seam_early", N2, (O.UINT2, O.F32, O.SET), None),
    ("seam_late", N2, (O.UINT4, O.BF16, O.ADD), None),
    ("device_offset_twice", N2, (O.UINT8, O.BF16, O.ADD), "in"),
    ("device_offset_twice", N2, (O.UINT8, O.BF16, O.ADD), "out"),
    ("device_offset_missing", N2, (O.UINT2, O.F32, O.SET), "in"),
    ("device_offset_missing", N2, (O.UINT2, O.F32, O.SET), "out"),
]


@pytest.mark.parametrize("fault,n,form,device", DEQUANT_FAULTS, ids=[f"{f}-{H.NAME[q]}-{H.NAME[t]}-{'add' if op else 'set'}-{d}" for f, _, (q, t, op), d in DEQUANT_FAULTS])
def test_a_faulty_dequantize_loop_changes_the_floats(fault, n, form, device):
    dt_q, dt_f, op = form
    q, acc = H.codes_input(n, dt_q), H.accumulator(n, dt_f)
    want = H.dequantize_model(q, dt_q, dt_f, n, op, acc)
    wrong = H.staged_dequantize(q, dt_q, dt_f, n, op, acc, fault=fault, device=device)
    assert not same_floats(wrong, want)
    if fault == "acc_not_uploaded" and n == N3:   # only the reuse of slot 0 tells what a fresh slot (zeros here, anything in the library) cannot
        assert not same_floats(wrong[2 * C:], want[2 * C:])


@pytest.mark.parametrize("dt_f", [O.F32, O.BF16], ids=["fp32", "bf16"])
def test_a_faulty_scan_fold_changes_the_parameters(dt_f):
    """each chunk left out is noticed by a pair of positions that has an extremum in it; the last chunk alone by every pair with one outside it"""
    noticed = {0: 0, 1: 0, 2: 0}
    last_only = 0
    for pos_min, pos_max in H.scan_pairs(N3):
        x = H.scan_input(N3, dt_f, pos_min, pos_max)
        want = H.scan_model(x, dt_f, O.UINT8)
        assert H.staged_scan(x, dt_f, O.UINT8) == want
        for k in range(3):
            wrong = H.staged_scan(x, dt_f, O.UINT8, fault="scan_chunk_left_out", left_out=k)
            assert (wrong != want) == (k in (pos_min // C, pos_max // C)), (pos_min, pos_max, k)
            noticed[k] += wrong != want
        last_only += H.staged_scan(x, dt_f, O.UINT8, fault="scan_last_chunk_only") != want
    assert min(noticed.values()) >= 2 and last_only == len(H.scan_pairs(N3))


def test_every_fault_has_a_proof():
    proven = {f for f, *_ in QUANT_FAULTS} | {f for f, *_ in DEQUANT_FAULTS} | {"scan_chunk_left_out", "scan_last_chunk_only"}
    assert proven == set(H.FAULTS)
