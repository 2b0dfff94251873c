"""Inputs for the per-chunk wire's device calls (quantize_dynamic_batch, reduce_quantize_dynamic, dequantize_sum, dequantize_dynamic_batch) at
their edges.  Small seeded generators; every case names itself.  tests/test_dynamic_wire_cases_cpu.py proves on the CPU that the cases tell the
right model (tests/dynamic_wire_model.py) from thirteen wrong ones, and that no case needs a NaN or negative computed scale;
tests/test_gpu_dynamic_wire_edges.py runs them on the device.

Sum cases are built as an accumulator, packed term codes and HAND-WRITTEN 16-byte term records, so that acc + sum of the dequantized terms is known
by construction (constant, all NaN, NaN where +inf meets -inf, ...).  Term values are (code - zero point) * scale with scales that keep that product
exact in both dequantize forms ((q - zp) * s and fma(q, s, -zp * s)).
"""
from typing import NamedTuple

import numpy as np

import dynamic_wire_model as M
import oracle as O

F32, BF16, UINT2, UINT4, UINT8 = O.F32, O.BF16, O.UINT2, O.UINT4, O.UINT8
PAIRS = [(F32, UINT8), (F32, UINT4), (F32, UINT2), (BF16, UINT8), (BF16, UINT4), (BF16, UINT2)]
QDS = (UINT8, UINT4, UINT2)
EPV = {F32: 4, BF16: 8}       # elements per 16-byte vector
ESIZE = {F32: 4, BF16: 2}
SIZES = (8, 4096, 4099, 1)    # whole vectors (one-launch reduce), ragged (two-step)

SEED = 0x5EED_0123_4567_89AB
INDEX_BASE = (1 << 32) - 1000   # the element index crosses 2^32 inside every tensor of more than 1000 elements
TAU = 0.28125
ROUNDS = (("nearest", M.NEAREST), ("per call", M.per_call(TAU)), ("per element", M.per_element(SEED, INDEX_BASE)))

REDUCE_COUNTS = (0, 1, 15, 16, 17, 32, 33)     # 16 = kDequantSumMaxInputs: the last count the one-launch reduce takes
SUM_COUNTS = (1, 16, 17, 33)
BATCH_COUNTS = (1, 2, 16, 17, 33)              # 16 = kFusedBatchMax = kDequantBatchMaxInputs

FLT_MAX = float(np.finfo(np.float32).max)
BF16_MAX = float(O.bf16_to_f32(np.array([0x7F7F], dtype=np.uint16))[0])
BIG = {F32: FLT_MAX, BF16: BF16_MAX}                       # the largest finite value of the accumulator's type
DENORMAL_UNIT = {F32: 2.0 ** -149, BF16: 2.0 ** -133}      # its smallest denormal
ORDER_BIG = {F32: 2.0 ** 24, BF16: 256.0}                  # from here on the type's ulp is 2: k + ORDER_BIG is a tie for odd k


class SumCase(NamedTuple):
    name: str
    acc: np.ndarray       # dt_f representation
    terms: list           # packed bytes per term
    records: list         # 16 bytes per term


def as_type(x, dt_f):
    x = np.asarray(x, dtype=np.float32)
    return x.copy() if dt_f == F32 else O.f32_to_bf16(x)


def as_f32(y, dt_f):
    return y if dt_f == F32 else O.bf16_to_f32(y)


def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key])


def _spots(rng, n, k):
    return rng.choice(n, min(n, k), replace=False)


def _term(codes, dt_q, scale, zp):
    return M.pack(np.asarray(codes, dtype=np.uint8), dt_q), M.record(scale, zp)


def ordinary_acc(rng, n, dt_f):
    return as_type(rng.uniform(-2, 2, n), dt_f)


def ordinary_term(rng, n, dt_q, i=0):
    """codes over the whole range with an ordinary positive scale and a zero point in range; term i has its own scale and zero point"""
    Q = M.QMAX[dt_q]
    codes = rng.integers(0, Q + 1, n).astype(np.uint8)
    return _term(codes, dt_q, np.float32((2.0 + i % 5) / Q), (Q // 2 + 3 * i) % (Q + 1))


def sum_cases(n, dt_f, dt_q):
    """the sum cases of the reduce for one size and one pair"""
    Q = M.QMAX[dt_q]
    big, unit = BIG[dt_f], DENORMAL_UNIT[dt_f]

    def case(idx):
        return _rng(n, dt_f, dt_q, idx)

    # 1. constant: acc = m, term 1 = Q - m, term 2 = exactly 0
    rng = case(1)
    m = rng.integers(0, Q + 1, n)
    m[0] = 0
    yield SumCase("constant", as_type(m, dt_f), *zip(_term(Q - m, dt_q, 1.0, 0), _term(np.ones(n), dt_q, 0.5, 1)))
    # 2. all NaN: a term whose scale is NaN
    rng = case(2)
    codes = rng.integers(0, Q + 1, n)
    yield SumCase("all nan", ordinary_acc(rng, n, dt_f), *zip(_term(codes, dt_q, np.nan, Q // 2), ordinary_term(rng, n, dt_q, 1)))
    # 3. NaN only where +inf of acc meets -inf of a term (code 2 * -BIG overflows; code 0 gives -0, which changes nothing)
    rng = case(3)
    a = rng.uniform(-2, 2, n)
    p = _spots(rng, n, 3)
    a[p] = np.inf
    codes = np.zeros(n)
    codes[p] = 2
    yield SumCase("nan where inf meets -inf", as_type(a, dt_f), *zip(_term(codes, dt_q, -big, 0), ordinary_term(rng, n, dt_q, 1)))
    # 4. one +inf (in acc), one -inf (from a term), both
    for name, plus, minus in (("plus inf", True, False), ("minus inf", False, True), ("both inf", True, True)):
        rng = case(4 + plus + 2 * minus)
        a = rng.uniform(-2, 2, n)
        p = _spots(rng, n, 2)
        codes = np.zeros(n)
        if plus:
            a[p[0]] = np.inf
        if minus:
            codes[p[-1]] = 2
        yield SumCase(name, as_type(a, dt_f), *zip(_term(codes, dt_q, -big, 0), ordinary_term(rng, n, dt_q, 1)))
    # 5. finite operands whose sum overflows: 0.9 BIG + 0.9 BIG
    rng = case(8)
    a = rng.uniform(-2, 2, n)
    p = _spots(rng, n, 1)
    near = float(as_f32(as_type([0.9 * big], dt_f), dt_f)[0])
    a[p] = near
    codes = np.zeros(n)
    codes[p] = 1
    yield SumCase("finite operands overflow", as_type(a, dt_f), *zip(_term(codes, dt_q, near, 0), ordinary_term(rng, n, dt_q, 1)))
    # 6. +BIG (acc) and -BIG (term: code 0 with zero point 1) both present: the range fits only in the epilogue's doubles
    rng = case(9)
    a = rng.uniform(-2, 2, n)
    p = _spots(rng, n, 2)
    codes = np.ones(n)
    codes[p[-1]] = 0
    a[p[-1]] = 0.0
    if n > 1:
        a[p[0]] = big
    yield SumCase("plus and minus the largest finite value", as_type(a, dt_f), *zip(_term(codes, dt_q, big, 1)))
    # 7. denormals only: (k + code - zp) units with |..| <= 90 < 128 units (still denormal in bfloat16)
    rng = case(10)
    k = rng.integers(-30, 31, n)
    zp = Q // 2
    codes = rng.integers(max(0, zp - 60), min(Q, zp + 60) + 1, n)
    codes[0] = min(Q, zp + 1)
    yield SumCase("denormals only", as_type(k * unit, dt_f), *zip(_term(codes, dt_q, unit, zp)))
    # 8. tiny range
    rng = case(11)
    codes = rng.integers(0, Q + 1, n)
    codes[0] = 0
    yield SumCase("tiny range", as_type(1e-30 * rng.uniform(-1, 1, n), dt_f), *zip(_term(codes, dt_q, 1e-32 * 256 / (Q + 1), Q // 2)))
    # 9. far from zero: the zero point clamps to 0 and every x / scale is beyond 2^31
    rng = case(12)
    codes = rng.integers(0, Q + 1, n)
    codes[0] = Q
    yield SumCase("far from zero", as_type(1e12 + rng.uniform(0, 1e11, n), dt_f), *zip(_term(codes, dt_q, 2.0 ** 34, 0)))
    # 10. all negative
    rng = case(13)
    codes = rng.integers(0, Q + 1, n)
    codes[0] = 0
    yield SumCase("all negative", as_type(rng.uniform(-6, -3, n), dt_f), *zip(_term(codes, dt_q, np.float32(2.0 / Q), Q)))
    # 11. exact cancellation: m + (-m) = +0 at even places; -0 + (0 * -1) at odd places: -0 where the oracle gives it
    rng = case(14)
    m = rng.integers(1, Q + 1, n).astype(np.float64)
    m[1::2] = 0
    a = m.copy()
    a[1::2] = -0.0
    yield SumCase("exact cancellation", as_type(a, dt_f), *zip(_term(m, dt_q, -1.0, 0)))
    # 12. the order of the terms matters: (k + B) - B rounds k + B first (a tie for odd k: the ulp is 2 from B on), (k - B) + B and (B - B) + k do
    #     not.  A large acc with small terms would show the same, but min > 0 clamps the zero point to 0 and every code saturates; here the sum is
    #     0 .. Q, scale 1, and one unit of difference is one code.
    rng = case(15)
    k = rng.integers(0, Q + 1, n)
    k[0] = 1
    k[n // 2] = 3
    k[-1] = 1 if n == 1 else 0
    ones = np.ones(n)
    yield SumCase("order of the terms", as_type(k, dt_f), *zip(_term(ones, dt_q, ORDER_BIG[dt_f], 0), _term(ones, dt_q, -ORDER_BIG[dt_f], 0)))


def count_case(n, dt_f, dt_q, K, seed=0):
    """an ordinary accumulator and K ordinary terms, each with its own record"""
    rng = _rng(n, dt_f, dt_q, K, 77, seed)
    acc = ordinary_acc(rng, n, dt_f)
    terms = [ordinary_term(rng, n, dt_q, i) for i in range(K)]
    return SumCase(f"{K} ordinary terms", acc, [t[0] for t in terms], [t[1] for t in terms])


def tie_case(n, dt_q, K):
    """bfloat16: acc at integers of both signs whose ulp is 2 (256..511) and 4 (512..1023), K terms of record (1.0, 0) with codes 0..qmax: every
    odd code lands exactly between two bfloat16 values, with even and odd neighbours, so rounding after every term differs from rounding once"""
    Q = M.QMAX[dt_q]
    rng = _rng(n, dt_q, K, 31)
    acc = np.where(np.arange(n) % 2 == 0, 256 + 2 * rng.integers(0, 128, n), 512 + 4 * rng.integers(0, 128, n))
    acc = np.where(np.arange(n) // 2 % 2 == 0, acc, -acc)   # both signs: the sum straddles zero, so the quantizer resolves it
    terms = [_term((np.arange(n) // 2 + 1 + 2 * t) % (Q + 1), dt_q, 1.0, 0) for t in range(K)]
    return SumCase(f"bfloat16 ties, {K} terms", as_type(acc, BF16), [t[0] for t in terms], [t[1] for t in terms])


def padded(case, dt_q, K):
    """the case with terms that add exactly +0 (code 1 - zero point 1) behind its own, K terms in all: more than one launch's worth"""
    q, rec = _term(np.ones(case.acc.size), dt_q, 1.0, 1)
    extra = K - len(case.terms)
    assert extra > 0
    return SumCase(f"{case.name}, {K} terms", case.acc, list(case.terms) + [q] * extra, list(case.records) + [rec] * extra)


# ---- records no quantize call writes

RECORD_SCALES = [("0", 0.0), ("-0", -0.0), ("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("negative", -0.75), ("smallest denormal", 2.0 ** -149),
                 ("reciprocal is denormal", 3e38), ("FLT_MAX", FLT_MAX)]
RECORD_ACCS = [0.0, -0.0, 1.0, np.inf, np.nan]
RECORD_N = 16    # 5 accumulators x 3 codes and one more element: whole vectors of both float types


def record_zero_points(dt_q):
    Q = M.QMAX[dt_q]
    return [0, Q, -1, Q + 1, 1 << 31, -(1 << 31), (1 << 63) - 1, -(1 << 63)]


def record_cases(dt_f, dt_q):
    """-> (name, acc, packed codes, record) for every scale x zero point: element 3 a + c has accumulator RECORD_ACCS[a] and code (0, 1, qmax)[c]"""
    Q = M.QMAX[dt_q]
    codes = np.array([c for _ in RECORD_ACCS for c in (0, 1, Q)] + [0], dtype=np.uint8)
    acc = as_type(np.array([a for a in RECORD_ACCS for _ in range(3)] + [0.5], dtype=np.float32), dt_f)
    assert codes.size == acc.size == RECORD_N
    for sname, scale in RECORD_SCALES:
        for zp in record_zero_points(dt_q):
            yield f"scale {sname}, zero point {zp}", acc, M.pack(codes, dt_q), M.record(scale, zp)


# ---- batches

def batch_sizes(count):
    """member sizes with empty members at the first, a middle and the last position (from three members on)"""
    cycle = [4096, 4099, 8, 1, 1000, 2049, 3072, 7]
    sizes = [cycle[i % len(cycle)] + (i // len(cycle)) for i in range(count)]
    if count == 2:
        sizes[0] = 0
    if count >= 3:
        sizes[0] = sizes[count // 2] = sizes[-1] = 0
    return sizes


def batch_members(count, dt_f):
    """ordinary members, each with its own range"""
    rng = _rng(count, dt_f, 5)
    return [as_type(rng.uniform(-1 - 0.1 * i, 2 + 0.2 * i, n), dt_f) for i, n in enumerate(batch_sizes(count))]


def edge_batch(n, dt_f):
    """16 different members for one launch: the edge cases of the single-tensor call (test_gpu_parity._dynamic_cases), an all-NaN member, and
    ordinary members between them -> [(name, x)]"""
    from test_gpu_parity import _dynamic_cases

    rng = _rng(n, dt_f, 404)
    edges = [(name, as_type(x, dt_f)) for name, x in _dynamic_cases(rng, n)]
    assert [e[0] for e in edges][:3] == ["uniform", "nan", "constant"] and len(edges) == 12

    def ordinary(i):
        return f"ordinary {i}", as_type(rng.uniform(-1 - i, 1 + 2 * i, n), dt_f)

    nan = ("all nan", as_type(np.full(n, np.nan), dt_f))
    members = edges[:2] + [ordinary(0), edges[2], ordinary(1)] + edges[3:7] + [nan] + edges[7:] + [ordinary(2)]
    assert len(members) == 16 and members[3][0] == "constant" and members[9][0] == "all nan"
    return members


# ---- the one-launch reduce's deal of rounds to blocks, restated (csrc/fused_kernels.hpp fused_first_round, csrc/kernels.hip fused_blocks_per_group)

FUSED_BLOCK = 1024       # kFusedBlock: one round is 1024 threads x one 16-byte vector
FUSED_MIN_ROUNDS = 2     # kFusedMinRounds
HAND_OVER_VECS = 7 * FUSED_BLOCK   # more than 3 x 2048 vectors: four blocks of 1, 2, 2, 2 rounds


def fused_share_begins(n_vec, cap=256):
    """first vector of every block's share"""
    rounds = -(-n_vec // FUSED_BLOCK)
    G = min(cap, max(-(-n_vec // (FUSED_BLOCK * FUSED_MIN_ROUNDS)), 1))
    return [b * rounds // G * FUSED_BLOCK for b in range(G)]


def hand_over_cases(dt_f, dt_q):
    """more than one block: under hand-over the last block adopts the others' shares and recomputes their terms and threshold keys"""
    n = HAND_OVER_VECS * EPV[dt_f]
    yield count_case(n, dt_f, dt_q, 2, seed=1)
    if dt_f == BF16:
        yield tie_case(n, dt_q, 3)
