"""GPU: the four device calls that carry the per-chunk wire -- quantize_dynamic_batch, reduce_quantize_dynamic, dequantize_sum and
dequantize_dynamic_batch -- at the edges that uniform data never reaches, bit for bit against a model made of the oracle alone
(tests/dynamic_wire_model.py) on the inputs of tests/dynamic_wire_cases.py (tests/test_dynamic_wire_cases_cpu.py proves that those inputs tell
thirteen wrong kernels from the right one).

  a  the reduce on every sum case, term count and rounding mode, through every path of its host code; which path ran is asserted: the one-launch
     form leaves the accumulator bit-identical, the two-step form leaves the model's sum in it
  b  dequantize_sum and dequantize_dynamic_batch on records no quantize call writes, on bfloat16 ties and on every term / member count
  c  the capacity edges of the one-launch reduce (10 | 11 and 19 | 20 rounds) and of a batch member (18 | 19, 27 | 28, 64 | 65 rounds), sizes from
     the device's CU count
  d  quantize_dynamic_batch with one edge case per member
  e  quantized_all_reduce on a one-rank RCCL group over the per-chunk wire

No tolerances: bytes and records are compared exactly (scales by bit pattern), floats with same_floats (any NaN equals any NaN)."""
import os
import socket

import numpy as np
import pytest

import dynamic_wire_cases as C
import dynamic_wire_model as M
import oracle as O
from helpers import same_floats

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAIR_IDS = ["f32-u8", "f32-u4", "f32-u2", "bf16-u8", "bf16-u4", "bf16-u2"]
ELEMENT = M.per_element(C.SEED, C.INDEX_BASE)


def new_context():
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context()
    c.set_reference_layout(False)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_blocking(False)
    return c


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    return new_context()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def DT(code):
    import piquant

    return piquant.DataType(code)


def OP(code):
    import piquant

    return piquant.ReduceOp(code)


def set_round(ctx, round):
    """-> the RoundMode of the call, with the context's stochastic state set for `round`"""
    import piquant

    if round[0] == "element":
        ctx.set_stochastic_threshold(None)
        ctx.set_stochastic_per_element(True, seed=round[1], index_base=round[2])
    else:
        ctx.set_stochastic_per_element(False)
        ctx.set_stochastic_threshold(round[1] if round[0] == "call" else None)
    return piquant.RoundMode(O.NEAREST if round[0] == "nearest" else O.STOCHASTIC)


class Buf:
    """`data` in device memory, `offset` bytes behind a 64-byte boundary, with 64 guard bytes of 0xAA on both sides"""

    def __init__(self, data, offset=0):
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.n, self.lo = raw.size, 64 + offset
        host = np.full(self.lo + self.n + 64, 0xAA, dtype=np.uint8)
        host[self.lo: self.lo + self.n] = raw
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 64 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def read(self, dtype=np.uint8):
        host = self.t.cpu().numpy()
        assert (host[: self.lo] == 0xAA).all(), "the call wrote in front of the buffer"
        assert (host[self.lo + self.n:] == 0xAA).all(), "the call wrote behind the buffer"
        return host[self.lo: self.lo + self.n].copy().view(dtype)


def fresh_out(n, dt_q):
    return Buf(np.full(O.packed_numel(n, dt_q), 0x55, dtype=np.uint8))


def assert_record(got_bytes, want, what):
    """the whole record: scale by bit pattern, 1 / scale as the float32 quotient, zero point"""
    scale, inv, zp = M.read_record(got_bytes.tobytes())
    assert M.same_record((scale, zp), want), f"{what}: record ({scale!r}, {zp}), want {want}"
    assert np.float32(inv).tobytes() == np.frombuffer(M.record(want[0], want[1]), dtype=np.float32)[1].tobytes(), f"{what}: 1 / scale is {inv!r}"


# ---------------------------------------------------------------------------------------------------
# a. the reduce
# ---------------------------------------------------------------------------------------------------
PATHS = ("one launch", "fusion off", "reference layout", "acc off by one element", "out off by one byte", "a term off by one byte")


class ReduceRunner:
    """runs reduce_quantize_dynamic on a case; read-only term buffers are kept per case"""

    def __init__(self, ctx, case, dt_f, dt_q):
        self.ctx, self.case, self.dt_f, self.dt_q = ctx, case, dt_f, dt_q
        self.kept = {}

    def dev(self, arr, offset=0):
        key = (id(arr), offset)
        if key not in self.kept:
            self.kept[key] = Buf(np.frombuffer(arr, dtype=np.uint8) if isinstance(arr, bytes) else arr, offset)
        return self.kept[key]

    def run(self, round, path="one launch"):
        """-> (bytes, record bytes, acc afterwards)"""
        ctx, case, dt_f, dt_q = self.ctx, self.case, self.dt_f, self.dt_q
        n = case.acc.size
        acc = Buf(case.acc, C.ESIZE[dt_f] if path == "acc off by one element" else 0)
        out = Buf(np.full(O.packed_numel(n, dt_q), 0x55, dtype=np.uint8), 1 if path == "out off by one byte" else 0)
        rec = Buf(np.zeros(16, dtype=np.uint8))
        off_term = len(case.terms) // 2 if path == "a term off by one byte" else -1
        terms = [self.dev(q, 1 if i == off_term else 0) for i, q in enumerate(case.terms)]
        records = [self.dev(r) for r in case.records]
        rm = set_round(ctx, round)
        ctx.set_fusion(path != "fusion off")
        ctx.set_reference_layout(path == "reference layout")
        try:
            ctx.reduce_quantize_dynamic_ptr(acc.ptr, DT(dt_f), [t.ptr for t in terms], [r.ptr for r in records], out.ptr, DT(dt_q), n, rec.ptr, rm, _device_ptrs=True)
        finally:
            ctx.set_fusion(True)
            ctx.set_reference_layout(False)
        return out.read(), rec.read(), acc.read(M.NP_OF[dt_f])


def takes_one_launch(case, dt_f, path):
    """launch_fused_reduce_quantize's conditions (csrc/kernels.hip), for tensors far below the chip's capacity"""
    return path == "one launch" and case.acc.size % C.EPV[dt_f] == 0 and 1 <= len(case.terms) <= 16


def check_reduce(got, want, case, dt_f, one_launch, what):
    q, rec, acc_after = got
    want_q, want_p, want_sum = want
    assert_record(rec, want_p, what)
    assert np.array_equal(q, want_q), f"{what}: {np.count_nonzero(q != want_q)} of {q.size} bytes differ, first at {np.flatnonzero(q != want_q)[:4]}"
    if not case.terms:
        assert np.array_equal(acc_after.view(np.uint8), case.acc.view(np.uint8)), f"{what}: nothing to add, yet the accumulator changed"
    elif one_launch:
        assert np.array_equal(acc_after.view(np.uint8), case.acc.view(np.uint8)), f"{what}: the one-launch form leaves the accumulator alone: the two-step form ran"
    else:
        assert same_floats(acc_after, want_sum), f"{what}: the two-step form leaves the sum in the accumulator: the one-launch form ran, or the sum is wrong"


def reduce_cases(n, dt_f, dt_q):
    """-> [(case, paths)]"""
    sums = list(C.sum_cases(n, dt_f, dt_q))
    out = [(c, PATHS) for c in sums]
    out += [(C.padded(c, dt_q, K), PATHS[:1]) for c in sums for K in (17, 33)]
    out += [(C.count_case(n, dt_f, dt_q, K), PATHS[:2]) for K in C.REDUCE_COUNTS]
    if dt_f == O.BF16:
        out += [(C.tie_case(n, dt_q, K), PATHS) for K in (1, 2, 3)]
    return out


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_reduce_every_case_round_mode_and_path(ctx, dt_f, dt_q, n):
    ran = {True: 0, False: 0}
    for case, paths in reduce_cases(n, dt_f, dt_q):
        runner = ReduceRunner(ctx, case, dt_f, dt_q)
        for rname, round in C.ROUNDS:
            want = M.reduce_quantize(O, case.acc, case.terms, case.records, dt_q, dt_f, round)
            for path in paths:
                one = takes_one_launch(case, dt_f, path)
                check_reduce(runner.run(round, path), want, case, dt_f, one, f"{case.name}, {n} elements, {rname}, path '{path}'")
                ran[one] += 1
    assert ran[False] > 0 and (ran[True] > 0) == (n % C.EPV[dt_f] == 0)
    assert ctx.barrier_bailouts() == 0


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_reduce_term_records_no_quantize_call_writes(ctx, dt_f, dt_q):
    """the term loop of the one-launch form and of the two-step form on scale 0, -0, +-inf, NaN, negative, denormal, ... and zero points outside
    [0, qmax], up to the ends of int64"""
    for name, acc, q, rec in C.record_cases(dt_f, dt_q):
        case = C.SumCase(name, acc, [q], [rec])
        want = M.reduce_quantize(O, acc, [q], [rec], dt_q, dt_f, M.NEAREST)
        runner = ReduceRunner(ctx, case, dt_f, dt_q)
        for path in PATHS[:2]:
            check_reduce(runner.run(M.NEAREST, path), want, case, dt_f, path == "one launch", f"term record with {name}, path '{path}'")


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_reduce_hands_over_with_per_element_thresholds_and_ties(dt_f, dt_q):
    """four blocks, all but the last hand their share over at once (the deterministic hook): the adopting block recomputes the terms of the shares
    it picks up and their threshold keys"""
    ctx = new_context()
    for case in C.hand_over_cases(dt_f, dt_q):
        runner = ReduceRunner(ctx, case, dt_f, dt_q)
        for rname, round in (C.ROUNDS[2], C.ROUNDS[0]):
            want = M.reduce_quantize(O, case.acc, case.terms, case.records, dt_q, dt_f, round)
            check_reduce(runner.run(round), want, case, dt_f, True, f"{case.name}, {rname}, no hand-over")
            ctx.set_barrier_timeout_us(ctx.HAND_OVER_ALWAYS)
            before = ctx.barrier_bailouts()
            try:
                got = runner.run(round)
            finally:
                ctx.set_barrier_timeout_us(0)
            handed = ctx.barrier_bailouts() - before
            check_reduce(got, want, case, dt_f, True, f"{case.name}, {rname}, every block but the last handing over")
            assert handed == len(C.fused_share_begins(C.HAND_OVER_VECS)) - 1 == 3, handed


# ---------------------------------------------------------------------------------------------------
# b. dequantize_sum and dequantize_dynamic_batch
# ---------------------------------------------------------------------------------------------------
ALIGNMENTS = (("aligned", 0, 0), ("out off by one element", 1, 0), ("inputs off by one byte", 0, 1))


def run_dequantize_sum(ctx, terms, records, dt_q, dt_f, n, op, prev, out_off, in_off, kept):
    def dev(arr, offset=0):
        key = (id(arr), offset)
        if key not in kept:
            kept[key] = Buf(np.frombuffer(arr, dtype=np.uint8) if isinstance(arr, bytes) else arr, offset)
        return kept[key]

    out = Buf(prev, out_off * C.ESIZE[dt_f])
    ctx.dequantize_sum_ptr([dev(q, in_off).ptr for q in terms], [dev(r).ptr for r in records], DT(dt_q), out.ptr, DT(dt_f), n, OP(op), _device_ptrs=True)
    return out.read(M.NP_OF[dt_f])


@pytest.mark.parametrize("op", [O.SET, O.ADD], ids=["set", "add"])
@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_dequantize_sum_records_ties_and_counts(ctx, dt_f, dt_q, op):
    jobs = [(f"record with {name}", acc, [q], [rec]) for name, acc, q, rec in C.record_cases(dt_f, dt_q)]
    for n in C.SIZES:
        jobs += [(f"{c.name}, {n} elements", c.acc, c.terms, c.records) for c in (C.count_case(n, dt_f, dt_q, K) for K in C.SUM_COUNTS)]
        if dt_f == O.BF16:
            jobs += [(f"{c.name}, {n} elements", c.acc, c.terms, c.records) for c in (C.tie_case(n, dt_q, K) for K in (1, 2, 3))]
    for what, prev, terms, records in jobs:
        want = M.dequantize_sum(O, terms, records, dt_q, dt_f, prev.size, op, prev)
        kept = {}
        for aname, out_off, in_off in ALIGNMENTS:
            got = run_dequantize_sum(ctx, terms, records, dt_q, dt_f, prev.size, op, prev, out_off, in_off, kept)
            assert same_floats(got, want), f"dequantize_sum {what}, {aname}: elements {np.flatnonzero(got.view(M.NP_OF[dt_f]) != want)[:6]} differ"


def decode_members(dt_f, dt_q):
    """members of the batched decode: every record case, the bfloat16 ties at every size, a member of more than one tile -> [(name, prev, q, rec)]"""
    members = [(f"record with {name}", acc, q, rec) for name, acc, q, rec in C.record_cases(dt_f, dt_q)]
    for n in C.SIZES + (12291,):
        c = C.tie_case(n, dt_q, 1) if dt_f == O.BF16 else C.count_case(n, dt_f, dt_q, 1)
        members.append((f"{c.name}, {n} elements", c.acc, c.terms[0], c.records[0]))
    return members


@pytest.mark.parametrize("op", [O.SET, O.ADD], ids=["set", "add"])
@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_dequantize_dynamic_batch_records_ties_and_member_counts(ctx, dt_f, dt_q, op):
    """launches of 1, 2, 16, 17 and 33 members, with empty members at the first, a middle and the last position"""
    members = decode_members(dt_f, dt_q)
    for aname, out_off, in_off in ALIGNMENTS:
        at, launch = 0, 0
        while at < len(members):
            count = C.BATCH_COUNTS[launch % len(C.BATCH_COUNTS)]
            launch += 1
            empty = {0, count // 2, count - 1} if count >= 3 else ({0} if count == 2 else set())
            slots, bufs = [], []
            for i in range(count):
                if i in empty or at >= len(members):
                    slots.append(None)
                    continue
                name, prev, q, rec = members[at]
                at += 1
                bufs.append((name, prev, q, rec, Buf(q, in_off), Buf(np.frombuffer(rec, dtype=np.uint8)), Buf(prev, out_off * C.ESIZE[dt_f])))
                slots.append(bufs[-1])
            ctx.dequantize_dp_batch_ptr([s[4].ptr if s else 0 for s in slots], DT(dt_q), [s[6].ptr if s else 0 for s in slots], DT(dt_f), [s[1].size if s else 0 for s in slots],
                                        [s[5].ptr if s else 0 for s in slots], OP(op), _device_ptrs=True)
            for name, prev, q, rec, _, _, out in bufs:
                want = M.dequantize_sum(O, [q], [rec], dt_q, dt_f, prev.size, op, prev)
                assert same_floats(out.read(M.NP_OF[dt_f]), want), f"dequantize_dynamic_batch of {count} members, {aname}: {name}"
        assert launch >= len(C.BATCH_COUNTS)


# ---------------------------------------------------------------------------------------------------
# quantize_dynamic_batch: member counts, per-element thresholds, edge data (d)
# ---------------------------------------------------------------------------------------------------
def run_batch(ctx, xs, dt_f, dt_q, round):
    """-> [(bytes, record bytes)] per member"""
    ins = [Buf(x) if x.size else None for x in xs]
    outs = [fresh_out(x.size, dt_q) if x.size else None for x in xs]
    recs = Buf(np.zeros(16 * len(xs), dtype=np.uint8))
    rm = set_round(ctx, round)
    ctx.quantize_dynamic_batch_ptr([b.ptr if b else 0 for b in ins], DT(dt_f), [b.ptr if b else 0 for b in outs], DT(dt_q), [x.size for x in xs],
                                   [recs.ptr + 16 * i for i in range(len(xs))], rm, _device_ptrs=True)
    r = recs.read()
    return [(o.read() if o else np.zeros(0, dtype=np.uint8), r[16 * i: 16 * i + 16]) for i, o in enumerate(outs)]


def check_batch(got, want, what, names=None):
    for i, ((q, rec), (want_q, want_p)) in enumerate(zip(got, want)):
        w = f"{what}, member {i}" + (f" ({names[i]})" if names else "")
        assert_record(rec, want_p, w)
        assert np.array_equal(q, want_q), f"{w}: {np.count_nonzero(q != want_q)} of {q.size} bytes differ"


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_batch_member_counts_empty_members_and_per_element_thresholds(ctx, dt_f, dt_q):
    """every member counts its elements from index_base + 0, in one launch (up to 16 members), over two or three launches and when fusion is off"""
    for count in C.BATCH_COUNTS:
        xs = C.batch_members(count, dt_f)
        for rname, round in C.ROUNDS:
            want = M.quantize_batch(O, xs, dt_f, dt_q, round)
            check_batch(run_batch(ctx, xs, dt_f, dt_q, round), want, f"batch of {count}, {rname}")
            ctx.set_fusion(False)
            try:
                got = run_batch(ctx, xs, dt_f, dt_q, round)
            finally:
                ctx.set_fusion(True)
            check_batch(got, want, f"batch of {count}, {rname}, single calls")
    assert ctx.barrier_bailouts() == 0


@pytest.mark.parametrize("n", [4096, 4099, 999])
@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_batch_with_one_edge_case_per_member(ctx, dt_f, dt_q, n):
    """NaN, constant, infinities, +-FLT_MAX, denormals, an all-NaN member ... next to ordinary members in ONE launch: no member's NaN, inf or
    degenerate record leaks into its neighbours' sub-grids; each equals the model and quantize_dynamic of that member alone"""
    members = C.edge_batch(n, dt_f)
    names, xs = [m[0] for m in members], [m[1] for m in members]
    want = M.quantize_batch(O, xs, dt_f, dt_q, M.NEAREST)
    got = run_batch(ctx, xs, dt_f, dt_q, M.NEAREST)
    check_batch(got, want, f"edge batch of {n}-element members", names)
    rm = set_round(ctx, M.NEAREST)
    for i, x in enumerate(xs):
        a, out, rec = Buf(x), fresh_out(n, dt_q), Buf(np.zeros(16, dtype=np.uint8))
        ctx.quantize_dynamic_ptr(a.ptr, DT(dt_f), out.ptr, DT(dt_q), n, rec.ptr, rm, _device_ptrs=True)
        assert np.array_equal(out.read(), got[i][0]) and np.array_equal(rec.read(), got[i][1]), f"member {i} ({names[i]}) differs from the single call"


# ---------------------------------------------------------------------------------------------------
# c. capacity edges
# ---------------------------------------------------------------------------------------------------
# restated from csrc/tuning.hpp and csrc/kernels.hip (fused_blocks_per_group, fused_rounds)
K_FUSED_BLOCK = 1024              # kFusedBlock
K_FUSED_MAX_BLOCKS = 256          # kFusedMaxBlocks
K_FUSED_REG_ROUNDS = 18           # kFusedRegRounds
K_FUSED_LDS_ROUNDS = 9            # kFusedLdsRounds
K_FUSED_MAX_ROUNDS = 64           # kFusedMaxRounds
K_FUSED_REDUCE_REG_ROUNDS = 10    # kFusedReduceRegRounds
K_FUSED_MIN_ROUNDS = 2            # kFusedMinRounds


def fused_rounds(n_vec, G):
    return -(-(-(-n_vec // K_FUSED_BLOCK)) // G)


def fused_blocks_per_group(numel, dt_f, count, cus):
    """0: the launch is refused"""
    n_vec = -(-numel // C.EPV[dt_f])
    cap = min(cus // count, K_FUSED_MAX_BLOCKS)
    if cap < 1 or fused_rounds(n_vec, cap) > K_FUSED_MAX_ROUNDS:
        return 0
    return min(cap, max(-(-n_vec // (K_FUSED_BLOCK * K_FUSED_MIN_ROUNDS)), 1))


def uniform_f32(rng, n, lo, hi):
    x = rng.random(n, dtype=np.float32)
    x *= np.float32(hi - lo)
    x += np.float32(lo)
    return x


@pytest.mark.parametrize("dt_f,R,more,round", [(O.F32, 10, 0, M.NEAREST), (O.F32, 10, 1, M.NEAREST), (O.F32, 19, 0, M.NEAREST), (O.F32, 19, 1, M.NEAREST),
                                               (O.BF16, 19, 0, M.NEAREST), (O.BF16, 19, 1, M.NEAREST), (O.F32, 19, 0, ELEMENT)],
                         ids=["f32-10", "f32-10+1", "f32-19", "f32-19+1", "bf16-19", "bf16-19+1", "f32-19-per-element"])
def test_reduce_capacity_edge(ctx, cus, dt_f, R, more, round):
    """R rounds per block and one vector more: 10 | 11 is the first LDS-resident round (kFusedReduceRegRounds), 19 | 20 the last size the one-launch
    form takes (+ kFusedLdsRounds).  One uint8 term; the one minimum of the sum in the last round of the last block, the one maximum in a block's
    eleventh round (its last, where it has ten)"""
    Cb = min(cus, K_FUSED_MAX_BLOCKS)
    epv = C.EPV[dt_f]
    n = (R * K_FUSED_BLOCK * Cb + more) * epv
    G = fused_blocks_per_group(n, dt_f, 1, cus)
    assert G == Cb and fused_rounds(n // epv, G) == R + more
    one_launch = R + more <= K_FUSED_REDUCE_REG_ROUNDS + K_FUSED_LDS_ROUNDS
    assert one_launch == (not (R == 19 and more))
    rng = np.random.default_rng([R, more, dt_f])
    a = uniform_f32(rng, n, -1, 1)
    codes = rng.integers(0, 256, n, dtype=np.uint8)
    lo = n - 3                                                                          # the last vector: the last round of the last block
    hi = (((Cb // 2) * R + min(10, R - 1)) * K_FUSED_BLOCK + 517) * epv + 1            # block Cb / 2, round index 10 (or R - 1)
    a[lo], codes[lo] = -1.5, 0
    a[hi], codes[hi] = 1.5, 255
    case = C.SumCase(f"{R} rounds + {more} vector(s)", C.as_type(a, dt_f), [codes], [M.record(1.0 / 64, 128)])
    del a
    want = M.reduce_quantize(O, case.acc, case.terms, case.records, O.UINT8, dt_f, round)
    y = C.as_f32(want[2], dt_f)
    assert int(np.argmin(y)) == lo and int(np.argmax(y)) == hi and (y == y[lo]).sum() == 1 and (y == y[hi]).sum() == 1
    got = ReduceRunner(ctx, case, dt_f, O.UINT8).run(round)
    check_reduce(got, want, case, dt_f, one_launch, f"reduce of {n} elements ({R} rounds + {more} vector)")
    assert ctx.barrier_bailouts() == 0


BATCH_EDGES = [(dt_f, dt_q, R, more, M.NEAREST) for dt_f, dt_q in ((O.F32, O.UINT8), (O.BF16, O.UINT4)) for R in (18, 27, 64) for more in (0, 1)]
BATCH_EDGES += [(dt_f, dt_q, R, 0, ELEMENT) for dt_f, dt_q in ((O.F32, O.UINT8), (O.BF16, O.UINT4)) for R in (27, 64)]


@pytest.mark.parametrize("dt_f,dt_q,R,more,round", BATCH_EDGES,
                         ids=[f"{'f32-u8' if e[0] == O.F32 else 'bf16-u4'}-{e[2]}{'+1' if e[3] else ''}{'-per-element' if e[4] is ELEMENT else ''}" for e in BATCH_EDGES])
def test_batch_capacity_edge(ctx, cus, dt_f, dt_q, R, more, round):
    """16 members share the chip: a sub-grid is CUs / 16 blocks.  15 members of 1000 to 5000 elements and one of R rounds per block of its sub-grid
    (and one vector more): 18 | 19 register -> LDS (kFusedRegRounds), 27 | 28 LDS -> streamed (+ kFusedLdsRounds), 64 the last size the one-launch
    form takes (kFusedMaxRounds), 65 refused: every member goes through single calls.  The large member's minimum sits in its last vector (streamed
    from 28 rounds on)"""
    G = min(cus // 16, K_FUSED_MAX_BLOCKS)
    epv = C.EPV[dt_f]
    n = (R * K_FUSED_BLOCK * G + more) * epv
    assert (fused_blocks_per_group(n, dt_f, 16, cus) == G) == (R + more <= K_FUSED_MAX_ROUNDS) and (R + more > K_FUSED_MAX_ROUNDS) == (fused_blocks_per_group(n, dt_f, 16, cus) == 0)
    rng = np.random.default_rng([R, more, dt_f, 16])
    big = uniform_f32(rng, n, -1, 1)
    big[n - 2] = -1.75
    big[n // 3] = 1.25
    sizes = [int(s) for s in rng.integers(1000, 5001, 15)]
    xs = [C.as_type(rng.uniform(-1 - 0.1 * i, 2 + 0.2 * i, s), dt_f) for i, s in enumerate(sizes)]
    xs.insert(5, C.as_type(big, dt_f))
    want = M.quantize_batch(O, xs, dt_f, dt_q, round)
    check_batch(run_batch(ctx, xs, dt_f, dt_q, round), want, f"batch with a member of {R} rounds + {more} vector")
    assert ctx.barrier_bailouts() == 0


# ---------------------------------------------------------------------------------------------------
# e. the wire end to end, one process
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pg():
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_all_reduce_over_the_per_chunk_wire_on_edge_tensors(pg, oracle_mod, dt_f, dt_q, algorithm):
    """quantized_all_reduce(group_size=None) on a one-rank RCCL group (the hook that runs the whole schedule with the rank as its own only peer):
    the tensor is the sum of a sum case -- NaN among finite values, one +inf, constant, all NaN -- and comes back as dequantize(quantize(x)) with
    the model's record.  With one rank the tensor is one chunk: 4099 elements make it ragged, 4096 whole"""
    import piquant.distributed as D

    qdtype = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}[dt_q]
    for n in (4099, 4096):
        sums = {c.name: M.reduce_quantize(O, c.acc, c.terms, c.records, dt_q, dt_f, M.NEAREST)[2] for c in C.sum_cases(n, dt_f, dt_q)}
        for name in ("nan where inf meets -inf", "plus inf", "constant", "all nan"):
            x = sums[name]
            q, (scale, zp) = M.quantize_dynamic(O, x, dt_f, dt_q, M.NEAREST)
            want = O.dequantize(q, dt_q, dt_f, n, scale, zp)
            t = torch.from_numpy(x.copy()).cuda() if dt_f == O.F32 else torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.bfloat16)
            D.quantized_all_reduce(t, quant_dtype=qdtype, algorithm=algorithm, _single_rank_collectives=True)
            torch.cuda.synchronize()
            got = t.cpu().numpy() if dt_f == O.F32 else t.view(torch.int16).cpu().numpy().view(np.uint16)
            assert same_floats(got, want), f"all-reduce ({algorithm}) of '{name}', {n} elements"


@pytest.mark.parametrize("dt_f,dt_q", C.PAIRS, ids=PAIR_IDS)
def test_wire_ops_on_an_empty_chunk(ctx, dt_f, dt_q):
    """More ranks than 4096-element blocks leave chunks of the ring empty (ring_chunks(4099, 3) is 4096, 3 and 0 elements): on the per-chunk wire such
    a chunk is its 16-byte record alone.  The wire's device ops on it, as the schedules call them: every encode writes the degenerate record and
    nothing else, every decode writes nothing"""
    import piquant.distributed as D

    assert D.ring_chunks(4099, 3, M.BITS[dt_q])[-1] == (4099, 4099)
    ops = D._DeviceOps(ctx)
    tdt = torch.float32 if dt_f == O.F32 else torch.bfloat16
    qdtype = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}[dt_q]
    empty = torch.empty(0, dtype=tdt, device="cuda")
    degenerate = np.frombuffer(M.record(1.0, M.QMAX[dt_q] >> 1), dtype=np.uint8)
    x = C.ordinary_acc(np.random.default_rng(3), 1000, dt_f)
    xd = torch.from_numpy(x).cuda() if dt_f == O.F32 else torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16)
    guarded = torch.full((4, 48), 0xAA, dtype=torch.uint8, device="cuda")
    full = torch.full((16 + O.packed_numel(1000, dt_q) + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    ops.encode(empty, guarded[0, 16:32], qdtype, "nearest")
    ops.reduce_encode([guarded[0, 16:32]], empty, guarded[1, 16:32], qdtype, "nearest")
    ops.encode_batch([empty, xd, empty], [guarded[2, 16:32], full[:-16], guarded[3, 16:32]], qdtype, "nearest")
    ops.decode(guarded[0, 16:32], empty, qdtype, "set")
    ops.decode_sum([guarded[1, 16:32]], empty, qdtype)
    ops.decode_batch([guarded[2, 16:32], guarded[3, 16:32]], [empty, empty], qdtype, "add")
    torch.cuda.synchronize()
    got = guarded.cpu().numpy()
    for row in got:
        assert np.array_equal(row[16:32], degenerate) and (row[:16] == 0xAA).all() and (row[32:] == 0xAA).all()
    q, p = M.quantize_dynamic(O, x, dt_f, dt_q, M.NEAREST)
    f = full.cpu().numpy()
    assert_record(f[:16], p, "the member between two empty ones")
    assert np.array_equal(f[16:-16], q) and (f[-16:] == 0xAA).all()
