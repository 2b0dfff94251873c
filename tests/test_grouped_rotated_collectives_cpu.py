"""CPU: the two steps of a grouped collective in the rotated domain (tests/grouped_rotated_sim.py: the model of
piquant_hip_reduce_quantize_grouped_rotated / _dequantize_sum_grouped_rotated) -- what the definition is and what it is not -- and
piquant.distributed's four collectives with rotation_seed= over gloo, the wire ops coming from that model.
tests/test_gpu_grouped_rotated_reduce.py and tests/test_gpu_grouped_rotated_all_reduce.py hold the HIP kernels to the same model bit for bit."""
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks

SEED = 0x1234567887654321


def _models(oracle_mod):
    sys.path.insert(0, os.path.dirname(__file__))
    import grouped_model as GM
    import grouped_rotated_sim as S
    import rot_model as RM

    return oracle_mod, GM, RM, S


def _heavy(n, seed, O, dt):
    """heavy-tailed values: N(0, 1) with a 30 sigma element every 97"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    x[::97] *= 30.0
    return O.f32_to_bf16(x) if dt == O.BF16 else x


# the committed cases: (tensor type, quantized type, G, numel, terms); numel % G != 0 in all but the last
def _cases(O):
    return [(O.F32, O.UINT8, 128, 3 * 128 + 37, 2), (O.BF16, O.UINT4, 32, 7 * 32 + 5, 3), (O.F32, O.UINT4, 64, 4 * 64 + 63, 3),
            (O.BF16, O.UINT8, 256, 2 * 256 + 1, 2), (O.F32, O.UINT2, 32, 5 * 32, 2)]


def _terms(O, RM, dt, qd, G, n, k, base=500):
    return [RM.quantize_grouped_rotated(_heavy(n, base + i, O, dt), dt, qd, G, SEED) for i in range(k)]


def _u(O, dt):
    return np.uint16 if dt == O.BF16 else np.uint32


# ---- the definition ----

def test_no_terms_is_the_rotated_quantize(oracle_mod):
    O, GM, RM, S = _models(oracle_mod)
    for dt, qd, G, n, _ in _cases(O):
        acc = _heavy(n, 1, O, dt)
        for got, want in zip(S.reduce_quantize_grouped_rotated(acc, dt, [], qd, G, SEED), RM.quantize_grouped_rotated(acc, dt, qd, G, SEED)):
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_one_term_sum_is_the_rotated_dequantize(oracle_mod):
    O, GM, RM, S = _models(oracle_mod)
    for dt, qd, G, n, _ in _cases(O):
        (q, s, z), = _terms(O, RM, dt, qd, G, n, 1)
        prev = _heavy(n, 2, O, dt)
        for op, p in ((O.SET, None), (O.ADD, prev)):
            got = S.dequantize_sum_grouped_rotated([(q, s, z)], qd, dt, n, G, SEED, op, p)
            want = RM.dequantize_grouped_rotated(q, qd, dt, n, G, s, z, SEED, op, p)
            assert np.array_equal(got.view(_u(O, dt)), want.view(_u(O, dt)))


def test_the_ragged_group_is_not_rotated_but_receives_its_terms(oracle_mod):
    O, GM, RM, S = _models(oracle_mod)
    for dt, qd, G, n, k in _cases(O):
        full = n // G * G
        if full == n:
            continue
        acc, terms = _heavy(n, 3, O, dt), _terms(O, RM, dt, qd, G, n, k)
        # the ragged group of the sum: the widened accumulator's own values plus its terms, no rotation anywhere
        y = S.rotated_sum(acc, dt, terms, qd, G, SEED)
        tail = RM.widen(acc, dt)[full:]
        for q, s, z in terms:
            tail = GM.dequantize_grouped(q, qd, O.F32, n, G, s, z, O.ADD, prev=np.concatenate([np.zeros(full, np.float32), tail]))[full:]
        assert np.array_equal(y[full:].view(np.uint32), tail.view(np.uint32))
        assert not np.array_equal(y[full:], RM.widen(acc, dt)[full:])                       # the terms did arrive
        out = S.dequantize_sum_grouped_rotated(terms, qd, O.F32, n, G, SEED)
        assert np.array_equal(out[full:].view(np.uint32), S.terms_sum(terms, qd, n, G)[full:].view(np.uint32))


# ---- what the definition is not: every variant changes at least one byte on at least one committed case ----

def _reduce_variants(O, GM, RM, S):
    def deq_add(y, t, qd, G):
        return GM.dequantize_grouped(t[0], qd, O.F32, y.size, G, t[1], t[2], O.ADD, prev=y)

    def unrotated_acc(acc, dt, terms, qd, G):
        y = RM.widen(acc, dt)
        for t in terms:
            y = deq_add(y, t, qd, G)
        return y

    def rotate_the_sum(acc, dt, terms, qd, G):
        return RM.rotate(unrotated_acc(acc, dt, terms, qd, G), G, SEED)

    def bf16_running_sum(acc, dt, terms, qd, G):
        y = RM.rotate(RM.widen(acc, dt), G, SEED)
        for t in terms:
            y = deq_add(y, t, qd, G)
            if dt == O.BF16:
                y = O.bf16_to_f32(O.f32_to_bf16(y))
        return y

    def reverse_order(acc, dt, terms, qd, G):
        return S.rotated_sum(acc, dt, terms[::-1], qd, G, SEED)

    def ragged_rotated(acc, dt, terms, qd, G):
        x = RM.widen(acc, dt)
        pad = np.zeros(-(-x.size // G) * G, dtype=np.float32)
        pad[: x.size] = x
        y = RM.rotate(pad, G, SEED)[: x.size]
        for t in terms:
            y = deq_add(y, t, qd, G)
        return y

    def inverse_for_forward(acc, dt, terms, qd, G):
        y = RM.rotate(RM.widen(acc, dt), G, SEED, inverse=True)
        for t in terms:
            y = deq_add(y, t, qd, G)
        return y

    def float64_sum(acc, dt, terms, qd, G):
        y = RM.rotate(RM.widen(acc, dt), G, SEED).astype(np.float64)
        for q, s, z in terms:
            y = y + GM.dequantize_grouped(q, qd, O.F32, y.size, G, s, z).astype(np.float64)
        return y.astype(np.float32)

    return [unrotated_acc, rotate_the_sum, bf16_running_sum, reverse_order, ragged_rotated, inverse_for_forward, float64_sum]


def _sum_variants(O, GM, RM, S):
    def deq(t, qd, n, G):
        return GM.dequantize_grouped(t[0], qd, O.F32, n, G, t[1], t[2])

    def store(z, prev, dt):
        if prev is not None:
            z = RM.widen(prev, dt) + z
        return z if dt == O.F32 else O.f32_to_bf16(z)

    def each_term_rotated_back(terms, qd, dt, n, G, prev):
        z = RM.rotate(deq(terms[0], qd, n, G), G, SEED, inverse=True)
        for t in terms[1:]:
            z = z + RM.rotate(deq(t, qd, n, G), G, SEED, inverse=True)
        return store(z, prev, dt)

    def reverse_order(terms, qd, dt, n, G, prev):
        return S.dequantize_sum_grouped_rotated(terms[::-1], qd, dt, n, G, SEED, O.SET if prev is None else O.ADD, prev)

    def old_contents_before_the_rotation(terms, qd, dt, n, G, prev):
        s = S.terms_sum(terms, qd, n, G)
        if prev is not None:
            s = s + RM.widen(prev, dt)
        return store(RM.rotate(s, G, SEED, inverse=True), None, dt)

    def ragged_rotated(terms, qd, dt, n, G, prev):
        s = S.terms_sum(terms, qd, n, G)
        pad = np.zeros(-(-n // G) * G, dtype=np.float32)
        pad[:n] = s
        return store(RM.rotate(pad, G, SEED, inverse=True)[:n], prev, dt)

    def forward_for_inverse(terms, qd, dt, n, G, prev):
        return store(RM.rotate(S.terms_sum(terms, qd, n, G), G, SEED), prev, dt)

    def float64_sum(terms, qd, dt, n, G, prev):
        s = deq(terms[0], qd, n, G).astype(np.float64)
        for t in terms[1:]:
            s = s + deq(t, qd, n, G).astype(np.float64)
        return store(RM.rotate(s.astype(np.float32), G, SEED, inverse=True), prev, dt)

    return [each_term_rotated_back, reverse_order, old_contents_before_the_rotation, ragged_rotated, forward_for_inverse, float64_sum]


def test_wrong_variants_of_the_reduce_change_a_byte(oracle_mod):
    O, GM, RM, S = _models(oracle_mod)
    for variant in _reduce_variants(O, GM, RM, S):
        differs = False
        for dt, qd, G, n, k in _cases(O):
            assert k >= 2
            acc, terms = _heavy(n, 4, O, dt), _terms(O, RM, dt, qd, G, n, k)
            want = S.reduce_quantize_grouped_rotated(acc, dt, terms, qd, G, SEED)
            got = GM.quantize_grouped(variant(acc, dt, terms, qd, G), O.F32, qd, G)
            differs = differs or any(not np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
        assert differs, variant.__name__


def test_wrong_variants_of_the_sum_change_a_byte(oracle_mod):
    O, GM, RM, S = _models(oracle_mod)
    with np.errstate(over="ignore", invalid="ignore"):
        for variant in _sum_variants(O, GM, RM, S):
            differs = False
            for dt, qd, G, n, k in _cases(O):
                terms, prev = _terms(O, RM, dt, qd, G, n, k), _heavy(n, 5, O, dt)
                for p in (None, prev):
                    want = S.dequantize_sum_grouped_rotated(terms, qd, dt, n, G, SEED, O.SET if p is None else O.ADD, p)
                    differs = differs or not np.array_equal(variant(terms, qd, dt, n, G, p).view(_u(O, dt)), want.view(_u(O, dt)))
            assert differs, variant.__name__


def test_every_term_rotated_back_separately_differs_in_most_words(oracle_mod):
    """the variant the composition of today's calls would be: with two terms most float32 words of 32 768 differ from one rotation of the sum"""
    O, GM, RM, S = _models(oracle_mod)
    G, n = 128, 32_768
    terms = [RM.quantize_grouped_rotated(RM.outlier_data(G, n // G, 100 + r), O.F32, O.UINT4, G, SEED) for r in range(2)]
    want = S.dequantize_sum_grouped_rotated(terms, O.UINT4, O.F32, n, G, SEED)
    apart = sum(RM.rotate(GM.dequantize_grouped(q, O.UINT4, O.F32, n, G, s, z), G, SEED, inverse=True) for q, s, z in terms)
    differing = int(np.sum(apart.view(np.uint32) != want.view(np.uint32)))
    print("words that differ:", differing, "of", n)
    assert differing > n // 2


# ---- the schedules, through the _ops seam ----

QDTYPES = {"uint8": 8, "quint4x2": 4}
# (world, numel, tensor type, wire type): ragged last groups; 5_001 elements leave rank 2 of 3 an empty chunk
SCHEDULES = [(2, 12_345, "float32", "uint8"), (3, 20_001, "bfloat16", "quint4x2"), (3, 5_001, "float32", "quint4x2"), (2, 8_195, "bfloat16", "uint8")]
G = 128


def _inputs(O, world, numel, fdt):
    return [_heavy(numel, 300 + r, O, O.BF16 if fdt == "bfloat16" else O.F32) for r in range(world)]


class _Recorder:
    """an ops object that forwards to `inner` and records (method, where its tensors start in their storages, the seed if any)"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        target = getattr(self.inner, name)

        def call(*args):
            where = []
            for a in args:
                if isinstance(a, torch.Tensor):
                    where.append(a.storage_offset())
                elif isinstance(a, (list, tuple)):
                    where.append([t.storage_offset() for t in a])
            self.calls.append((name, where, args[-1] if name.endswith("_rotated") else None))
            return target(*args)

        return call


def _schedule_worker(rank, world, port, numel, fdt, qname):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import oracle as O
        import piquant.distributed as D
        from grouped_rotated_sim import GroupedRotatedOracleOps

        x = _inputs(O, world, numel, fdt)[rank]
        qdtype = getattr(torch, qname)

        def fresh():
            return torch.from_numpy(x.view(np.int16).copy()).view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy())

        def host(t):
            return t.view(torch.int16).numpy().view(np.uint16).copy() if fdt == "bfloat16" else t.numpy().copy()

        out, traces = {}, {}
        for name in ("ring", "direct"):
            ops, t = _Recorder(GroupedRotatedOracleOps()), fresh()
            D.quantized_all_reduce(t, quant_dtype=qdtype, algorithm=name, group_size=G, rotation_seed=SEED, _ops=ops)
            out[name], traces[name] = host(t), ops.calls
        ops, t = _Recorder(GroupedRotatedOracleOps()), fresh()
        D.quantized_reduce_scatter(t, quant_dtype=qdtype, group_size=G, rotation_seed=SEED, _ops=ops)
        out["scatter"], traces["scatter"] = host(t), ops.calls
        ops = _Recorder(GroupedRotatedOracleOps())
        D.quantized_all_gather(t, quant_dtype=qdtype, group_size=G, rotation_seed=SEED, _ops=ops)
        out["both"], traces["gather"] = host(t), ops.calls
        if fdt == "float32":   # rotation_seed=None next to no rotation_seed at all (the un-rotated stand-ins take float32 only)
            for key, kwargs in (("none", dict(rotation_seed=None)), ("absent", {})):
                calls = []
                for fn, extra in ((D.quantized_all_reduce, dict(algorithm="ring")), (D.quantized_all_reduce, dict(algorithm="direct")),
                                  (D.quantized_reduce_scatter, {}), (D.quantized_all_gather, {})):
                    ops = _Recorder(GroupedRotatedOracleOps())
                    fn(fresh(), quant_dtype=qdtype, group_size=G, _ops=ops, **extra, **kwargs)
                    calls.append(ops.calls)
                traces[key] = calls
        return out, traces
    finally:
        dist.destroy_process_group()


_RESULTS = {}


def _schedule_results(case):
    if case not in _RESULTS:   # the ranks run once per case; every test below reads the same results
        _RESULTS[case] = run_ranks(case[0], _schedule_worker, case[1:], timeout=240)
    return _RESULTS[case]


def _expected(oracle_mod, case):
    O, GM, RM, S = _models(oracle_mod)
    import piquant.distributed as D

    world, numel, fdt, qname = case
    bits = QDTYPES[qname]
    qd, dt = {8: O.UINT8, 4: O.UINT4}[bits], O.BF16 if fdt == "bfloat16" else O.F32
    chunks = D.ring_chunks(numel, world, bits)
    xs = _inputs(O, world, numel, fdt)
    want = {"ring": S.simulate_ring_rotated(xs, dt, qd, chunks, G, SEED), "direct": S.simulate_direct_rotated(xs, dt, qd, chunks, G, SEED),
            "scatter": S.simulate_reduce_scatter_rotated(xs, dt, qd, chunks, G, SEED)}
    want["both"] = S.simulate_all_gather_rotated(want["scatter"], dt, qd, chunks, G, SEED)
    return want, _u(O, dt), chunks


@pytest.mark.parametrize("case", SCHEDULES, ids=lambda c: "-".join(map(str, c)))
def test_rotated_schedules_equal_the_simulation_and_all_ranks_agree(oracle_mod, case):
    assert case[1] % G != 0
    results = _schedule_results(case)
    want, u, chunks = _expected(oracle_mod, case)
    if case[1] == 5_001:
        assert chunks[2][0] == chunks[2][1]   # an empty chunk
    for r in range(case[0]):
        out = results[r][0]
        for name in ("ring", "direct", "scatter", "both"):
            assert np.array_equal(out[name].view(u), want[name][r].view(u)), (name, r)
        for name in ("ring", "direct", "both"):
            assert np.array_equal(out[name].view(u), results[0][0][name].view(u)), (name, r)


@pytest.mark.parametrize("case", SCHEDULES, ids=lambda c: "-".join(map(str, c)))
def test_reduce_scatter_then_all_gather_leaves_the_bytes_of_the_direct_all_reduce(oracle_mod, case):
    """Bit for bit, on every rank: the direct schedule's owner step in the rotated domain IS the reduce-scatter's step (decode_sum 'add' into the
    own chunk) followed by the all-gather's encode.  With the one-launch rotated reduce in its place the property fails -- that one quantizes
    H(x) + sum(T), the two halves H(convert(x + H^-1(sum(T)))), equal in exact arithmetic only: on the model 5 007 of 12 345 float32 words
    (world 2, uint8) to 8 223 of 20 001 bfloat16 words (world 3, uint4) differed -- which is why the schedule does not use it there."""
    results = _schedule_results(case)
    _, u, _ = _expected(oracle_mod, case)
    for r in range(case[0]):
        out = results[r][0]
        differing = int(np.sum(out["both"].view(u) != out["direct"].view(u)))
        print(f"rank {r}: {differing} of {case[1]} words differ")
        assert differing == 0, r


def test_no_seed_makes_exactly_todays_ops_calls(oracle_mod):
    case = SCHEDULES[0]
    results = _schedule_results(case)
    today = [["encode_grouped", "reduce_encode_grouped", "decode_grouped", "decode_grouped"],               # ring, world 2
             ["encode_batch_grouped", "reduce_encode_grouped", "decode_batch_grouped"],                      # direct
             ["encode_batch_grouped", "decode_sum_grouped"],                                                 # reduce-scatter
             ["encode_grouped", "decode_batch_grouped"]]                                                     # all-gather
    for r in range(case[0]):
        traces = results[r][1]
        assert traces["none"] == traces["absent"]
        assert [[c[0] for c in calls] for calls in traces["none"]] == today
        assert all(c[2] is None for calls in traces["none"] for c in calls)


def test_the_call_trace_with_a_seed(oracle_mod):
    """which method, on which chunk (where the tensor's view starts), in which slot (where the record starts in its buffer), in which order"""
    import piquant.distributed as D

    case = SCHEDULES[1]   # world 3, 20 001 bfloat16 elements, quint4x2
    world, numel, _, qname = case
    results = _schedule_results(case)
    chunks = D.ring_chunks(numel, world, QDTYPES[qname])
    begin = [b for b, _ in chunks]
    lens = [D.grouped_wire_layout(e - b, G, QDTYPES[qname]).nbytes for b, e in chunks]
    slot = -(-max(lens) // 16) * 16
    for r in range(world):
        traces = results[r][1]
        peers = [j for j in range(world) if j != r]
        assert traces["direct"] == [
            ("encode_batch_grouped_rotated", [[begin[j] for j in peers], [j * slot for j in peers]], SEED),
            ("decode_sum_grouped_rotated", [[j * slot for j in peers], begin[r]], SEED),      # the owner's step: the reduce-scatter's ...
            ("encode_grouped_rotated", [begin[r], 0], SEED),                                   # ... and the all-gather's
            ("decode_batch_grouped_rotated", [[j * slot for j in range(world)], begin], SEED)], r
        assert traces["direct"] == traces["scatter"] + traces["gather"]
        assert traces["scatter"] == [
            ("encode_batch_grouped_rotated", [[begin[j] for j in peers], [j * slot for j in peers]], SEED),
            ("decode_sum_grouped_rotated", [[j * slot for j in peers], begin[r]], SEED)], r
        assert traces["gather"] == [
            ("encode_grouped_rotated", [begin[r], 0], SEED),
            ("decode_batch_grouped_rotated", [[j * slot for j in range(world)], begin], SEED)], r
        ring = traces["ring"]
        hops = [(r - step - 1) % world for step in range(world - 1)]
        stores = [(r + 1) % world] + [(r - step) % world for step in range(world - 1)]
        assert [c[0] for c in ring] == ["encode_grouped_rotated"] + ["reduce_encode_grouped_rotated"] * (world - 1) + ["decode_grouped_rotated"] * world
        assert ring[0][1] == [begin[r], 0]
        assert [c[1] for c in ring[1:world]] == [[[0], begin[j], 0] for j in hops]
        assert [c[1] for c in ring[world:]] == [[0, begin[j]] for j in stores]
        assert all(c[2] == SEED for c in ring)


def test_rotation_seed_arguments_raise_before_anything_moves():
    """no process group exists here: every one of these raises before the group is asked for anything, and the tensor is untouched"""
    import piquant.distributed as D

    def raises(fn, match, **kwargs):
        x = torch.ones(5000)
        with pytest.raises(ValueError, match=match):
            fn(x, quant_dtype=torch.uint8, rotation_seed=SEED, _ops=object(), **kwargs)
        assert bool((x == 1).all())

    for algorithm in ("ring", "direct"):
        raises(D.quantized_all_reduce, "group_size", algorithm=algorithm)
        raises(D.quantized_all_reduce, "p2p", algorithm=algorithm, group_size=128, transport="p2p")
        raises(D.quantized_all_reduce, "error_feedback", algorithm=algorithm, group_size=128, error_feedback=torch.zeros(5000))
    raises(D.quantized_all_reduce_direct, "group_size")
    raises(D.quantized_all_reduce_direct, "p2p", group_size=128, transport="p2p")
    raises(D.quantized_all_reduce_direct, "error_feedback", group_size=128, error_feedback=torch.zeros(5000))
    for fn in (D.quantized_reduce_scatter, D.quantized_all_gather):
        raises(fn, "group_size", group_size=None)
        raises(fn, "error_feedback", group_size=128, error_feedback=torch.zeros(5000))
    with pytest.raises(ValueError, match="rotation_seed"):
        D.quantized_all_reduce(torch.ones(5000), group_size=128, rotation_seed=1.5, _ops=object())
    # more than 16 records for the owner's one launch: the direct schedule and the reduce-scatter in a group of 18
    with mock.patch.object(D.dist, "get_world_size", return_value=18), mock.patch.object(D.dist, "get_rank", return_value=0):
        raises(D.quantized_all_reduce, "at most 17 ranks", algorithm="direct", group_size=128)
        raises(D.quantized_all_reduce_direct, "at most 17 ranks", group_size=128)
        raises(D.quantized_reduce_scatter, "at most 17 ranks", group_size=128)


def test_more_than_sixteen_terms_raise_in_python():
    """the ctypes methods raise ValueError before the call (which would abort)"""
    import piquant

    class Unreachable:
        def assume_device_pointers(self, flag):
            raise AssertionError("the call was about to be made")

    ptrs = list(range(16, 16 * 18, 16))
    with pytest.raises(ValueError, match="at most 16"):
        piquant.Context.reduce_quantize_grouped_rotated_ptr(Unreachable(), 0, piquant.DataType.F32, ptrs, ptrs, ptrs, 0, piquant.DataType.UINT8, 1, 128, 0, 0,
                                                            SEED, piquant.RoundMode.NEAREST)
    with pytest.raises(ValueError, match="at most 16"):
        piquant.Context.dequantize_sum_grouped_rotated_ptr(Unreachable(), ptrs, piquant.DataType.UINT8, ptrs, ptrs, 0, piquant.DataType.F32, 1, 128, SEED,
                                                           piquant.ReduceOp.SET)


# ---- quality ----

def test_quality_of_the_rotated_collectives_on_outlier_data(oracle_mod):
    """uint4, G = 128, 256 groups, world 3, N(0, 1) with one 50 sigma element per group on every rank, the owner's view of one chunk: the MSE against
    the float64 sum, rotated / un-rotated.  The model gives 0.161 (all-reduce) and 0.087 (reduce-scatter); each bound is twice that, rounded up to
    two digits, and below 1.  The device tests demand bit-identity with this model, so the device inherits the ratios."""
    O, GM, RM, S = _models(oracle_mod)
    from grouped_ring_sim import simulate_direct_grouped
    from grouped_scatter_sim import simulate_reduce_scatter

    world, qd = 3, O.UINT4
    xs = [RM.outlier_data(128, 256, 100 + r) for r in range(world)]
    n = xs[0].size
    chunks = [(0, n)] + [(n, n)] * (world - 1)
    exact = np.sum([x.astype(np.float64) for x in xs], axis=0)

    def mse(a):
        return float(np.mean((a.astype(np.float64) - exact) ** 2))

    all_reduce = mse(S.simulate_direct_rotated(xs, O.F32, qd, chunks, 128, SEED)[0]) / mse(simulate_direct_grouped(xs, O.F32, qd, chunks, 128)[0])
    scatter = mse(S.simulate_reduce_scatter_rotated(xs, O.F32, qd, chunks, 128, SEED)[0]) / mse(simulate_reduce_scatter(xs, O.F32, qd, chunks, 128)[0][0])
    print(f"rotated / un-rotated MSE: all-reduce {all_reduce:.4f}, reduce-scatter {scatter:.4f}")
    assert all_reduce <= 0.33 and all_reduce < 1
    assert scatter <= 0.18 and scatter < 1
