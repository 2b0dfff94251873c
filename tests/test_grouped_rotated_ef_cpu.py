"""CPU: error feedback in the rotated domain (tests/rot_ef_model.py: the model of piquant_hip_quantize_grouped_rotated_ef /
_reduce_quantize_grouped_rotated_ef) -- what the definition is, what it is not, what it conserves and what it buys -- and piquant.distributed's
four collectives with rotated_error_feedback= over gloo, the wire ops coming from that model (tests/grouped_rotated_ef_sim.py).
tests/test_gpu_grouped_rotated_ef.py and tests/test_gpu_grouped_rotated_ef_all_reduce.py hold the HIP kernels to the same models bit for bit."""
import functools
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks

SEED = 0x1234567887654321
QSEED = 0x9E3779B97F4A7C15   # the seed of the quality tables


def _models(oracle_mod):
    sys.path.insert(0, os.path.dirname(__file__))
    import ef_model as EF
    import grouped_model as GM
    import grouped_rotated_ef_sim as ES
    import grouped_rotated_sim as S
    import rot_ef_model as RE
    import rot_model as RM

    return oracle_mod, GM, RM, S, EF, RE, ES


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


def _residual(O, RE, dt, qd, G, n):
    """a residual of a realistic size: what one step on other data leaves"""
    return RE.quantize_grouped_rotated_ef(_heavy(n, 77, O, dt), dt, np.zeros(n, dtype=np.float32), qd, G, SEED)[3]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the definition ----

def test_no_terms_is_the_plain_call_and_a_zero_residual_gives_the_rotated_quantize(oracle_mod):
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    for dt, qd, G, n, _ in _cases(O):
        x, r = _heavy(n, 1, O, dt), _residual(O, RE, dt, qd, G, n)
        for got, want in zip(RE.reduce_quantize_grouped_rotated_ef(x, dt, r, [], qd, G, SEED)[:4], RE.quantize_grouped_rotated_ef(x, dt, r, qd, G, SEED)[:4]):
            assert np.array_equal(_bits(got), _bits(want))
        zero = RE.quantize_grouped_rotated_ef(x, dt, np.zeros(n, dtype=np.float32), qd, G, SEED)
        for got, want in zip(zero[:3], RM.quantize_grouped_rotated(x, dt, qd, G, SEED)):
            assert np.array_equal(_bits(got), _bits(want))
        assert zero[3].dtype == np.float32 and r.dtype == np.float32   # float32 also for a bfloat16 tensor
        # the definition, written as the composition of the existing models
        q, s, z, new, _, _ = EF.ef_step(RM.hadamard_grouped(RM.widen(x, dt), O.F32, G, SEED), r, O.F32, qd, G)
        for got, want in zip(RE.quantize_grouped_rotated_ef(x, dt, r, qd, G, SEED)[:4], (q, s, z, new)):
            assert np.array_equal(_bits(got), _bits(want))


def test_the_ragged_group_is_not_rotated_but_gets_its_residual_and_its_terms(oracle_mod):
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    for dt, qd, G, n, k in _cases(O):
        full = n // G * G
        if full == n:
            continue
        acc, terms, r = _heavy(n, 3, O, dt), _terms(O, RM, dt, qd, G, n, k), _residual(O, RE, dt, qd, G, n)
        y = RE.reduce_quantize_grouped_rotated_ef(acc, dt, r, terms, qd, G, SEED)[4]
        tail = RM.widen(acc, dt)[full:]
        for q, s, z in terms:
            tail = GM.dequantize_grouped(q, qd, O.F32, n, G, s, z, O.ADD, prev=np.concatenate([np.zeros(full, np.float32), tail]))[full:]
        assert not np.array_equal(tail, RM.widen(acc, dt)[full:])            # the terms did arrive
        assert np.any(r[full:] != 0)
        assert np.array_equal((tail + r[full:]).view(np.uint32), y[full:].view(np.uint32))


def test_a_nan_poisons_the_residual_of_its_whole_group_and_nothing_else(oracle_mod):
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    G, n, qd = 64, 4 * 64 + 9, O.UINT4
    x = _heavy(n, 5, O, O.F32).copy()
    x[G + 3] = np.nan          # a full group
    x[4 * G + 2] = np.nan      # the ragged group: not rotated, so the NaN stays one element
    r0 = np.zeros(n, dtype=np.float32)
    q, s, z, r1, _, _ = RE.quantize_grouped_rotated_ef(x, O.F32, r0, qd, G, SEED)
    nan = np.isnan(r1)
    assert nan[G: 2 * G].all() and nan[4 * G + 2] and nan.sum() == G + 1
    # the next step, on clean data: the group's residual is still NaN -- until the caller zeroes it
    r2 = RE.quantize_grouped_rotated_ef(_heavy(n, 6, O, O.F32), O.F32, r1, qd, G, SEED)[3]
    assert np.array_equal(np.isnan(r2), nan)
    r1[nan] = 0
    assert not np.isnan(RE.quantize_grouped_rotated_ef(_heavy(n, 6, O, O.F32), O.F32, r1, qd, G, SEED)[3]).any()


# ---- what the definition is not: every variant changes at least one byte of the output or of the residual on a committed case ----

def _variants(O, GM, RM, S, EF):
    def terms_added(y, terms, qd, G):
        for q, s, z in terms:
            y = GM.dequantize_grouped(q, qd, O.F32, y.size, G, s, z, O.ADD, prev=y)
        return y

    def tail(y, qd, G, params_from=None, flip=False):
        s, z = GM.group_params_all(y if params_from is None else params_from, G, qd)
        q = GM.quantize_grouped(y, O.F32, qd, G, params=(s, z))[0]
        d = GM.dequantize_grouped(q, qd, O.F32, y.size, G, s, z)
        return q, s, z, (d - y if flip else y - d)

    def residual_before_the_rotation(acc, dt, r, terms, qd, G):
        return tail(terms_added(RM.rotate(RM.widen(acc, dt) + r, G, SEED), terms, qd, G), qd, G)

    def residual_in_the_original_domain(acc, dt, r, terms, qd, G):
        y = terms_added(RM.rotate(RM.widen(acc, dt), G, SEED), terms, qd, G) + RM.rotate(r, G, SEED)
        q, s, z, _ = tail(y, qd, G)
        d = GM.dequantize_grouped(q, qd, O.F32, y.size, G, s, z)
        return q, s, z, RM.rotate(y, G, SEED, inverse=True) - RM.rotate(d, G, SEED, inverse=True)

    def residual_before_the_terms(acc, dt, r, terms, qd, G):
        return tail(terms_added(RM.rotate(RM.widen(acc, dt), G, SEED) + r, terms, qd, G), qd, G)

    def bf16_residual(acc, dt, r, terms, qd, G):
        q, s, z, new = tail(terms_added(RM.rotate(RM.widen(acc, dt), G, SEED), terms, qd, G) + r, qd, G)
        return q, s, z, O.bf16_to_f32(O.f32_to_bf16(new))

    def bf16_running_sum(acc, dt, r, terms, qd, G):
        y = RM.rotate(RM.widen(acc, dt), G, SEED)
        for t in terms:
            y = O.bf16_to_f32(O.f32_to_bf16(terms_added(y, [t], qd, G)))
        return tail(y + r, qd, G)

    def d_minus_y(acc, dt, r, terms, qd, G):
        return tail(terms_added(RM.rotate(RM.widen(acc, dt), G, SEED), terms, qd, G) + r, qd, G, flip=True)

    def ragged_rotated(acc, dt, r, terms, qd, G):
        x = RM.widen(acc, dt)
        pad = np.zeros(-(-x.size // G) * G, dtype=np.float32)
        pad[: x.size] = x
        return tail(terms_added(RM.rotate(pad, G, SEED)[: x.size], terms, qd, G) + r, qd, G)

    def parameters_from_before_the_residual(acc, dt, r, terms, qd, G):
        Y = terms_added(RM.rotate(RM.widen(acc, dt), G, SEED), terms, qd, G)
        return tail(Y + r, qd, G, params_from=Y)

    return [residual_before_the_rotation, residual_in_the_original_domain, residual_before_the_terms, bf16_residual, bf16_running_sum, d_minus_y,
            ragged_rotated, parameters_from_before_the_residual]


def test_wrong_variants_change_a_byte(oracle_mod):
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    with np.errstate(over="ignore", invalid="ignore"):
        for variant in _variants(O, GM, RM, S, EF):
            differs = False
            for dt, qd, G, n, k in _cases(O):
                acc, terms, r = _heavy(n, 4, O, dt), _terms(O, RM, dt, qd, G, n, k), _residual(O, RE, dt, qd, G, n)
                want = RE.reduce_quantize_grouped_rotated_ef(acc, dt, r, terms, qd, G, SEED)[:4]
                got = variant(acc, dt, r, terms, qd, G)
                differs = differs or any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want))
            assert differs, variant.__name__


def test_the_right_composition_written_the_variants_way_changes_nothing(oracle_mod):
    """the variants' helpers, put together the right way round, reproduce the model: a variant differs because of its one change"""
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    for dt, qd, G, n, k in _cases(O):
        acc, terms, r = _heavy(n, 4, O, dt), _terms(O, RM, dt, qd, G, n, k), _residual(O, RE, dt, qd, G, n)
        y = RM.rotate(RM.widen(acc, dt), G, SEED)
        for q, s, z in terms:
            y = GM.dequantize_grouped(q, qd, O.F32, n, G, s, z, O.ADD, prev=y)
        y = y + r
        s, z = GM.group_params_all(y, G, qd)
        q = GM.quantize_grouped(y, O.F32, qd, G, params=(s, z))[0]
        new = y - GM.dequantize_grouped(q, qd, O.F32, n, G, s, z)
        for got, want in zip((q, s, z, new), RE.reduce_quantize_grouped_rotated_ef(acc, dt, r, terms, qd, G, SEED)[:4]):
            assert np.array_equal(_bits(got), _bits(want))


# ---- conservation and quality: G = 128, 64 groups, float32, 16 chained steps, step t on rot_model.outlier_data(128, 64, 100 + t) ----

STEPS, QG, QNG = 16, 128, 64


@pytest.mark.parametrize("wire", ("uint4", "uint8"))
def test_conservation_over_sixteen_steps(oracle_mod, wire):
    """sum_t D_t = sum_t H(x_t) + R_0 - R_K in the rotated domain, within K 2^-23 M (ef_model.conservation_defect)"""
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    qd = {"uint4": O.UINT4, "uint8": O.UINT8}[wire]
    r = np.zeros(QG * QNG, dtype=np.float32)
    Ys, ds, ys = [], [], []
    for t in range(STEPS):
        x = RM.outlier_data(QG, QNG, 100 + t)
        q, s, z, r, y, d = RE.quantize_grouped_rotated_ef(x, O.F32, r, qd, QG, QSEED)
        Ys.append(RM.rotate(x, QG, QSEED))
        ds.append(d)
        ys.append(y)
    defect, bound = EF.conservation_defect(Ys, ds, r, ys, O.F32)
    print(f"{wire}: conservation defect {defect:.3g}, bound {bound:.3g}")
    assert defect <= bound


def _mse(a, exact):
    return float(np.mean((a.astype(np.float64) - exact) ** 2))


@pytest.mark.parametrize("wire,vs_ef,vs_rot", [("uint4", 0.0709, 0.0684), ("uint8", 0.373, 0.0775)])
def test_quality_of_chained_steps(oracle_mod, wire, vs_ef, vs_rot):
    """The MSE of the accumulated dequantized sum against the float64 sum: plain, error feedback only, rotation only, both.  The bounds are twice
    the model's ratios (the margin of the existing quality tests) and below 1."""
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    qd = {"uint4": O.UINT4, "uint8": O.UINT8}[wire]
    n = QG * QNG
    exact = np.zeros(n)
    acc = {k: np.zeros(n) for k in ("plain", "ef", "rot", "rot_ef")}
    r_ef, r_rot = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    for t in range(STEPS):
        x = RM.outlier_data(QG, QNG, 100 + t)
        exact += x
        q, s, z = GM.quantize_grouped(x, O.F32, qd, QG)
        acc["plain"] += GM.dequantize_grouped(q, qd, O.F32, n, QG, s, z)
        q, s, z, r_ef, _, d = EF.ef_step(x, r_ef, O.F32, qd, QG)
        acc["ef"] += d
        q, s, z = RM.quantize_grouped_rotated(x, O.F32, qd, QG, QSEED)
        acc["rot"] += RM.dequantize_grouped_rotated(q, qd, O.F32, n, QG, s, z, QSEED)
        q, s, z, r_rot, _, d = RE.quantize_grouped_rotated_ef(x, O.F32, r_rot, qd, QG, QSEED)
        acc["rot_ef"] += RM.dequantize_grouped_rotated(q, qd, O.F32, n, QG, s, z, QSEED)
    m = {k: _mse(v, exact) for k, v in acc.items()}
    print(f"{wire}: plain {m['plain']:.4g}, EF {m['ef']:.4g}, rotation {m['rot']:.4g}, rotation + EF {m['rot_ef']:.4g}; "
          f"rot+EF / EF {m['rot_ef'] / m['ef']:.4f}, rot+EF / rot {m['rot_ef'] / m['rot']:.4f}")
    assert m["rot_ef"] / m["ef"] <= 2 * vs_ef and m["rot_ef"] / m["ef"] < 1
    assert m["rot_ef"] / m["rot"] <= 2 * vs_rot and m["rot_ef"] / m["rot"] < 1


@pytest.mark.parametrize("wire", ("uint4", "uint2"))
def test_quality_of_the_all_reduce(oracle_mod, wire):
    """The owner's view of one chunk of a 3-rank direct all-reduce over 16 steps, rank r, step t on outlier_data(128, 64, 1000 r + 100 + t), error
    feedback on every quantization, the owner's re-quantization included.  uint4: rot+EF / EF <= 2 * 0.103 and rot+EF / rot <= 2 * 0.0625, both
    below 1; uint2 (where the rotation alone loses): rot+EF < EF."""
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    from grouped_reduce_ef_sim import simulate_direct_grouped_ef_all
    from grouped_ring_sim import simulate_direct_grouped

    qd = {"uint4": O.UINT4, "uint2": O.UINT2}[wire]
    W, n = 3, QG * QNG
    chunks = [(0, n)] + [(n, n)] * (W - 1)
    exact = np.zeros(n)
    acc = {k: np.zeros(n) for k in ("plain", "ef", "rot", "rot_ef")}
    rs_ef = [np.zeros(n, dtype=np.float32) for _ in range(W)]
    rs_rot = [np.zeros(n, dtype=np.float32) for _ in range(W)]
    for t in range(STEPS):
        xs = [RM.outlier_data(QG, QNG, 1000 * r + 100 + t) for r in range(W)]
        exact += np.sum([x.astype(np.float64) for x in xs], axis=0)
        acc["plain"] += simulate_direct_grouped(xs, O.F32, qd, chunks, QG)[0]
        out, rs_ef = simulate_direct_grouped_ef_all(xs, rs_ef, O.F32, qd, chunks, QG)
        acc["ef"] += out[0]
        acc["rot"] += S.simulate_direct_rotated(xs, O.F32, qd, chunks, QG, QSEED)[0]
        out, rs_rot = ES.simulate_direct_rotated_ef(xs, rs_rot, O.F32, qd, chunks, QG, QSEED, True)
        acc["rot_ef"] += out[0]
    m = {k: _mse(v, exact) for k, v in acc.items()}
    print(f"{wire}: plain {m['plain']:.4g}, EF {m['ef']:.4g}, rotation {m['rot']:.4g}, rotation + EF {m['rot_ef']:.4g}; "
          f"rot+EF / EF {m['rot_ef'] / m['ef']:.4f}, rot+EF / rot {m['rot_ef'] / m['rot']:.4f}")
    if wire == "uint4":
        assert m["rot_ef"] / m["ef"] <= 2 * 0.103 and m["rot_ef"] / m["ef"] < 1
        assert m["rot_ef"] / m["rot"] <= 2 * 0.0625 and m["rot_ef"] / m["rot"] < 1
    else:
        assert m["rot_ef"] < m["ef"]


# ---- argument checks: before anything moves ----

def test_rotated_error_feedback_arguments_raise_before_anything_moves():
    """no process group exists here: every one of these raises before the group is asked for anything, and tensor and residual are untouched"""
    import piquant.distributed as D

    def raises(fn, match, residual=None, **kwargs):
        x = torch.ones(5000)
        r = torch.full((5000,), 2.0) if residual is None else residual
        before = r.clone() if isinstance(r, torch.Tensor) else list(r)
        kwargs.setdefault("rotation_seed", SEED)
        kwargs.setdefault("group_size", 128)
        with pytest.raises(ValueError, match=match):
            fn(x, quant_dtype=torch.uint8, rotated_error_feedback=r, _ops=object(), **kwargs)
        assert bool((x == 1).all()) and (torch.equal(r, before) if isinstance(r, torch.Tensor) else r == before)

    fns = [(D.quantized_all_reduce, dict(algorithm="ring")), (D.quantized_all_reduce, dict(algorithm="direct")), (D.quantized_all_reduce_direct, {}),
           (D.quantized_reduce_scatter, {}), (D.quantized_all_gather, {})]
    for fn, kw in fns:
        raises(fn, "group_size", group_size=None, **kw)
        raises(fn, "rotation_seed", rotation_seed=None, **kw)
        raises(fn, "error_feedback", error_feedback=torch.zeros(5000), **kw)
        raises(fn, "float32", residual=torch.zeros(5000, dtype=torch.bfloat16), **kw)
        raises(fn, "float32", residual=torch.zeros(5000, dtype=torch.float64), **kw)
        raises(fn, "numel", residual=torch.zeros(4999), **kw)
        raises(fn, "contiguous", residual=torch.zeros(10000)[::2], **kw)
        raises(fn, "torch.Tensor", residual=[0.0] * 5000, **kw)
        if torch.cuda.is_available():
            raises(fn, "device", residual=torch.zeros(5000, device="cuda"), **kw)
    for fn, kw in fns[:3]:
        raises(fn, "p2p", transport="p2p", **kw)
    # a bfloat16 tensor takes a float32 residual only
    with pytest.raises(ValueError, match="float32"):
        D.quantized_all_reduce(torch.ones(5000, dtype=torch.bfloat16), group_size=128, rotation_seed=SEED,
                               rotated_error_feedback=torch.zeros(5000, dtype=torch.bfloat16), _ops=object())
    # error_feedback_requantize: accepted with either residual keyword (the call then reaches the process group), still raises with neither
    for fn, kw in fns[:3]:
        with pytest.raises(ValueError, match="error_feedback_requantize"):
            fn(torch.ones(5000), group_size=128, rotation_seed=SEED, error_feedback_requantize=True, _ops=object(), **kw)
        with mock.patch.object(D.dist, "get_world_size", return_value=1), mock.patch.object(D.dist, "get_rank", return_value=0):
            x = torch.ones(5000)
            assert fn(x, group_size=128, rotation_seed=SEED, error_feedback_requantize=True, rotated_error_feedback=torch.zeros(5000), _ops=object(),
                      **kw) is x
            assert fn(x, group_size=128, error_feedback_requantize=True, error_feedback=torch.zeros(5000), _ops=object(), **kw) is x
    # error_feedback= with a rotation keeps raising, and names the keyword that goes with a rotation
    with pytest.raises(ValueError, match="rotated_error_feedback"):
        D.quantized_all_reduce(torch.ones(5000), group_size=128, rotation_seed=SEED, error_feedback=torch.zeros(5000), _ops=object())


def test_more_than_sixteen_terms_raise_in_python():
    import piquant

    class Unreachable:
        def assume_device_pointers(self, flag):
            raise AssertionError("the call was about to be made")

    ptrs = list(range(16, 16 * 18, 16))
    with pytest.raises(ValueError, match="at most 16"):
        piquant.Context.reduce_quantize_grouped_rotated_ef_ptr(Unreachable(), 0, piquant.DataType.F32, 0, ptrs, ptrs, ptrs, 0, piquant.DataType.UINT8, 1, 128,
                                                               0, 0, SEED, piquant.RoundMode.NEAREST)


# ---- the schedules, through the _ops seam ----

QDTYPES = {"uint8": 8, "quint4x2": 4}
# (world, numel, tensor type, wire type): ragged last groups; 5_001 elements leave rank 2 of 3 an empty chunk
SCHEDULES = [(2, 12_345, "float32", "uint8"), (3, 20_001, "bfloat16", "quint4x2"), (3, 5_001, "float32", "quint4x2")]
G = 128
CALLS = 2   # consecutive calls, the residual carried over


def _inputs(O, world, numel, fdt, call):
    return [_heavy(numel, 300 + 10 * call + r, O, O.BF16 if fdt == "bfloat16" else O.F32) for r in range(world)]


def _schedule_worker(rank, world, port, numel, fdt, qname):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import oracle as O
        import piquant.distributed as D
        from grouped_rotated_ef_sim import GroupedRotatedEfOracleOps

        qdtype = getattr(torch, qname)

        def tensor(x):
            return torch.from_numpy(x.view(np.int16).copy()).view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy())

        def host(t):
            return t.view(torch.int16).numpy().view(np.uint16).copy() if fdt == "bfloat16" else t.numpy().copy()

        kw = dict(quant_dtype=qdtype, group_size=G, rotation_seed=SEED, _ops=GroupedRotatedEfOracleOps())
        out = {}
        for name, algorithm, requantize in (("ring", "ring", False), ("ring-rq", "ring", True), ("direct", "direct", False), ("direct-rq", "direct", True)):
            r, steps = torch.zeros(numel), []
            for call in range(CALLS):
                t = tensor(_inputs(O, world, numel, fdt, call)[rank])
                D.quantized_all_reduce(t, algorithm=algorithm, rotated_error_feedback=r, error_feedback_requantize=requantize, **kw)
                steps.append((host(t), r.numpy().copy()))
            out[name] = steps
        r, scatter, both = torch.zeros(numel), [], []
        for call in range(CALLS):
            t = tensor(_inputs(O, world, numel, fdt, call)[rank])
            D.quantized_reduce_scatter(t, rotated_error_feedback=r, **kw)
            scatter.append((host(t), r.numpy().copy()))
            D.quantized_all_gather(t, rotated_error_feedback=r, **kw)
            both.append((host(t), r.numpy().copy()))
        out["scatter"], out["both"] = scatter, both
        return out
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _schedule_results(case):
    return run_ranks(case[0], _schedule_worker, case[1:], timeout=240)


def _expected(oracle_mod, case):
    O, GM, RM, S, EF, RE, ES = _models(oracle_mod)
    import piquant.distributed as D

    world, numel, fdt, qname = case
    bits = QDTYPES[qname]
    qd, dt = {8: O.UINT8, 4: O.UINT4}[bits], O.BF16 if fdt == "bfloat16" else O.F32
    chunks = D.ring_chunks(numel, world, bits)
    zeros = [np.zeros(numel, dtype=np.float32) for _ in range(world)]
    want = {}
    for name, sim, requantize in (("ring", ES.simulate_ring_rotated_ef, False), ("ring-rq", ES.simulate_ring_rotated_ef, True),
                                  ("direct", ES.simulate_direct_rotated_ef, False), ("direct-rq", ES.simulate_direct_rotated_ef, True)):
        rs, steps = zeros, []
        for call in range(CALLS):
            outs, rs = sim(_inputs(O, world, numel, fdt, call), rs, dt, qd, chunks, G, SEED, requantize)
            steps.append((outs, rs))
        want[name] = steps
    rs, scatter, both = zeros, [], []
    for call in range(CALLS):
        outs, rs = ES.simulate_reduce_scatter_rotated_ef(_inputs(O, world, numel, fdt, call), rs, dt, qd, chunks, G, SEED)
        scatter.append((outs, rs))
        outs, rs = ES.simulate_all_gather_rotated_ef(outs, rs, dt, qd, chunks, G, SEED)
        both.append((outs, rs))
    want["scatter"], want["both"] = scatter, both
    return want, (np.uint16 if dt == O.BF16 else np.uint32), chunks


@pytest.mark.parametrize("case", SCHEDULES, ids=lambda c: "-".join(map(str, c)))
def test_schedules_equal_the_simulation_in_tensor_and_residual_over_two_calls(oracle_mod, case):
    assert case[1] % G != 0
    results = _schedule_results(case)
    want, u, chunks = _expected(oracle_mod, case)
    for r in range(case[0]):
        for name, steps in want.items():
            for call, (outs, rs) in enumerate(steps):
                got_t, got_r = results[r][name][call]
                assert np.array_equal(got_t.view(u), outs[r].view(u)), (name, r, call, "tensor")
                assert np.array_equal(got_r.view(np.uint32), rs[r].view(np.uint32)), (name, r, call, "residual")
                if name != "scatter":
                    assert np.array_equal(got_t.view(u), results[0][name][call][0].view(u)), (name, r, call, "ranks agree")
        assert np.any(results[r]["direct-rq"][0][1] != 0)
        # without requantize the mesh leaves the rank's own chunk of the residual alone; with it every chunk is fed
        b, e = chunks[r]
        assert not np.any(results[r]["direct"][CALLS - 1][1][b:e])
        if e > b:
            assert np.any(results[r]["direct-rq"][CALLS - 1][1][b:e])


@pytest.mark.parametrize("case", SCHEDULES, ids=lambda c: "-".join(map(str, c)))
def test_reduce_scatter_then_all_gather_is_the_direct_all_reduce_with_requantize(oracle_mod, case):
    """tensor bytes AND residual bytes, on every rank, after each of the two calls"""
    results = _schedule_results(case)
    for r in range(case[0]):
        for call in range(CALLS):
            (bt, br), (dt_, dr) = results[r]["both"][call], results[r]["direct-rq"][call]
            assert np.array_equal(bt.view(np.uint8), dt_.view(np.uint8)), (r, call, "tensor")
            assert np.array_equal(br.view(np.uint32), dr.view(np.uint32)), (r, call, "residual")


# ---- the call trace ----

def _describe(arg):
    if isinstance(arg, torch.Tensor):
        return (arg.numel(), arg.storage_offset())
    if isinstance(arg, (list, tuple)):
        return tuple(_describe(a) for a in arg)
    return str(arg) if isinstance(arg, torch.dtype) else arg


class RecordingOps:
    """Stands in for ``_DeviceOps``: every method appends (its name, a description of its arguments) and does nothing else."""

    def __init__(self):
        self.trace = []

    def __getattr__(self, name):
        def record(*args):
            self.trace.append((name, tuple(_describe(a) for a in args)))
        return record


TRACE_NUMEL, TRACE_G, TRACE_Q, TRACE_BITS = 3 * 4096 + 3, 32, "quint4x2", 4
TRACE_CASES = [(collective, requantize, residual) for collective in ("ring", "direct", "reduce_scatter", "all_gather")
               for requantize in (False, True) for residual in (True, False) if not (requantize and (collective in ("reduce_scatter", "all_gather") or not residual))]


def _trace_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        traces = {}
        for collective, requantize, residual in TRACE_CASES:
            for variant in ((True,) if residual else ("none", "absent")):
                ops = RecordingOps()
                kw = dict(quant_dtype=getattr(torch, TRACE_Q), group_size=TRACE_G, rotation_seed=SEED, _ops=ops)
                if residual:
                    kw["rotated_error_feedback"] = torch.zeros(TRACE_NUMEL)
                elif variant == "none":
                    kw["rotated_error_feedback"] = None
                x = torch.zeros(TRACE_NUMEL, dtype=torch.bfloat16)
                if collective in ("ring", "direct"):
                    D.quantized_all_reduce(x, algorithm=collective, error_feedback_requantize=requantize, **kw)
                elif collective == "reduce_scatter":
                    D.quantized_reduce_scatter(x, **kw)
                else:
                    D.quantized_all_gather(x, **kw)
                traces[(collective, requantize, variant)] = ops.trace
        return traces
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _trace_results(world):
    return run_ranks(world, _trace_worker, (), timeout=120)


def _expected_trace(collective, requantize, residual, world, rank):
    import piquant.distributed as D

    chunks = D.ring_chunks(TRACE_NUMEL, world, TRACE_BITS)
    q, tail = "torch." + TRACE_Q, ("nearest", TRACE_G, SEED)

    def full(j):
        return chunks[j][1] > chunks[j][0]

    def part(j):
        return (chunks[j][1] - chunks[j][0], chunks[j][0])

    def nbytes(j):
        return D.grouped_wire_layout(chunks[j][1] - chunks[j][0], TRACE_G, TRACE_BITS).nbytes

    def encode(j, offset, ef):
        if ef:
            return ("encode_grouped_rotated_ef", (part(j), part(j), (nbytes(j), offset), q) + tail)
        return ("encode_grouped_rotated", (part(j), (nbytes(j), offset), q) + tail)

    def decode(j, offset):
        return ("decode_grouped_rotated", ((nbytes(j), offset), part(j), q, "set", TRACE_G, SEED))

    if collective == "ring":
        want = [encode(rank, 0, residual)] if full(rank) else []
        for step in range(world - 1):
            j = (rank - step - 1) % world
            if full(j):
                if requantize:
                    want.append(("reduce_encode_grouped_rotated_ef", (((nbytes(j), 0),), part(j), part(j), (nbytes(j), 0), q) + tail))
                else:
                    want.append(("reduce_encode_grouped_rotated", (((nbytes(j), 0),), part(j), (nbytes(j), 0), q) + tail))
        return want + [decode(j, 0) for j in [(rank + 1) % world] + [(rank - step) % world for step in range(world - 1)] if full(j)]
    slot = -(-max(nbytes(j) for j in range(world)) // 16) * 16
    peers = [j for j in range(world) if j != rank and full(j)]
    everyone = [j for j in range(world) if full(j)]
    records, parts = tuple((nbytes(j), j * slot) for j in peers), tuple(part(j) for j in peers)
    scatter = ("encode_batch_grouped_rotated_ef", (parts, parts, records, q) + tail) if residual else ("encode_batch_grouped_rotated", (parts, records, q) + tail)
    received = tuple((nbytes(rank), i * slot) for i in range(world) if i != rank)
    add = [("decode_sum_grouped_rotated", (received, part(rank), q, "add", TRACE_G, SEED))] if full(rank) and received else []
    gather = ("decode_batch_grouped_rotated", (tuple((nbytes(j), j * slot) for j in everyone), tuple(part(j) for j in everyone), q, "set", TRACE_G, SEED))
    if collective == "direct":
        return [scatter] + add + ([encode(rank, 0, residual and requantize)] if full(rank) else []) + [gather]
    if collective == "reduce_scatter":
        return [scatter] + add
    return ([encode(rank, 0, residual)] if full(rank) else []) + [gather]


@pytest.mark.parametrize("world", (1, 2, 3, 4))
def test_the_wire_calls_with_the_rotated_residual(world):
    """which op, on which chunk of the tensor AND of the residual, into which slot: every chunk of the residual at most once per call -- exactly
    once with requantize.  A one-rank group returns at once: no call at all.  Without the keyword (absent, or None) the trace is the rotated one."""
    import piquant.distributed as D

    results = _trace_results(world)
    chunks = D.ring_chunks(TRACE_NUMEL, world, TRACE_BITS)
    for rank in range(world):
        for collective, requantize, residual in TRACE_CASES:
            for variant in ((True,) if residual else ("none", "absent")):
                got = results[rank][(collective, requantize, variant)]
                want = [] if world == 1 else _expected_trace(collective, requantize, residual, world, rank)
                assert got == want, f"{collective}, requantize={requantize}, residual={variant}, rank {rank} of {world}:\n  made     {got}\n  expected {want}"
                if residual and world > 1:
                    fed = [a[2 if name.startswith("reduce") else 1] for name, a in got if name.endswith("_ef") and not name.startswith("encode_batch")]
                    fed += [p for name, a in got if name.startswith("encode_batch") and name.endswith("_ef") for p in a[1]]
                    assert len(fed) == len(set(fed)), (collective, requantize, rank)
                    if requantize:
                        assert sorted(fed) == sorted((e - b, b) for b, e in chunks if e > b), (collective, rank)
