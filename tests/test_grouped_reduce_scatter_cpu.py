"""CPU, gloo: quantized_reduce_scatter and quantized_all_gather on the grouped wire -- the schedules, what they leave alone, error feedback and
the argument checks.  The wire ops come from the oracle (tests/grouped_scatter_sim.py, GroupedScatterOracleOps);
tests/test_gpu_grouped_reduce_scatter.py runs the HIP ones."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks

QDTYPES = {"uint8": 8, "quint4x2": 4, "quint2x4": 2}
SENTINEL = np.float32(-12345.5)


def _inputs(world, numel, step=0):
    xs = [np.random.default_rng(300 + 17 * step + r).uniform(-1, 1, numel).astype(np.float32) for r in range(world)]
    for r, x in enumerate(xs):   # one outlier per rank, in different groups
        x[(r * 7919 + 13 + step) % numel] = 50.0 * (1 if r % 2 else -1)
    return xs


def _worker(rank, world, port, numel, qname, G):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_scatter_sim import GroupedScatterOracleOps

        qdtype, ops = getattr(torch, qname), GroupedScatterOracleOps()
        b, e = D.ring_chunks(numel, world, QDTYPES[qname])[rank]
        x = torch.from_numpy(_inputs(world, numel)[rank].copy())
        view = D.quantized_reduce_scatter(x, quant_dtype=qdtype, group_size=G, _ops=ops)
        is_view = view.numel() == e - b and (view.numel() == 0 or view.data_ptr() == x.view(-1)[b:e].data_ptr())
        view_then = view.numpy().copy()
        scattered = x.numpy().copy()
        got = D.quantized_all_gather(x, quant_dtype=qdtype, group_size=G, _ops=ops)
        both = x.numpy().copy()
        y = torch.from_numpy(_inputs(world, numel)[rank].copy())
        D.quantized_all_reduce(y, quant_dtype=qdtype, algorithm="direct", group_size=G, _ops=ops)
        g = torch.from_numpy(_inputs(world, numel)[rank].copy())
        D.quantized_all_gather(g, quant_dtype=qdtype, group_size=G, _ops=ops)
        return dict(is_view=is_view, returns_tensor=got is x, view=view_then, scattered=scattered, both=both, all_reduce=y.numpy().copy(),
                    gathered=g.numpy().copy())
    finally:
        dist.destroy_process_group()


# world 2 and 3, ragged numel (numel % G != 0); 5_000 elements over three ranks: chunks of 4096, 904 and NOTHING
@pytest.mark.parametrize("world,numel,qname,G", [(2, 12_345, "uint8", 128), (3, 20_001, "quint4x2", 128), (3, 9_001, "quint2x4", 64),
                                                 (3, 5_000, "quint4x2", 32), (2, 8_195, "uint8", 4096)])
def test_reduce_scatter_and_all_gather_schedules(oracle_mod, world, numel, qname, G):
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import simulate_direct_grouped
    from grouped_scatter_sim import simulate_all_gather, simulate_reduce_scatter

    O = oracle_mod
    assert numel % G != 0
    bits = QDTYPES[qname]
    qd = {8: O.UINT8, 4: O.UINT4, 2: O.UINT2}[bits]
    chunks = D.ring_chunks(numel, world, bits)
    if numel == 5_000:
        assert chunks[-1][0] == chunks[-1][1], "this case is here for its empty chunk"
    results = run_ranks(world, _worker, (numel, qname, G), timeout=240)
    xs = _inputs(world, numel)
    want_rs, _ = simulate_reduce_scatter(xs, O.F32, qd, chunks, G)
    want_both, _ = simulate_all_gather(want_rs, O.F32, qd, chunks, G)
    want_ag, _ = simulate_all_gather(xs, O.F32, qd, chunks, G)
    want_ar = simulate_direct_grouped(xs, O.F32, qd, chunks, G)
    for r in range(world):
        res = results[r]
        b, e = chunks[r]
        assert res["is_view"] and res["returns_tensor"], r
        assert np.array_equal(res["view"].view(np.uint32), want_rs[r][b:e].view(np.uint32)), f"rank {r}: the returned view differs from the simulation"
        assert np.array_equal(res["scattered"].view(np.uint32), want_rs[r].view(np.uint32)), f"rank {r}: a chunk that is not its own was changed"
        untouched = np.ones(numel, dtype=bool)
        untouched[b:e] = False
        assert np.array_equal(res["scattered"][untouched].view(np.uint32), xs[r][untouched].view(np.uint32)), r
        assert np.array_equal(res["gathered"].view(np.uint32), want_ag[r].view(np.uint32)), r
        assert np.array_equal(res["gathered"].view(np.uint32), results[0]["gathered"].view(np.uint32)), f"rank {r}: all-gather must leave all ranks identical"
        assert np.array_equal(res["both"].view(np.uint32), want_both[r].view(np.uint32)), r
        assert np.array_equal(res["both"].view(np.uint32), want_ar[r].view(np.uint32)), f"rank {r}: reduce-scatter + all-gather != the simulated all-reduce"
        assert np.array_equal(res["both"].view(np.uint32), res["all_reduce"].view(np.uint32)), f"rank {r}: reduce-scatter + all-gather != quantized_all_reduce"


# ---- error feedback -------------------------------------------------------------------------------------------------------------------
def _ef_worker(rank, world, port, numel, qname, G, steps):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_scatter_sim import GroupedScatterOracleOps

        qdtype, ops = getattr(torch, qname), GroupedScatterOracleOps()
        b, e = D.ring_chunks(numel, world, QDTYPES[qname])[rank]
        res_rs = torch.zeros(numel)
        res_rs[b:e] = float(SENTINEL)                  # reduce-scatter must not look at the rank's own chunk of the residual
        res_ag = torch.full((numel,), float(SENTINEL))
        res_ag[b:e] = 0.0                              # all-gather must look at nothing else
        views, gathers = [], []
        for step in range(steps):
            x = torch.from_numpy(_inputs(world, numel, step)[rank].copy())
            views.append(D.quantized_reduce_scatter(x, quant_dtype=qdtype, group_size=G, error_feedback=res_rs, _ops=ops).numpy().copy())
            g = torch.from_numpy(_inputs(world, numel, step)[rank].copy())
            D.quantized_all_gather(g, quant_dtype=qdtype, group_size=G, error_feedback=res_ag, _ops=ops)
            gathers.append(g.numpy().copy())
        return views, gathers, res_rs.numpy().copy(), res_ag.numpy().copy()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,numel,qname,G", [(2, 12_345, "uint8", 128), (3, 20_001, "quint4x2", 128)])
def test_error_feedback_covers_the_peers_chunks_only(oracle_mod, world, numel, qname, G):
    """Two consecutive steps with the residual carried over: views and residuals equal the simulation bit for bit; the own chunk of a
    reduce-scatter's residual, and every other chunk of an all-gather's, keep their sentinel."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_scatter_sim import simulate_all_gather, simulate_reduce_scatter

    O = oracle_mod
    steps, bits = 2, QDTYPES[qname]
    qd = {8: O.UINT8, 4: O.UINT4, 2: O.UINT2}[bits]
    chunks = D.ring_chunks(numel, world, bits)
    results = run_ranks(world, _ef_worker, (numel, qname, G, steps), timeout=240)
    rs_rs, rs_ag = [], []
    for r, (b, e) in enumerate(chunks):
        a = np.zeros(numel, dtype=np.float32)
        a[b:e] = SENTINEL
        g = np.full(numel, SENTINEL, dtype=np.float32)
        g[b:e] = 0.0
        rs_rs.append(a)
        rs_ag.append(g)
    for step in range(steps):
        xs = _inputs(world, numel, step)
        want, rs_rs = simulate_reduce_scatter(xs, O.F32, qd, chunks, G, rs_rs)
        want_g, rs_ag = simulate_all_gather(xs, O.F32, qd, chunks, G, rs_ag)
        for r, (b, e) in enumerate(chunks):
            assert np.array_equal(results[r][0][step].view(np.uint32), want[r][b:e].view(np.uint32)), (step, r)
            assert np.array_equal(results[r][1][step].view(np.uint32), want_g[r].view(np.uint32)), (step, r)
    for r, (b, e) in enumerate(chunks):
        got_rs, got_ag = results[r][2], results[r][3]
        assert np.array_equal(got_rs.view(np.uint32), rs_rs[r].view(np.uint32)), r
        assert np.array_equal(got_ag.view(np.uint32), rs_ag[r].view(np.uint32)), r
        assert np.all(got_rs[b:e] == SENTINEL), f"rank {r}: reduce-scatter touched its own chunk of the residual"
        other = np.ones(numel, dtype=bool)
        other[b:e] = False
        assert np.any(got_rs[other] != 0), "the residual was never written"
        assert np.all(got_ag[other] == SENTINEL), f"rank {r}: all-gather touched a chunk of the residual that is not its own"
        assert e == b or np.any(got_ag[b:e] != 0)


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_scatter_is_conservative_over_steps(oracle_mod, world):
    """K = 8 chained reduce-scatters of U(-1, 1) float32 inputs over a quint4x2 wire, simulated in-process.  In float64,
        S = sum_t (the owners' sums, laid end to end) + sum_ranks residual_final - sum_t sum_ranks x_t.
    Every quantization of the collective is an error-feedback one, so with the residual S is nothing but roundings to float32: per element and
    step the W - 1 peer encodes round twice each (y = rn(x + r), r' = rn(y - d)) and the owner adds W - 1 terms, 3W - 3 roundings of at most
    eps / 2 M.  The margin is the one tests/test_grouped_reduce_ef_cpu.py asserts for the all-reduce, K (3W - 1) / 2 eps M: the run with the
    residual stays below it, the simulation's own run with the residual dropped exceeds it (a uint4 step loses about range / 30)."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from ef_model import EPS
    from grouped_scatter_sim import simulate_reduce_scatter

    O = oracle_mod
    dt, qd, numel, G, K = O.F32, O.UINT4, 5_003, 128, 8
    chunks = D.ring_chunks(numel, world, 4, align=1024)              # several non-empty chunks at a few thousand elements
    assert sum(1 for b, e in chunks if e > b) == world
    rng = np.random.default_rng(977 + world)
    steps = [[rng.uniform(-1, 1, numel).astype(np.float32) for _ in range(world)] for _ in range(K)]

    def defect(with_residual, seen):
        rs = [np.zeros(numel, dtype=np.float32) for _ in range(world)] if with_residual else None
        S = np.zeros(numel, dtype=np.float64)
        for xs in steps:
            outs, rs = simulate_reduce_scatter(xs, dt, qd, chunks, G, rs, seen)
            for r, (b, e) in enumerate(chunks):
                S[b:e] += outs[r][b:e].astype(np.float64)
                if with_residual:
                    assert not rs[r][b:e].any(), "the own chunk of the residual is not touched"
            for x in xs:
                S -= x.astype(np.float64)
        for r in rs or []:
            S += r.astype(np.float64)
        return float(np.abs(S).max())

    seen = [max(float(np.abs(x).max()) for xs in steps for x in xs)]
    d_on = defect(True, seen)
    M = max(seen)
    bound = K * (3 * world - 1) / 2 * EPS[dt] * M
    d_off = defect(False, None)
    print(f"W={world}: with the residual max|S| = {d_on:.4g}, residual dropped max|S| = {d_off:.4g}, bound = {bound:.4g} (M = {M:.4g})")
    assert d_on <= bound, (d_on, bound)
    assert d_off > bound, (d_off, bound)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_anything_moves():
    """The checks come before the first use of the process group: no group is needed to see them, and the tensor and residual are untouched."""
    import piquant.distributed as D

    n = 5000
    for call in (D.quantized_reduce_scatter, D.quantized_all_gather):
        for bad in (None, 100, 16, 8192, True, 128.0):
            x = torch.ones(n)
            with pytest.raises(ValueError, match="group_size"):
                call(x, group_size=bad)
            assert bool((x == 1).all())
        good = torch.zeros(n)
        for residual, what in ((torch.zeros(n, dtype=torch.bfloat16), "dtype"), (torch.zeros(n - 1), "numel"), (torch.zeros(2 * n)[::2], "contiguous"),
                               (torch.zeros(n, device="meta"), "device"), ("no tensor", "Tensor")):
            x = torch.ones(n)
            with pytest.raises(ValueError, match=what):
                call(x, error_feedback=residual)
            assert bool((x == 1).all())
        with pytest.raises(ValueError, match="group_size"):
            call(torch.ones(n), group_size=100, error_feedback=good)
        with pytest.raises(ValueError, match="contiguous float32 or bfloat16"):
            call(torch.ones(n, dtype=torch.float64))
        with pytest.raises(ValueError, match="contiguous float32 or bfloat16"):
            call(torch.ones(2 * n)[::2])
        assert bool((good == 0).all())


def _one_rank_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        x = torch.arange(5000, dtype=torch.float32)
        res = torch.full((5000,), 3.0)
        v = D.quantized_reduce_scatter(x, quant_dtype=torch.quint4x2, error_feedback=res)
        ok = v.data_ptr() == x.data_ptr() and v.numel() == 5000
        ok = ok and D.quantized_all_gather(x, quant_dtype=torch.quint4x2, error_feedback=res) is x
        return ok and bool((res == 3.0).all()) and bool((x == torch.arange(5000, dtype=torch.float32)).all())
    finally:
        dist.destroy_process_group()


def test_a_one_rank_group_returns_at_once():
    """No device, no ops: a one-rank group never reaches them, and leaves tensor and residual alone."""
    assert run_ranks(1, _one_rank_worker, (), timeout=120)[0] is True
