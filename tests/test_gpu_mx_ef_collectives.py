"""GPU: the quantized collectives over the MX wire with error feedback (mx_format= with mx_error_feedback=).  Two processes share the one GPU over
gloo; the schedules and every kernel are the real ones, so each rank's tensor AND residual must equal, bit for bit, the few lines below that write
the schedule from tests/mx_model.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mx_model as M
from rank_procs import run_ranks
from test_gpu_mx_collectives import _add, _encode, _rank_input

pytestmark = pytest.mark.gpu

NUMEL, WORLD = 3 * 4096 + 37, 2
SCHEDULES = [("ring", M.FP4), ("direct", M.FP8)]   # one format per schedule


def _rank_residual(rank):
    rng = np.random.default_rng(2400 + rank)
    return (rng.uniform(-0.25, 0.25, (-(-NUMEL // 32), 32)) * np.ldexp(1.0, rng.integers(-12, 12, (-(-NUMEL // 32), 1)))).astype(np.float32).ravel()[:NUMEL]


def _worker(rank, world, port, algorithm, fmt):
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for p in (str(root), str(root / "pi-quant_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        torch.cuda.set_device(0)
        out = {}
        for fdt in ("float32", "bfloat16"):
            x = _rank_input(rank, fdt)

            def fresh():
                t = torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy()).cuda()
                return t, torch.from_numpy(_rank_residual(rank)).cuda()

            def host(t, r):
                torch.cuda.synchronize()
                return (t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy()), r.cpu().numpy()

            runs = []
            for requantize in (False, True):
                t, r = fresh()
                D.quantized_all_reduce(t, algorithm=algorithm, mx_format=fmt, mx_error_feedback=r, error_feedback_requantize=requantize)
                runs.append(host(t, r))
            t, r = fresh()
            D.quantized_reduce_scatter(t, mx_format=fmt, mx_error_feedback=r)
            D.quantized_all_gather(t, mx_format=fmt, mx_error_feedback=r)
            runs.append(host(t, r))
            out[fdt] = runs
        return out
    finally:
        dist.destroy_process_group()


def _encode_ef(held, res, fmt, bf16):
    """quantize_mx_ef: (the record, the new residual) of the held values and their float32 residual."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = (M.bf16_to_f32(held) if bf16 else held) + res
        rec = M.quantize(y, fmt)
        return rec, y - M.dequantize(*rec, fmt)


def _model(xs, residuals, chunks, algorithm, fmt, bf16, requantize):
    """(the all-reduced tensor every rank ends with, the residual of every rank)"""
    world = len(xs)
    final, res = xs[0].copy(), [r.copy() for r in residuals]
    for c, (b, e) in enumerate(chunks):
        def step(rank, held, ef):   # an encode at `rank`, feeding that rank's chunk of its residual or leaving it alone
            if not ef:
                return _encode(held, fmt, bf16)
            rec, res[rank][b:e] = _encode_ef(held, res[rank][b:e], fmt, bf16)
            return rec

        if algorithm == "ring":       # chunk c starts at rank c (its own values: always fed) and is re-quantized at each of the world - 1 hops
            rec = step(c, xs[c][b:e], True)
            for hop in range(1, world):
                q = (c + hop) % world
                rec = step(q, _add(xs[q][b:e], [rec], fmt, bf16), requantize)
        else:                         # rank c owns chunk c: the peers' records (always fed) in increasing rank order, then the owner's step
            rec = step(c, _add(xs[c][b:e], [step(i, xs[i][b:e], True) for i in range(world) if i != c], fmt, bf16), requantize)
        final[b:e] = M.store(M.dequantize(*rec, fmt), None, bf16)
    return final, res


@pytest.mark.parametrize("algorithm,fmt", SCHEDULES)
def test_tensor_and_residual_equal_the_model_of_the_schedule(algorithm, fmt):
    import piquant.distributed as D

    results = run_ranks(WORLD, _worker, (algorithm, fmt), timeout=300)
    chunks = D.ring_chunks(NUMEL, WORLD, 8)
    for fdt in ("float32", "bfloat16"):
        bf16 = fdt == "bfloat16"
        u = np.uint16 if bf16 else np.uint32
        xs, rs = [_rank_input(r, fdt) for r in range(WORLD)], [_rank_residual(r) for r in range(WORLD)]
        wants = [_model(xs, rs, chunks, algorithm, fmt, bf16, requantize) for requantize in (False, True)]
        wants.append(_model(xs, rs, chunks, "direct", fmt, bf16, True))   # reduce-scatter + all-gather: the direct all-reduce that feeds every step
        for r in range(WORLD):
            for (got, got_res), (want, want_res), what in zip(results[r][fdt], wants, ("plain", "requantize", "reduce-scatter + all-gather")):
                assert np.array_equal(got.view(u), want.view(u)), f"rank {r} {fdt} {what}: the tensor differs from the model of the schedule"
                assert np.array_equal(got_res.view(np.uint32), want_res[r].view(np.uint32)), f"rank {r} {fdt} {what}: the residual differs"


REFUSED = [dict(mx_format=None), dict(error_feedback=True), dict(transport="p2p"), dict(mx_error_feedback=torch.bfloat16)]
ALL_REDUCES, SHARDED = ["quantized_all_reduce", "quantized_all_reduce_direct"], ["quantized_reduce_scatter", "quantized_all_gather"]
CASES = [(n, e) for e in REFUSED for n in ALL_REDUCES + SHARDED if not (n in SHARDED and "transport" in e)]


@pytest.mark.parametrize("name,extra", CASES, ids=[f"{n}-{next(iter(e))}" for n, e in CASES])
def test_refused_combinations_raise_before_anything_moves(monkeypatch, name, extra):
    import piquant.distributed as D

    t = torch.arange(4096, dtype=torch.float32, device="cuda")
    kw = dict(mx_format=M.FP4, mx_error_feedback=torch.ones(4096, device="cuda"))
    kw.update(extra)
    if kw.get("error_feedback") is True:
        kw.update(error_feedback=torch.zeros_like(t))
    if kw["mx_error_feedback"] is torch.bfloat16:
        kw["mx_error_feedback"] = torch.ones(4096, dtype=torch.bfloat16, device="cuda")
    residual = kw["mx_error_feedback"]
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    with pytest.raises(ValueError):
        getattr(D, name)(t, **kw)
    assert torch.equal(t, torch.arange(4096, dtype=torch.float32, device="cuda")) and torch.equal(residual, torch.ones_like(residual))
