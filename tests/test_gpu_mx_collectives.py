"""GPU: the four quantized collectives over the MX wire (mx_format=).  Two processes share the one GPU over gloo; the schedules and every kernel are
the real ones, so each rank must equal, bit for bit, the few lines below that write the schedule from tests/mx_model.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mx_model as M
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu

NUMEL, WORLD = 3 * 4096 + 37, 2


def _rank_input(rank, fdt):
    """Blocks that span exponents; float32, or bfloat16 bits."""
    rng = np.random.default_rng(2300 + rank)
    x = (rng.uniform(-1, 1, (-(-NUMEL // 32), 32)) * np.ldexp(1.0, rng.integers(-12, 12, (-(-NUMEL // 32), 1)))).astype(np.float32).ravel()[:NUMEL]
    return (x.view(np.uint32) >> 16).astype(np.uint16) if fdt == "bfloat16" else x


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
                return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) if fdt == "bfloat16" else torch.from_numpy(x.copy()).cuda()

            def host(t):
                return t.view(torch.int16).cpu().numpy().view(np.uint16) if fdt == "bfloat16" else t.cpu().numpy()

            a = D.quantized_all_reduce(fresh(), algorithm=algorithm, mx_format=fmt)
            direct = D.quantized_all_reduce(fresh(), algorithm="direct", mx_format=fmt)
            t = fresh()
            D.quantized_reduce_scatter(t, mx_format=fmt)
            torch.cuda.synchronize()
            scattered = host(t)
            D.quantized_all_gather(t, mx_format=fmt)
            torch.cuda.synchronize()
            out[fdt] = host(a), host(direct), scattered, host(t)
        return out
    finally:
        dist.destroy_process_group()


def _add(held, terms, fmt, bf16):
    """dequantize_mx ADD of every term, in order, into a copy of `held`: the sum rounded to its type after each."""
    for codes, scales in terms:
        held = M.store(M.dequantize(codes, scales, fmt), held, bf16)
    return held


def _encode(held, fmt, bf16):
    return M.quantize(M.bf16_to_f32(held) if bf16 else held, fmt)


def _model(xs, chunks, algorithm, fmt, bf16):
    """(the all-reduced tensor every rank ends with, the tensor each rank holds after the reduce-scatter alone)"""
    world = len(xs)
    final, scattered = xs[0].copy(), [x.copy() for x in xs]
    for c, (b, e) in enumerate(chunks):
        if algorithm == "ring":       # chunk c starts at rank c and is re-quantized at each of the world - 1 hops
            rec = _encode(xs[c][b:e], fmt, bf16)
            for step in range(1, world):
                rec = _encode(_add(xs[(c + step) % world][b:e], [rec], fmt, bf16), fmt, bf16)
        else:                         # rank c owns chunk c: the peers' records in increasing rank order, one reduce_quantize_mx
            scattered[c][b:e] = _add(xs[c][b:e], [_encode(xs[i][b:e], fmt, bf16) for i in range(world) if i != c], fmt, bf16)
            rec = _encode(scattered[c][b:e], fmt, bf16)
        final[b:e] = M.store(M.dequantize(*rec, fmt), None, bf16)
    return final, scattered


@pytest.mark.parametrize("fmt", [M.FP4, M.FP8])
@pytest.mark.parametrize("algorithm", ["ring", "direct"])
def test_collectives_equal_the_model_of_their_schedule(algorithm, fmt):
    import piquant.distributed as D

    results = run_ranks(WORLD, _worker, (algorithm, fmt), timeout=300)
    chunks = D.ring_chunks(NUMEL, WORLD, 8)
    for fdt in ("float32", "bfloat16"):
        bf16 = fdt == "bfloat16"
        u = np.uint16 if bf16 else np.uint32
        xs = [_rank_input(r, fdt) for r in range(WORLD)]
        want, _ = _model(xs, chunks, algorithm, fmt, bf16)
        want_direct, want_scattered = _model(xs, chunks, "direct", fmt, bf16)
        for r in range(WORLD):
            got, direct, scattered, both = (v.view(u) for v in results[r][fdt])
            assert np.array_equal(got, want.view(u)), f"rank {r} {fdt}: all-reduce differs from the model of the {algorithm} schedule"
            assert np.array_equal(direct, want_direct.view(u)) and np.array_equal(scattered, want_scattered[r].view(u)), (r, fdt)
            assert np.array_equal(both, direct), f"rank {r} {fdt}: reduce-scatter + all-gather != the direct all-reduce"
            assert np.array_equal(got, results[0][fdt][0].view(u)), f"rank {r} {fdt}: the ranks differ"


REFUSED = [dict(group_size=64), dict(error_feedback=True), dict(rotation_seed=1), dict(rotated_error_feedback=True), dict(clip_steps=2),
           dict(transport="p2p"), dict(quant_dtype=torch.quint4x2), dict(round_mode="stochastic"), dict(world=18)]


ALL_REDUCES, SHARDED = ["quantized_all_reduce", "quantized_all_reduce_direct"], ["quantized_reduce_scatter", "quantized_all_gather"]
# transport= is the all-reduces' argument; the all-gather sums nothing, so any world size goes
CASES = [(n, e) for e in REFUSED for n in ALL_REDUCES + SHARDED if not (n in SHARDED and "transport" in e) and not (n == SHARDED[1] and "world" in e)]


@pytest.mark.parametrize("name,extra", CASES, ids=[f"{n}-{next(iter(e))}" for n, e in CASES])
def test_refused_combinations_raise_before_anything_moves(monkeypatch, name, extra):
    import piquant.distributed as D

    fn = getattr(D, name)
    extra = dict(extra)
    world = extra.pop("world", None)
    t = torch.arange(4096, dtype=torch.float32, device="cuda")
    for k in extra:
        if extra[k] is True:
            extra[k] = torch.zeros_like(t)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: world or 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    with pytest.raises(ValueError):
        fn(t, mx_format=M.FP4, **extra)
    assert torch.equal(t, torch.arange(4096, dtype=torch.float32, device="cuda"))
