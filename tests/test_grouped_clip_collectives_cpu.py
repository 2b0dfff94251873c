"""CPU, gloo: with ``clip_steps=`` the reduce-scatter and the all-gather make exactly the clipped encode calls -- the batched one on the peers'
chunks, the single one on the own chunk -- and leave the decode side as it is; every combination the clip search does not cover raises
ValueError before anything moves.  The recording ops object is the one of tests/test_collective_call_trace_cpu.py, which pins the calls made
with ``clip_steps=None``."""
import functools
import os
import sys

import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks
from test_collective_call_trace_cpu import BITS, G, QNAME, ROUND, SHAPES, RecordingOps

STEPS = 9


def _worker(rank, world, port, numel):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        traces, refused = {}, {}
        for name, call in (("reduce_scatter", D.quantized_reduce_scatter), ("all_gather", D.quantized_all_gather)):
            ops = RecordingOps()
            call(torch.zeros(numel), quant_dtype=getattr(torch, QNAME), round_mode=ROUND, group_size=G, clip_steps=STEPS, _ops=ops)
            traces[name] = ops.trace
            for what, kw in (("rotation_seed", dict(rotation_seed=5)), ("error_feedback", dict(error_feedback=torch.zeros(numel))),
                             ("rotated_error_feedback", dict(rotation_seed=5, rotated_error_feedback=torch.zeros(numel))),
                             ("steps 0", dict(clip_steps=0)), ("steps 13", dict(clip_steps=13)), ("steps 2.0", dict(clip_steps=2.0)),
                             ("steps True", dict(clip_steps=True))):
                ops = RecordingOps()
                try:
                    call(torch.zeros(numel), **{**dict(quant_dtype=getattr(torch, QNAME), group_size=G, clip_steps=STEPS, _ops=ops), **kw})
                    refused[name, what] = "no error"
                except ValueError as e:
                    refused[name, what] = ("ValueError", "clip_steps" in str(e), ops.trace)
        for algorithm in ("ring", "direct"):
            for what, kw in (("grouped", dict(group_size=G)), ("per-chunk", dict()), ("p2p", dict(transport="p2p"))):
                ops = RecordingOps()
                try:
                    D.quantized_all_reduce(torch.zeros(numel), quant_dtype=getattr(torch, QNAME), algorithm=algorithm, clip_steps=STEPS, _ops=ops, **kw)
                    refused[algorithm, what] = "no error"
                except ValueError as e:
                    refused[algorithm, what] = ("ValueError", "clip_steps" in str(e), ops.trace)
        ops = RecordingOps()
        try:
            D.quantized_all_reduce_direct(torch.zeros(numel), quant_dtype=getattr(torch, QNAME), group_size=G, clip_steps=STEPS, _ops=ops)
            refused["direct entry", "grouped"] = "no error"
        except ValueError as e:
            refused["direct entry", "grouped"] = ("ValueError", "clip_steps" in str(e), ops.trace)
        return traces, refused
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _results(world, numel):
    return run_ranks(world, _worker, (numel,), timeout=120)


def _expected(collective, world, rank, numel):
    import piquant.distributed as D

    chunks = D.ring_chunks(numel, world, BITS)
    q = "torch." + QNAME
    full = lambda j: chunks[j][1] > chunks[j][0]                                   # noqa: E731
    part = lambda j: (chunks[j][1] - chunks[j][0], chunks[j][0])                   # noqa: E731
    nbytes = lambda j: D.grouped_wire_layout(chunks[j][1] - chunks[j][0], G, BITS).nbytes   # noqa: E731
    slot = -(-max(nbytes(j) for j in range(world)) // 16) * 16
    if collective == "reduce_scatter":
        peers = [j for j in range(world) if j != rank and full(j)]
        scatter = ("encode_batch_grouped_clipped", (tuple(part(j) for j in peers), tuple((nbytes(j), j * slot) for j in peers), q, ROUND, G, STEPS))
        received = tuple((nbytes(rank), i * slot) for i in range(world) if i != rank)
        return [scatter] + ([("decode_sum_grouped", (received, part(rank), q, "add", G))] if full(rank) else [])
    everyone = [j for j in range(world) if full(j)]
    gather = ("decode_batch_grouped", (tuple((nbytes(j), j * slot) for j in everyone), tuple(part(j) for j in everyone), q, "set", G))
    return ([("encode_grouped_clipped", (part(rank), (nbytes(rank), 0), q, ROUND, G, STEPS))] if full(rank) else []) + [gather]


@pytest.mark.parametrize("collective", ["reduce_scatter", "all_gather"])
@pytest.mark.parametrize("world,numel", SHAPES)
def test_clip_steps_changes_the_encode_calls_and_nothing_else(world, numel, collective):
    for rank in range(world):
        got = _results(world, numel)[rank][0][collective]
        want = _expected(collective, world, rank, numel)
        assert got == want, f"{collective}, rank {rank} of {world}, {numel} elements:\n  made     {got}\n  expected {want}"


def test_every_refused_combination_raises_before_anything_moves():
    world, numel = SHAPES[0]
    for rank in range(world):
        refused = _results(world, numel)[rank][1]
        assert len(refused) == 2 * 7 + 2 * 3 + 1
        for key, outcome in refused.items():
            assert outcome == ("ValueError", True, []), (rank, key, outcome)
