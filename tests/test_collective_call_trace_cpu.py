"""CPU, gloo: the wire calls every quantized collective makes, in order -- which ``_ops`` method, on which chunk of the tensor and of the residual,
into or out of which slot of the exchange buffers.  The value tests (tests/test_grouped_*_cpu.py) compare results with simulations; this one
states the launches the docstrings of ``piquant.distributed`` promise ("three launches per all-reduce", "two kernel launches per call"): one
batched call that became several, or a residual slice taken from another chunk, changes a trace and not necessarily a value.

The ops object records and computes nothing.  The expected traces are written out below from ``ring_chunks``, ``grouped_wire_layout`` and the
schedules as the docstrings describe them."""
import functools
import os
import sys

import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks

QNAME, BITS, G, ROUND = "quint4x2", 4, 32, "nearest"
HEADER = 16   # the per-chunk record: a 16-byte parameter header, then the packed bytes

# (world, numel): chunks of 4096, 4096 and 3 (a ragged last chunk and a ragged last group); chunk 0 holds everything, chunks 1 and 2 are empty;
# rank 1's chunk is empty
SHAPES = [(3, 8195), (3, 5), (2, 4096)]

# name -> (collective, grouped wire, residual, error_feedback_requantize)
CASES = {
    "ring-perchunk": ("ring", False, False, False),
    "ring-grouped": ("ring", True, False, False),
    "ring-grouped-ef": ("ring", True, True, False),
    "ring-grouped-ef-requantize": ("ring", True, True, True),
    "direct-perchunk": ("direct", False, False, False),
    "direct-grouped": ("direct", True, False, False),
    "direct-grouped-ef": ("direct", True, True, False),
    "direct-grouped-ef-requantize": ("direct", True, True, True),
    "reduce_scatter": ("reduce_scatter", True, False, False),
    "reduce_scatter-ef": ("reduce_scatter", True, True, False),
    "all_gather": ("all_gather", True, False, False),
    "all_gather-ef": ("all_gather", True, True, False),
}


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


def _worker(rank, world, port, numel):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D

        traces = {}
        for name, (collective, grouped, residual, requantize) in CASES.items():
            ops = RecordingOps()
            kw = dict(quant_dtype=getattr(torch, QNAME), round_mode=ROUND, _ops=ops)
            if grouped:
                kw["group_size"] = G
            if residual:
                kw["error_feedback"] = torch.zeros(numel)
            x = torch.zeros(numel)
            if collective in ("ring", "direct"):
                D.quantized_all_reduce(x, algorithm=collective, error_feedback_requantize=requantize, **kw)
            elif collective == "reduce_scatter":
                D.quantized_reduce_scatter(x, **kw)
            else:
                D.quantized_all_gather(x, **kw)
            traces[name] = ops.trace
        return traces
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _traces(world, numel):
    return run_ranks(world, _worker, (numel,), timeout=120)


def _expected(collective, grouped, residual, requantize, world, rank, numel):
    import piquant.distributed as D

    chunks = D.ring_chunks(numel, world, BITS)
    q = "torch." + QNAME
    tail = (G,) if grouped else ()                    # the grouped methods take the group size last
    sfx = "_grouped" if grouped else ""

    def full(j):
        return chunks[j][1] > chunks[j][0]

    def part(j):                                      # chunk j of the flat tensor, and of the flat residual
        b, e = chunks[j]
        return (e - b, b)

    def nbytes(j):                                    # chunk j's record
        b, e = chunks[j]
        return D.grouped_wire_layout(e - b, G, BITS).nbytes if grouped else HEADER + ((e - b) * BITS + 7) // 8

    def encode(j, offset):
        if residual:
            return ("encode_grouped_ef", (part(j), part(j), (nbytes(j), offset), q, ROUND, G))
        return ("encode" + sfx, (part(j), (nbytes(j), offset), q, ROUND) + tail)

    def reduce_encode(terms, j, offset):
        if requantize:
            return ("reduce_encode_grouped_ef", (terms, part(j), part(j), (nbytes(j), offset), q, ROUND, G))
        return ("reduce_encode" + sfx, (terms, part(j), (nbytes(j), offset), q, ROUND) + tail)

    def decode(j, offset):
        return ("decode" + sfx, ((nbytes(j), offset), part(j), q, "set") + tail)

    if collective == "ring":
        # reduce-scatter: the own chunk is encoded; at hop s chunk rank - s - 1 arrives and its sum is re-encoded, one term.  all-gather: the
        # finished chunk rank + 1 is decoded, then at hop s chunk rank - s.  Every buffer is a record at offset 0; empty chunks are skipped.
        want = [encode(rank, 0)] if full(rank) else []
        for step in range(world - 1):
            j = (rank - step - 1) % world
            if full(j):
                want.append(reduce_encode(((nbytes(j), 0),), j, 0))
        for j in [(rank + 1) % world] + [(rank - step) % world for step in range(world - 1)]:
            if full(j):
                want.append(decode(j, 0))
        return want

    # the mesh: slot j of a world-slot buffer belongs to rank j; a slot is the longest record, rounded up to 16 bytes
    slot = -(-max(nbytes(j) for j in range(world)) // 16) * 16
    peers = [j for j in range(world) if j != rank and full(j)]
    everyone = [j for j in range(world) if full(j)]
    records = tuple((nbytes(j), j * slot) for j in peers)
    parts = tuple(part(j) for j in peers)
    if residual:
        scatter = ("encode_batch_grouped_ef", (parts, parts, records, q, ROUND, G))     # one batched call, made even when there is nothing to encode
    else:
        scatter = ("encode_batch" + sfx, (parts, records, q, ROUND) + tail)
    received = tuple((nbytes(rank), i * slot) for i in range(world) if i != rank)        # the peers' records of the own chunk, by rank
    gather = ("decode_batch" + sfx, (tuple((nbytes(j), j * slot) for j in everyone), tuple(part(j) for j in everyone), q, "set") + tail)
    if collective == "direct":
        return [scatter] + ([reduce_encode(received, rank, 0)] if full(rank) else []) + [gather]
    if collective == "reduce_scatter":
        return [scatter] + ([("decode_sum_grouped", (received, part(rank), q, "add", G))] if full(rank) else [])
    return ([encode(rank, 0)] if full(rank) else []) + [gather]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("world,numel", SHAPES)
def test_the_wire_calls_of_every_schedule(world, numel, case):
    import piquant.distributed as D

    chunks = D.ring_chunks(numel, world, BITS)
    assert chunks == {8195: [(0, 4096), (4096, 8192), (8192, 8195)], 5: [(0, 5), (5, 5), (5, 5)], 4096: [(0, 4096), (4096, 4096)]}[numel]
    results = _traces(world, numel)
    for rank in range(world):
        want = _expected(*CASES[case], world, rank, numel)
        got = results[rank][case]
        assert got == want, f"{case}, rank {rank} of {world}, {numel} elements:\n  made     {got}\n  expected {want}"


def test_the_launch_counts_the_docstrings_promise():
    """With no empty chunk: three calls per mesh all-reduce, two per reduce-scatter and per all-gather, 2 * world per ring all-reduce."""
    world, numel = SHAPES[0]
    results = _traces(world, numel)
    for rank in range(world):
        for case, (collective, *_) in CASES.items():
            want = {"ring": 2 * world, "direct": 3, "reduce_scatter": 2, "all_gather": 2}[collective]
            assert len(results[rank][case]) == want, (case, rank)
