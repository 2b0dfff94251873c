"""CPU, gloo: quantized_all_reduce(group_size=G) -- the grouped ring and mesh schedules, the grouped wire layout and the argument checks.
The wire ops come from the oracle (tests/grouped_ring_sim.py, GroupedOracleOps); tests/test_gpu_grouped_all_reduce.py runs the HIP ones."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
from rank_procs import run_ranks

QDTYPES = {"uint8": 8, "quint4x2": 4, "quint2x4": 2}


def _inputs(world, numel):
    xs = [np.random.default_rng(300 + r).uniform(-1, 1, numel).astype(np.float32) for r in range(world)]
    for r, x in enumerate(xs):   # one outlier per rank, in different groups
        x[(r * 7919 + 13) % numel] = 50.0 * (1 if r % 2 else -1)
    return xs


def _grouped_worker(rank, world, port, numel, qname, algorithm, G):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_ring_sim import GroupedOracleOps

        x = torch.from_numpy(_inputs(world, numel)[rank])
        D.quantized_all_reduce(x, quant_dtype=getattr(torch, qname), algorithm=algorithm, group_size=G, _ops=GroupedOracleOps())
        return x.numpy().copy()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("algorithm", ["ring", "direct"])
@pytest.mark.parametrize("world,numel,qname,G", [(2, 12_345, "uint8", 128), (3, 20_001, "quint4x2", 128), (3, 9_001, "quint2x4", 64),
                                                 (2, 8_195, "quint4x2", 4096)])
def test_grouped_all_reduce_schedule(oracle_mod, world, numel, qname, G, algorithm):
    """Every rank equals the grouped simulation byte for byte (ragged numel: the last group of the last chunk is partial) and all ranks agree."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import simulate_direct_grouped, simulate_ring_grouped

    O = oracle_mod
    assert numel % G != 0
    results = run_ranks(world, _grouped_worker, (numel, qname, algorithm, G), timeout=240)
    bits = QDTYPES[qname]
    qd = {8: O.UINT8, 4: O.UINT4, 2: O.UINT2}[bits]
    xs = _inputs(world, numel)
    sim = simulate_ring_grouped if algorithm == "ring" else simulate_direct_grouped
    want = sim(xs, O.F32, qd, D.ring_chunks(numel, world, bits), G)
    for r in range(world):
        assert np.array_equal(results[r].view(np.uint32), want[r].view(np.uint32)), r
        assert np.array_equal(results[r].view(np.uint32), results[0].view(np.uint32)), r


def test_grouped_simulation_differs_from_the_per_chunk_one(oracle_mod):
    """The grouped schedule is not the per-chunk one in disguise: with an outlier per rank the two give different (and, grouped, closer) sums."""
    sys.path.insert(0, os.path.dirname(__file__))
    import piquant.distributed as D
    from grouped_ring_sim import simulate_direct_grouped
    from ring_sim import simulate_direct

    O = oracle_mod
    world, numel = 3, 20_001
    xs = _inputs(world, numel)
    chunks = D.ring_chunks(numel, world, 4)
    g = simulate_direct_grouped(xs, O.F32, O.UINT4, chunks, 128)[0]
    t = simulate_direct(O, xs, O.UINT4, chunks)[0]
    exact = np.sum(xs, axis=0)
    assert not np.array_equal(g, t)
    assert np.abs(g - exact).mean() * 4 <= np.abs(t - exact).mean()


def test_grouped_wire_layout():
    import piquant.distributed as D

    for numel, G, bits in [(1, 32, 8), (128, 128, 4), (129, 128, 4), (4096, 128, 2), (3_408_000, 128, 8), (27_264_000 // 8, 128, 4), (7, 4096, 2)]:
        lay = D.grouped_wire_layout(numel, G, bits)
        ng = -(-numel // G)
        assert lay.ngroups == ng
        assert lay.zero_points_offset == 4 * ng
        assert lay.data_offset % 16 == 0 and lay.zero_points_offset + ng <= lay.data_offset < lay.zero_points_offset + ng + 16
        assert lay.nbytes == lay.data_offset + -(-numel * bits // 8)
    assert D.grouped_wire_layout(0, 128, 8) == (0, 0, 0, 0)
    # quint4x2 at G = 128: 64 packed bytes and 5 parameter bytes per group, +7.8 %
    lay = D.grouped_wire_layout(1 << 20, 128, 4)
    assert lay.nbytes - (1 << 19) == 5 * (1 << 13)
    # ring_chunks' interior boundaries are multiples of 4096 elements: every wire group is a group of the whole tensor
    for n, world in ((27_264_000, 8), (1_000_003, 3), (20_001, 3)):
        for b, e in D.ring_chunks(n, world, 4)[:-1]:
            assert b % 4096 == 0 and e % 4096 == 0


def _args_worker(rank, world, port):
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import piquant.distributed as D
        from grouped_ring_sim import GroupedOracleOps

        seen = []
        for kwargs in (dict(group_size=100), dict(group_size=16), dict(group_size=8192), dict(group_size=True), dict(group_size=128.0),
                       dict(algorithm="direct", transport="p2p", group_size=128), dict(algorithm="ring", transport="p2p", group_size=128)):
            x = torch.ones(5000)
            try:
                D.quantized_all_reduce(x, quant_dtype=torch.uint8, _ops=GroupedOracleOps(), **kwargs)
                seen.append("no error")
            except (ValueError, RuntimeError) as exc:
                seen.append(type(exc).__name__ + ": " + str(exc))
            seen.append(bool((x == 1).all()))
        for kwargs in (dict(group_size=100), dict(transport="p2p", group_size=128)):
            try:
                D.quantized_all_reduce_direct(torch.ones(10), quant_dtype=torch.uint8, _ops=GroupedOracleOps(), **kwargs)
                seen.append("no error")
            except ValueError as exc:
                seen.append("ValueError: " + str(exc))
        return seen
    finally:
        dist.destroy_process_group()


def test_group_size_arguments_are_checked_before_anything_moves():
    """A bad group_size and group_size with the peer-to-peer transport raise ValueError on every rank alike, and the tensor is untouched."""
    results = run_ranks(2, _args_worker, (), timeout=240)
    for r in range(2):
        seen = results[r]
        msgs, untouched, direct = seen[0:14:2], seen[1:14:2], seen[14:]
        assert all(untouched)
        for m in msgs[:5]:
            assert m.startswith("ValueError") and "group_size" in m, m
        assert msgs[5].startswith("ValueError") and "p2p" in msgs[5], msgs[5]
        assert msgs[6].startswith("ValueError"), msgs[6]
        assert direct[0].startswith("ValueError") and "group_size" in direct[0]
        assert direct[1].startswith("ValueError") and "p2p" in direct[1]


def test_torch_batch_and_reduce_arguments_raise_value_error():
    """piquant.torch's grouped batch / reduce calls check their arguments in Python (ValueError), before any native call could abort."""
    import piquant.torch as pt

    x = torch.zeros(1000)   # a host tensor: every check below fails before the device would be touched
    s, z = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="empty"):
        pt.quantize_grouped_batch([], dtype=torch.uint8)
    with pytest.raises(ValueError, match="empty"):
        pt.dequantize_grouped_batch([], [], [], dtype=torch.float32, group_size=128)
    with pytest.raises(ValueError, match="same length"):
        pt.quantize_grouped_batch([x, x], dtype=torch.uint8, scales=[s], zero_points=[z, z])
    with pytest.raises(ValueError, match="same length"):
        pt.dequantize_grouped_batch([x, x], [s], [z, z], dtype=torch.float32, group_size=128)
    with pytest.raises(ValueError, match="same length"):
        pt.reduce_quantize_grouped(x, [x, x], [s], [z], dtype=torch.uint8)
    for bad in (100, 16, 8192, None, 128.0):
        with pytest.raises(ValueError, match="group_size"):
            pt.quantize_grouped_batch([x], dtype=torch.uint8, group_size=bad)
        with pytest.raises(ValueError, match="group_size"):
            pt.reduce_quantize_grouped(x, [], [], [], dtype=torch.uint8, group_size=bad)
        with pytest.raises(ValueError, match="group_size"):
            pt.dequantize_grouped_batch([x], [s], [z], dtype=torch.float32, group_size=bad)
    with pytest.raises(ValueError, match="ROCm"):
        pt.reduce_quantize_grouped(x, [], [], [], dtype=torch.uint8)
    with pytest.raises(ValueError, match="ROCm"):
        pt.quantize_grouped_batch([x], dtype=torch.uint8)
    with pytest.raises(ValueError):
        pt.reduce_quantize_grouped(x, [], [], [], dtype=torch.float32)
