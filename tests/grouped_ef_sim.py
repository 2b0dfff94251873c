"""Reference simulation of piquant.distributed.quantized_all_reduce(group_size=G, error_feedback=residual) for W ranks in one process, built from
the error-feedback model (tests/ef_model.py) and the group model, and an oracle-backed stand-in for the error-feedback wire ops of
piquant.distributed._DeviceOps.  The schedules are those of tests/grouped_ring_sim.py; only the quantizations a rank applies to its own
contribution change: they quantize values + residual and leave what the quantization lost in the residual."""
import numpy as np

import oracle as O
from ef_model import ef_step
from grouped_model import dequantize_grouped, quantize_grouped
from grouped_ring_sim import GroupedOracleOps, _assemble


def simulate_ring_grouped_ef(xs, rs, dt, qd, chunks, G):
    """The ring: chunk c is first encoded by rank c -- with error feedback on rank c's slice [b, e) of its residual --, then ranks c + 1, ... add
    their own values to the decoded partial sum and re-encode it (no residual).  -> (results, new residuals)."""
    W = len(xs)
    rs = [r.copy() for r in rs]
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        q, s, z, rs[c][b:e], _, _ = ef_step(xs[c][b:e], rs[c][b:e], dt, qd, G)
        for j in range(1, W):
            acc = dequantize_grouped(q, qd, dt, e - b, G, s, z, O.ADD, prev=xs[(c + j) % W][b:e])
            q, s, z = quantize_grouped(acc, dt, qd, G)
        final.append(dequantize_grouped(q, qd, dt, e - b, G, s, z))
    return _assemble(xs, chunks, final), rs


def simulate_direct_grouped_ef(xs, rs, dt, qd, chunks, G):
    """The mesh: every rank src != c encodes its chunk c with error feedback on its slice [b, e) of its residual; the owner adds the decoded chunks
    to its own (unquantized) values in increasing rank order and encodes the sum once (no residual).  -> (results, new residuals)."""
    W = len(xs)
    rs = [r.copy() for r in rs]
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        acc = xs[c][b:e].copy()
        for src in range(W):
            if src != c:
                q, s, z, rs[src][b:e], _, _ = ef_step(xs[src][b:e], rs[src][b:e], dt, qd, G)
                acc = dequantize_grouped(q, qd, dt, e - b, G, s, z, O.ADD, prev=acc)
        q, s, z = quantize_grouped(acc, dt, qd, G)
        final.append(dequantize_grouped(q, qd, dt, e - b, G, s, z))
    return _assemble(xs, chunks, final), rs


def untouched_slices(chunks, rank, algorithm):
    """The chunks of rank `rank`'s residual that the schedule neither reads nor writes."""
    if algorithm == "ring":
        return [(b, e) for c, (b, e) in enumerate(chunks) if c != rank]
    return [chunks[rank]]


class GroupedEfOracleOps(GroupedOracleOps):
    """GroupedOracleOps plus the error-feedback encodes, on CPU float32 torch tensors (nearest rounding)."""

    def encode_grouped_ef(self, x, residual, buf, qdtype, round_mode, group_size):
        import torch

        qd = self._qd(qdtype)
        lay, _ = self._split(buf, x.numel(), qd, group_size)
        q, s, z, r_new, _, _ = ef_step(x.numpy(), residual.numpy(), O.F32, qd, group_size)
        rec = np.zeros(lay.nbytes, dtype=np.uint8)
        rec[: lay.zero_points_offset] = s.view(np.uint8)
        rec[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups] = z
        rec[lay.data_offset:] = q
        buf.copy_(torch.from_numpy(rec))
        residual.copy_(torch.from_numpy(r_new))

    def encode_batch_grouped_ef(self, xs, residuals, bufs, qdtype, round_mode, group_size):
        for x, r, buf in zip(xs, residuals, bufs):
            self.encode_grouped_ef(x, r, buf, qdtype, round_mode, group_size)
