"""Reference simulation of piquant.distributed.quantized_all_reduce(group_size=G, error_feedback=residual[, error_feedback_requantize=True]) for
a BFLOAT16 tensor with a FLOAT32 residual, W ranks in one process, and an oracle-backed stand-in for the wire ops on CPU bfloat16 tensors.

The schedules are those of tests/grouped_ef_sim.py (flag off) and tests/grouped_reduce_ef_sim.py (flag on).  Everything that carries no residual
stays in the bfloat16 pipeline (partial sums rounded to bfloat16 after every term, re-quantizations and decodes of bfloat16 values); every
quantization that carries one is the mixed step of tests/ef_f32r_model.py: float32 on the widened values, residual float32.
Values are bf16 bit patterns (uint16 arrays), residuals float32 arrays."""
import numpy as np

import oracle as O
from ef_f32r_model import ef_f32r_step
from grouped_model import dequantize_grouped, quantize_grouped
from grouped_reduce_ef_sim import GroupedReduceEfOracleOps
from grouped_ring_sim import _assemble

BF16 = O.BF16


def reduce_ef_f32r_step(acc, r, terms, qd, G):
    """the terms by grouped dequantize ADD into the bfloat16 acc, in order, then the mixed step on (acc, r)"""
    acc = acc.copy()
    for q, s, z in terms:
        acc = dequantize_grouped(q, qd, BF16, acc.size, G, s, z, O.ADD, prev=acc)
    return ef_f32r_step(acc, r, qd, G)


def simulate_ring_f32r(xs, rs, qd, chunks, G, requantize):
    """-> (results as bf16 bits, new float32 residuals)"""
    W = len(xs)
    rs = [r.copy() for r in rs]
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        q, s, z, rs[c][b:e], _, _ = ef_f32r_step(xs[c][b:e], rs[c][b:e], qd, G)
        for j in range(1, W):
            k = (c + j) % W
            if requantize:
                q, s, z, rs[k][b:e], _, _ = reduce_ef_f32r_step(xs[k][b:e], rs[k][b:e], [(q, s, z)], qd, G)
            else:
                acc = dequantize_grouped(q, qd, BF16, e - b, G, s, z, O.ADD, prev=xs[k][b:e])
                q, s, z = quantize_grouped(acc, BF16, qd, G)
        final.append(dequantize_grouped(q, qd, BF16, e - b, G, s, z))
    return _assemble(xs, chunks, final), rs


def simulate_direct_f32r(xs, rs, qd, chunks, G, requantize):
    """-> (results as bf16 bits, new float32 residuals)"""
    W = len(xs)
    rs = [r.copy() for r in rs]
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        terms = []
        for src in range(W):
            if src != c:
                q, s, z, rs[src][b:e], _, _ = ef_f32r_step(xs[src][b:e], rs[src][b:e], qd, G)
                terms.append((q, s, z))
        if requantize:
            q, s, z, rs[c][b:e], _, _ = reduce_ef_f32r_step(xs[c][b:e], rs[c][b:e], terms, qd, G)
        else:
            acc = xs[c][b:e].copy()
            for tq, ts, tz in terms:
                acc = dequantize_grouped(tq, qd, BF16, e - b, G, ts, tz, O.ADD, prev=acc)
            q, s, z = quantize_grouped(acc, BF16, qd, G)
        final.append(dequantize_grouped(q, qd, BF16, e - b, G, s, z))
    return _assemble(xs, chunks, final), rs


def simulate_f32r(algorithm, xs, rs, qd, chunks, G, requantize):
    return (simulate_ring_f32r if algorithm == "ring" else simulate_direct_f32r)(xs, rs, qd, chunks, G, requantize)


def bf16_bits(t):
    """a CPU torch.bfloat16 tensor's bit patterns as a uint16 array (a copy)"""
    import torch

    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def bf16_tensor(bits):
    """uint16 bit patterns as a CPU torch.bfloat16 tensor"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


class GroupedEfF32rOracleOps(GroupedReduceEfOracleOps):
    """The grouped wire ops on CPU BFLOAT16 torch tensors through the oracle (nearest rounding), the error-feedback encodes with a FLOAT32
    residual.  bfloat16 moves through view(torch.int16).  The batch and reduce forms are the base classes': loops over the three ops below."""

    def _write(self, buf, lay, q, s, z):
        import torch

        rec = np.zeros(lay.nbytes, dtype=np.uint8)
        rec[: lay.zero_points_offset] = s.view(np.uint8)
        rec[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups] = z
        rec[lay.data_offset:] = q
        buf.copy_(torch.from_numpy(rec))

    def encode_grouped(self, x, buf, qdtype, round_mode, group_size):
        import torch

        assert x.dtype == torch.bfloat16
        qd = self._qd(qdtype)
        lay, _ = self._split(buf, x.numel(), qd, group_size)
        q, s, z = quantize_grouped(bf16_bits(x), BF16, qd, group_size)
        self._write(buf, lay, q, s, z)

    def decode_grouped(self, buf, out, qdtype, reduce_op, group_size):
        import torch

        assert out.dtype == torch.bfloat16
        qd = self._qd(qdtype)
        lay, raw = self._split(buf, out.numel(), qd, group_size)
        s = raw[: lay.zero_points_offset].copy().view(np.float32)
        z = raw[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups]
        res = dequantize_grouped(raw[lay.data_offset:], qd, BF16, out.numel(), group_size, s, z, O.ADD if reduce_op == "add" else O.SET, prev=bf16_bits(out))
        out.view(torch.int16).copy_(torch.from_numpy(res.view(np.int16)))

    def encode_grouped_ef(self, x, residual, buf, qdtype, round_mode, group_size):
        import torch

        assert x.dtype == torch.bfloat16 and residual.dtype == torch.float32
        qd = self._qd(qdtype)
        lay, _ = self._split(buf, x.numel(), qd, group_size)
        q, s, z, r_new, _, _ = ef_f32r_step(bf16_bits(x), residual.numpy(), qd, group_size)
        self._write(buf, lay, q, s, z)
        residual.copy_(torch.from_numpy(r_new))
