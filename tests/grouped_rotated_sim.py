"""CPU model of the two steps of a grouped collective in the rotated domain (include/piquant_hip.h, piquant_hip_reduce_quantize_grouped_rotated /
_dequantize_sum_grouped_rotated), made only from tests/rot_model.py, tests/grouped_model.py and tests/per_element_model.py; the simulation of
piquant.distributed's four collectives with rotation_seed= for W ranks in one process; and a model-backed stand-in for the rotated wire ops of
piquant.distributed._DeviceOps.

A term is (packed bytes, scales, zero points): a record of ROTATED values.  Values are float32 arrays or bf16 bit patterns (uint16 arrays)."""
import numpy as np

import oracle as O
import grouped_model as GM
import per_element_model as PE
import rot_model as RM
from grouped_scatter_sim import GroupedScatterOracleOps


def rotated_sum(acc, dt, terms, qd, G, seed):
    """y = rotate(widen(acc)) + the terms' float32 grouped dequantizes, added in order: one separately rounded float32 add each"""
    y = RM.rotate(RM.widen(acc, dt), G, seed)
    for q, s, z in terms:
        y = GM.dequantize_grouped(q, qd, O.F32, y.size, G, s, z, O.ADD, prev=y)
    return y


def reduce_quantize_grouped_rotated(acc, dt, terms, qd, G, seed, round_mode=O.NEAREST, threshold=0.0):
    """-> (packed bytes, scales, zero points): quantize_grouped (float32, computed parameters) of rotated_sum"""
    return GM.quantize_grouped(rotated_sum(acc, dt, terms, qd, G, seed), O.F32, qd, G, round_mode, threshold)


def reduce_quantize_grouped_rotated_per_element(acc, dt, terms, qd, G, seed, elem_seed, index_base):
    """the same in per-element stochastic mode: element i draws the threshold of index index_base + i"""
    return PE.quantize(rotated_sum(acc, dt, terms, qd, G, seed), O.F32, qd, G, elem_seed, index_base)


def terms_sum(terms, qd, n, G):
    """the first term stored, the others added in order, in float32"""
    q, s, z = terms[0]
    acc = GM.dequantize_grouped(q, qd, O.F32, n, G, s, z)
    for q, s, z in terms[1:]:
        acc = GM.dequantize_grouped(q, qd, O.F32, n, G, s, z, O.ADD, prev=acc)
    return acc


def dequantize_sum_grouped_rotated(terms, qd, dt_out, n, G, seed, reduce_op=O.SET, prev=None):
    """z = the float32 inverse rotation of terms_sum; SET converts z, ADD converts widen(prev) + z (one float32 add, one rounding)"""
    assert len(terms) >= 1
    z = RM.rotate(terms_sum(terms, qd, n, G), G, seed, inverse=True)
    if reduce_op == O.ADD:
        with np.errstate(over="ignore", invalid="ignore"):
            z = RM.widen(prev, dt_out) + z
    return z if dt_out == O.F32 else O.f32_to_bf16(z)


# ---- the four collectives with rotation_seed=, chunk by chunk (chunk c belongs to rank c in the mesh schedules) ----

def _decode(rec, qd, dt, n, G, seed):
    return RM.dequantize_grouped_rotated(rec[0], qd, dt, n, G, rec[1], rec[2], seed)


def _assemble(xs, chunks, final):
    out = [x.copy() for x in xs]
    for o in out:
        for c, (b, e) in enumerate(chunks):
            if e > b:
                o[b:e] = final[c]
    return out


def simulate_ring_rotated(xs, dt, qd, chunks, G, seed):
    """chunk c is encoded by rank c; ranks c + 1, .., c + W - 1 each fold their own values in with a one-term rotated reduce; every rank decodes
    the last one's bytes (SET)"""
    W = len(xs)
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        rec = RM.quantize_grouped_rotated(xs[c][b:e], dt, qd, G, seed)
        for j in range(1, W):
            rec = reduce_quantize_grouped_rotated(xs[(c + j) % W][b:e], dt, [rec], qd, G, seed)
        final.append(_decode(rec, qd, dt, e - b, G, seed))
    return _assemble(xs, chunks, final)


def simulate_direct_rotated(xs, dt, qd, chunks, G, seed):
    """the owner of chunk c adds the inverse rotation of the sum of the other ranks' records (increasing rank order) into its own values -- the
    reduce-scatter's step: the sum is in the tensor's type and the original domain --, encodes that with the rotated quantize, and every rank
    decodes those bytes (SET)"""
    W = len(xs)
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        terms = [RM.quantize_grouped_rotated(xs[src][b:e], dt, qd, G, seed) for src in range(W) if src != c]
        own = dequantize_sum_grouped_rotated(terms, qd, dt, e - b, G, seed, O.ADD, prev=xs[c][b:e]) if terms else xs[c][b:e]
        final.append(_decode(RM.quantize_grouped_rotated(own, dt, qd, G, seed), qd, dt, e - b, G, seed))
    return _assemble(xs, chunks, final)


def simulate_reduce_scatter_rotated(xs, dt, qd, chunks, G, seed):
    """rank r's result is its tensor with chunk r replaced by own + the inverse rotation of the sum of the peers' records (ADD)"""
    W = len(xs)
    out = [x.copy() for x in xs]
    for c, (b, e) in enumerate(chunks):
        if e == b or W == 1:
            continue
        terms = [RM.quantize_grouped_rotated(xs[src][b:e], dt, qd, G, seed) for src in range(W) if src != c]
        out[c][b:e] = dequantize_sum_grouped_rotated(terms, qd, dt, e - b, G, seed, O.ADD, prev=xs[c][b:e])
    return out


def simulate_all_gather_rotated(xs, dt, qd, chunks, G, seed):
    """chunk c of every rank's result is what rank c's chunk c decodes to"""
    final = [None if e == b else _decode(RM.quantize_grouped_rotated(xs[c][b:e], dt, qd, G, seed), qd, dt, e - b, G, seed)
             for c, (b, e) in enumerate(chunks)]
    return _assemble(xs, chunks, final)


class GroupedRotatedOracleOps(GroupedScatterOracleOps):
    """The rotated wire ops of piquant.distributed._DeviceOps on CPU float32 / bfloat16 torch tensors through the model above (nearest rounding),
    on top of the un-rotated stand-ins.  Same wire records (piquant.distributed.grouped_wire_layout)."""

    @staticmethod
    def _host(t):
        import torch

        if t.dtype == torch.bfloat16:
            return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy(), O.BF16
        return t.contiguous().numpy().copy(), O.F32

    @staticmethod
    def _store(out, values):
        import torch

        if out.dtype == torch.bfloat16:
            out.copy_(torch.from_numpy(values.view(np.int16).copy()).view(torch.bfloat16))
        else:
            out.copy_(torch.from_numpy(values))

    def _write(self, buf, numel, qd, G, rec):
        import torch

        lay, _ = self._split(buf, numel, qd, G)
        q, s, z = rec
        raw = np.zeros(lay.nbytes, dtype=np.uint8)
        raw[: lay.zero_points_offset] = s.view(np.uint8)
        raw[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups] = z
        raw[lay.data_offset:] = q
        buf.copy_(torch.from_numpy(raw))

    def _read(self, buf, numel, qd, G):
        lay, raw = self._split(buf, numel, qd, G)
        return (raw[lay.data_offset:].copy(), raw[: lay.zero_points_offset].copy().view(np.float32),
                raw[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups].copy())

    def encode_grouped_rotated(self, x, buf, qdtype, round_mode, group_size, seed):
        qd = self._qd(qdtype)
        v, dt = self._host(x)
        self._write(buf, x.numel(), qd, group_size, RM.quantize_grouped_rotated(v, dt, qd, group_size, seed))

    def decode_grouped_rotated(self, buf, out, qdtype, reduce_op, group_size, seed):
        qd = self._qd(qdtype)
        prev, dt = self._host(out)
        q, s, z = self._read(buf, out.numel(), qd, group_size)
        self._store(out, RM.dequantize_grouped_rotated(q, qd, dt, out.numel(), group_size, s, z, seed, O.ADD if reduce_op == "add" else O.SET, prev))

    def encode_batch_grouped_rotated(self, xs, bufs, qdtype, round_mode, group_size, seed):
        for x, buf in zip(xs, bufs):
            self.encode_grouped_rotated(x, buf, qdtype, round_mode, group_size, seed)

    def decode_batch_grouped_rotated(self, bufs, outs, qdtype, reduce_op, group_size, seed):
        for buf, out in zip(bufs, outs):
            self.decode_grouped_rotated(buf, out, qdtype, reduce_op, group_size, seed)

    def reduce_encode_grouped_rotated(self, bufs, acc, buf, qdtype, round_mode, group_size, seed):
        qd = self._qd(qdtype)
        v, dt = self._host(acc)
        terms = [self._read(b, acc.numel(), qd, group_size) for b in bufs]
        self._write(buf, acc.numel(), qd, group_size, reduce_quantize_grouped_rotated(v, dt, terms, qd, group_size, seed))

    def decode_sum_grouped_rotated(self, bufs, out, qdtype, reduce_op, group_size, seed):
        if bufs:
            qd = self._qd(qdtype)
            prev, dt = self._host(out)
            terms = [self._read(b, out.numel(), qd, group_size) for b in bufs]
            self._store(out, dequantize_sum_grouped_rotated(terms, qd, dt, out.numel(), group_size, seed,
                                                            O.ADD if reduce_op == "add" else O.SET, prev))
