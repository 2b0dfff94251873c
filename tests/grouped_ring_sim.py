"""Reference simulation of piquant.distributed.quantized_all_reduce(group_size=G) for W ranks in one process, built from the CPU group model
(tests/grouped_model.py, i.e. the oracle group by group), and an oracle-backed stand-in for the grouped wire ops of piquant.distributed._DeviceOps.

Values are float32 arrays or bf16 bit patterns (uint16 arrays), as grouped_model takes them.  A chunk's partial sum is rounded to the tensor's
type after every term, which is what grouped dequantize ADD into the tensor's own chunk does."""
import numpy as np

import oracle as O
from grouped_model import dequantize_grouped, quantize_grouped


def _assemble(xs, chunks, final):
    out = [x.copy() for x in xs]
    for r in range(len(xs)):
        for c, (b, e) in enumerate(chunks):
            if e > b:
                out[r][b:e] = final[c]
    return out


def simulate_ring_grouped(xs, dt, qd, chunks, G):
    """The ring: chunk c is encoded by rank c, then ranks c + 1, ..., c + W - 1 add their own values to the decoded partial sum and re-encode it;
    the last of them owns the finished bytes, which every rank decodes (SET)."""
    W = len(xs)
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        q, s, z = quantize_grouped(xs[c][b:e], dt, qd, G)
        for j in range(1, W):
            acc = dequantize_grouped(q, qd, dt, e - b, G, s, z, O.ADD, prev=xs[(c + j) % W][b:e])
            q, s, z = quantize_grouped(acc, dt, qd, G)
        final.append(dequantize_grouped(q, qd, dt, e - b, G, s, z))
    return _assemble(xs, chunks, final)


def simulate_direct_grouped(xs, dt, qd, chunks, G):
    """The mesh: the owner of chunk c adds the decoded chunks of the other ranks to its own values in increasing rank order, encodes the sum once,
    and every rank decodes those bytes (SET)."""
    W = len(xs)
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        acc = xs[c][b:e].copy()
        for src in range(W):
            if src != c:
                q, s, z = quantize_grouped(xs[src][b:e], dt, qd, G)
                acc = dequantize_grouped(q, qd, dt, e - b, G, s, z, O.ADD, prev=acc)
        q, s, z = quantize_grouped(acc, dt, qd, G)
        final.append(dequantize_grouped(q, qd, dt, e - b, G, s, z))
    return _assemble(xs, chunks, final)


def round_trip_grouped(x, dt, qd, G):
    """What a one-rank all-reduce leaves: the grouped quantize / dequantize round trip of the tensor."""
    q, s, z = quantize_grouped(x, dt, qd, G)
    return dequantize_grouped(q, qd, dt, x.size, G, s, z)


class GroupedOracleOps:
    """The grouped wire ops of piquant.distributed on CPU float32 torch tensors through the oracle (nearest rounding): stands in for the HIP
    ops where there is no GPU.  Same wire records (piquant.distributed.grouped_wire_layout)."""

    def _qd(self, qdtype):
        import torch

        return {torch.uint8: O.UINT8, torch.quint8: O.UINT8, torch.quint4x2: O.UINT4, torch.quint2x4: O.UINT2}[qdtype]

    @staticmethod
    def _bits(qd):
        return {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}[qd]

    def _split(self, buf, numel, qd, G):
        import piquant.distributed as D

        lay = D.grouped_wire_layout(numel, G, self._bits(qd))
        raw = buf.numpy()
        assert raw.size == lay.nbytes, (raw.size, lay)
        return lay, raw

    def encode_grouped(self, x, buf, qdtype, round_mode, group_size):
        import torch

        qd = self._qd(qdtype)
        lay, _ = self._split(buf, x.numel(), qd, group_size)
        q, s, z = quantize_grouped(x.numpy(), O.F32, qd, group_size)
        rec = np.zeros(lay.nbytes, dtype=np.uint8)
        rec[: lay.zero_points_offset] = s.view(np.uint8)
        rec[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups] = z
        rec[lay.data_offset:] = q
        buf.copy_(torch.from_numpy(rec))

    def decode_grouped(self, buf, out, qdtype, reduce_op, group_size):
        import torch

        qd = self._qd(qdtype)
        lay, raw = self._split(buf, out.numel(), qd, group_size)
        s = raw[: lay.zero_points_offset].copy().view(np.float32)
        z = raw[lay.zero_points_offset: lay.zero_points_offset + lay.ngroups]
        res = dequantize_grouped(raw[lay.data_offset:], qd, O.F32, out.numel(), group_size, s, z, O.ADD if reduce_op == "add" else O.SET,
                                 prev=out.numpy().copy())
        out.copy_(torch.from_numpy(res))

    def encode_batch_grouped(self, xs, bufs, qdtype, round_mode, group_size):
        for x, buf in zip(xs, bufs):
            self.encode_grouped(x, buf, qdtype, round_mode, group_size)

    def decode_batch_grouped(self, bufs, outs, qdtype, reduce_op, group_size):
        for buf, out in zip(bufs, outs):
            self.decode_grouped(buf, out, qdtype, reduce_op, group_size)

    def reduce_encode_grouped(self, bufs, acc, buf, qdtype, round_mode, group_size):
        for b in bufs:
            self.decode_grouped(b, acc, qdtype, "add", group_size)
        self.encode_grouped(acc, buf, qdtype, round_mode, group_size)
