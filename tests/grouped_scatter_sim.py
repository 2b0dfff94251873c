"""Reference simulation of piquant.distributed.quantized_reduce_scatter / quantized_all_gather for W ranks in one process, built from the CPU
group model (tests/grouped_model.py) and the error-feedback model (tests/ef_model.py), and the oracle-backed wire ops the two collectives
need on top of tests/grouped_ef_sim.py: decode_sum_grouped.

Chunk c belongs to rank c.  Reduce-scatter: every rank src != c encodes its values of chunk c (with error feedback: on its slice [b, e) of its
residual); the owner adds the decoded records to its own, unquantized values in increasing rank order -- the running sum rounded to the tensor's
type after every term -- and keeps the sum.  All-gather: the owner encodes its chunk (with error feedback: on its own slice of its residual)
and every rank, the owner included, decodes those bytes (SET)."""
import numpy as np

import oracle as O
from ef_model import ef_step, widen
from grouped_ef_sim import GroupedEfOracleOps
from grouped_model import dequantize_grouped, quantize_grouped


def _note(seen, *arrays, dt=O.F32):
    if seen is not None:
        for a in arrays:
            seen.append(float(np.abs(widen(a, dt)).max(initial=0.0)))


def simulate_reduce_scatter(xs, dt, qd, chunks, G, rs=None, seen=None):
    """-> (results, new residuals): rank r's result is its tensor with chunk r replaced by the sum; rs=None: no error feedback (residuals None).
    seen: a list that collects the largest magnitudes met (inputs + residual, decoded terms, partial sums)."""
    W = len(xs)
    rs = None if rs is None else [r.copy() for r in rs]
    out = [x.copy() for x in xs]
    for c, (b, e) in enumerate(chunks):
        if e == b:
            continue
        acc = xs[c][b:e].copy()
        for src in range(W):
            if src == c:
                continue
            if rs is None:
                q, s, z = quantize_grouped(xs[src][b:e], dt, qd, G)
            else:
                q, s, z, rs[src][b:e], y, d = ef_step(xs[src][b:e], rs[src][b:e], dt, qd, G)
                _note(seen, y, d, dt=dt)
            acc = dequantize_grouped(q, qd, dt, e - b, G, s, z, O.ADD, prev=acc)
            _note(seen, acc, dt=dt)
        out[c][b:e] = acc
    return out, rs


def simulate_all_gather(xs, dt, qd, chunks, G, rs=None):
    """-> (results, new residuals): chunk c of every rank's result is what rank c's chunk c decodes to; all ranks end identical."""
    rs = None if rs is None else [r.copy() for r in rs]
    out = [x.copy() for x in xs]
    for c, (b, e) in enumerate(chunks):
        if e == b:
            continue
        if rs is None:
            q, s, z = quantize_grouped(xs[c][b:e], dt, qd, G)
        else:
            q, s, z, rs[c][b:e], _, _ = ef_step(xs[c][b:e], rs[c][b:e], dt, qd, G)
        final = dequantize_grouped(q, qd, dt, e - b, G, s, z)
        for o in out:
            o[b:e] = final
    return out, rs


class GroupedScatterOracleOps(GroupedEfOracleOps):
    """GroupedOracleOps (through GroupedEfOracleOps, for the error-feedback encodes) plus decode_sum_grouped, on CPU float32 torch tensors."""

    def decode_sum_grouped(self, bufs, out, qdtype, reduce_op, group_size):
        for i, b in enumerate(bufs):
            self.decode_grouped(b, out, qdtype, reduce_op if i == 0 else "add", group_size)
