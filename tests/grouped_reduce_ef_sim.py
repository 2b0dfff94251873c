"""Reference for error feedback on RE-quantized partial sums (piquant_hip_reduce_quantize_grouped_ef and
quantized_all_reduce(..., error_feedback_requantize=True)), built from the group model and the error-feedback model.

One owner / hop step, with T the accumulator's type:
  1. for every term in order: acc <- grouped dequantize ADD of the term into acc (the running sum rounded to T after each term)
  2. ef_step(acc, r): y = rn_T(acc + r), quantize_grouped(y), r <- rn_T(y - d)
The schedules are those of tests/grouped_ef_sim.py with the residual on EVERY quantization: the mesh owner's on its own chunk of its residual,
every hop of the ring on the hop's chunk of the hopping rank's residual."""
import numpy as np

import oracle as O
from ef_model import ef_step, widen
from grouped_ef_sim import GroupedEfOracleOps
from grouped_model import dequantize_grouped
from grouped_ring_sim import _assemble


def reduce_ef_step(acc, r, terms, dt, qd, G, round_mode=O.NEAREST, threshold=0.0, seen=None):
    """terms: [(packed bytes, scales, zero points), ...] -> (packed bytes, scales, zero points, new residual, y, d); acc and r are not modified."""
    acc = acc.copy()
    for q, s, z in terms:
        acc = dequantize_grouped(q, qd, dt, acc.size, G, s, z, O.ADD, prev=acc)
        _see(seen, dt, acc)
    return ef_step(acc, r, dt, qd, G, round_mode, threshold)


def _see(seen, dt, *arrays):
    if seen is not None:
        for a in arrays:
            seen.append(float(np.abs(widen(a, dt)).max(initial=0.0)))


def simulate_ring_grouped_ef_all(xs, rs, dt, qd, chunks, G, seen=None):
    """The ring with the residual on every quantization: chunk c is first encoded by rank c on its slice of its residual, then rank c + j
    (j = 1 .. W - 1) adds its own values to the decoded partial sum, adds ITS slice [b, e) of ITS residual, re-encodes and keeps what that lost.
    -> (results, new residuals).  `seen` collects the largest magnitudes of partial sums, y and d."""
    W = len(xs)
    rs = [r.copy() for r in rs]
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        q, s, z, rs[c][b:e], y, d = ef_step(xs[c][b:e], rs[c][b:e], dt, qd, G)
        _see(seen, dt, y, d)
        for j in range(1, W):
            k = (c + j) % W
            q, s, z, rs[k][b:e], y, d = reduce_ef_step(xs[k][b:e], rs[k][b:e], [(q, s, z)], dt, qd, G, seen=seen)
            _see(seen, dt, y, d)
        final.append(dequantize_grouped(q, qd, dt, e - b, G, s, z))
    return _assemble(xs, chunks, final), rs


def simulate_direct_grouped_ef_all(xs, rs, dt, qd, chunks, G, seen=None):
    """The mesh with the residual on every quantization: every rank src != c encodes its chunk c on its slice of its residual; the owner adds the
    decoded chunks to its own values in increasing rank order, then its OWN slice of its residual, encodes once and keeps what that lost."""
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
                q, s, z, rs[src][b:e], y, d = ef_step(xs[src][b:e], rs[src][b:e], dt, qd, G)
                _see(seen, dt, y, d)
                terms.append((q, s, z))
        q, s, z, rs[c][b:e], y, d = reduce_ef_step(xs[c][b:e], rs[c][b:e], terms, dt, qd, G, seen=seen)
        _see(seen, dt, y, d)
        final.append(dequantize_grouped(q, qd, dt, e - b, G, s, z))
    return _assemble(xs, chunks, final), rs


class GroupedReduceEfOracleOps(GroupedEfOracleOps):
    """GroupedEfOracleOps plus the error-feedback re-quantization, on CPU float32 torch tensors (nearest rounding)."""

    def reduce_encode_grouped_ef(self, bufs, acc, residual, buf, qdtype, round_mode, group_size):
        for b in bufs:
            self.decode_grouped(b, acc, qdtype, "add", group_size)
        self.encode_grouped_ef(acc, residual, buf, qdtype, round_mode, group_size)
