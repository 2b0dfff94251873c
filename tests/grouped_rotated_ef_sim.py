"""The simulation of piquant.distributed's four collectives with rotated_error_feedback= for W ranks in one process, and a model-backed stand-in
for the three wire ops they add to piquant.distributed._DeviceOps.  Made only from tests/rot_ef_model.py, tests/rot_model.py and
tests/grouped_rotated_sim.py: no arithmetic of its own.

xs[r] is rank r's tensor (float32 array, or bf16 bit patterns), rs[r] its residual: a float32 array of rotated values.  Every simulation returns
(the ranks' results, the ranks' new residuals) and modifies neither input."""
import numpy as np

import oracle as O
import grouped_rotated_sim as S
import rot_ef_model as RE
import rot_model as RM


def _encode_ef(x, dt, r, b, e, qd, G, seed):
    """rank-local encode of [b, e) with error feedback: -> the record; r[b:e] is replaced"""
    q, s, z, new, _, _ = RE.quantize_grouped_rotated_ef(x[b:e], dt, r[b:e], qd, G, seed)
    r[b:e] = new
    return q, s, z


def simulate_ring_rotated_ef(xs, rs, dt, qd, chunks, G, seed, requantize):
    """simulate_ring_rotated with the residual: rank c's first encode of chunk c feeds its chunk c; with `requantize` every hop feeds the hop's
    chunk of the folding rank's residual"""
    W = len(xs)
    rs = [r.copy() for r in rs]
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        rec = _encode_ef(xs[c], dt, rs[c], b, e, qd, G, seed)
        for j in range(1, W):
            k = (c + j) % W
            if requantize:
                q, s, z, new, _, _ = RE.reduce_quantize_grouped_rotated_ef(xs[k][b:e], dt, rs[k][b:e], [rec], qd, G, seed)
                rs[k][b:e] = new
                rec = (q, s, z)
            else:
                rec = S.reduce_quantize_grouped_rotated(xs[k][b:e], dt, [rec], qd, G, seed)
        final.append(S._decode(rec, qd, dt, e - b, G, seed))
    return S._assemble(xs, chunks, final), rs


def _scatter(xs, rs, dt, qd, chunks, G, seed):
    """the mesh's first half: -> (per chunk c: own values + the inverse rotation of the sum of the peers' records, or None), residuals fed"""
    W = len(xs)
    own = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            own.append(None)
            continue
        terms = [_encode_ef(xs[src], dt, rs[src], b, e, qd, G, seed) for src in range(W) if src != c]
        own.append(S.dequantize_sum_grouped_rotated(terms, qd, dt, e - b, G, seed, O.ADD, prev=xs[c][b:e]) if terms else xs[c][b:e].copy())
    return own


def simulate_direct_rotated_ef(xs, rs, dt, qd, chunks, G, seed, requantize):
    """simulate_direct_rotated with the residual: the peers' chunks feed the encoding ranks' residuals; the owner's encode feeds its own chunk
    only with `requantize`"""
    rs = [r.copy() for r in rs]
    own = _scatter(xs, rs, dt, qd, chunks, G, seed)
    final = []
    for c, (b, e) in enumerate(chunks):
        if e == b:
            final.append(None)
            continue
        if requantize:
            q, s, z, new, _, _ = RE.quantize_grouped_rotated_ef(own[c], dt, rs[c][b:e], qd, G, seed)
            rs[c][b:e] = new
            rec = (q, s, z)
        else:
            rec = RM.quantize_grouped_rotated(own[c], dt, qd, G, seed)
        final.append(S._decode(rec, qd, dt, e - b, G, seed))
    return S._assemble(xs, chunks, final), rs


def simulate_reduce_scatter_rotated_ef(xs, rs, dt, qd, chunks, G, seed):
    rs = [r.copy() for r in rs]
    own = _scatter(xs, rs, dt, qd, chunks, G, seed)
    out = [x.copy() for x in xs]
    for c, (b, e) in enumerate(chunks):
        if e > b:
            out[c][b:e] = own[c]
    return out, rs


def simulate_all_gather_rotated_ef(xs, rs, dt, qd, chunks, G, seed):
    rs = [r.copy() for r in rs]
    final = [None if e == b else S._decode(_encode_ef(xs[c], dt, rs[c], b, e, qd, G, seed), qd, dt, e - b, G, seed) for c, (b, e) in enumerate(chunks)]
    return S._assemble(xs, chunks, final), rs


class GroupedRotatedEfOracleOps(S.GroupedRotatedOracleOps):
    """encode_grouped_rotated_ef / encode_batch_grouped_rotated_ef / reduce_encode_grouped_rotated_ef of piquant.distributed._DeviceOps on CPU
    tensors through tests/rot_ef_model.py (nearest rounding); the residual is a float32 torch tensor, updated in place."""

    @staticmethod
    def _update(residual, new):
        import torch

        residual.copy_(torch.from_numpy(np.ascontiguousarray(new)))

    def encode_grouped_rotated_ef(self, x, residual, buf, qdtype, round_mode, group_size, seed):
        qd = self._qd(qdtype)
        v, dt = self._host(x)
        q, s, z, new, _, _ = RE.quantize_grouped_rotated_ef(v, dt, residual.contiguous().numpy().copy(), qd, group_size, seed)
        self._write(buf, x.numel(), qd, group_size, (q, s, z))
        self._update(residual, new)

    def encode_batch_grouped_rotated_ef(self, xs, residuals, bufs, qdtype, round_mode, group_size, seed):
        for x, r, buf in zip(xs, residuals, bufs):
            self.encode_grouped_rotated_ef(x, r, buf, qdtype, round_mode, group_size, seed)

    def reduce_encode_grouped_rotated_ef(self, bufs, acc, residual, buf, qdtype, round_mode, group_size, seed):
        qd = self._qd(qdtype)
        v, dt = self._host(acc)
        terms = [self._read(b, acc.numel(), qd, group_size) for b in bufs]
        q, s, z, new, _, _ = RE.reduce_quantize_grouped_rotated_ef(v, dt, residual.contiguous().numpy().copy(), terms, qd, group_size, seed)
        self._write(buf, acc.numel(), qd, group_size, (q, s, z))
        self._update(residual, new)
