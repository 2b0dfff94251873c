"""CPU model of the grouped calls in per-element stochastic mode (RM_STOCH_ELEM), made only from the oracle's quantize_per_element and the group
model (tests/grouped_model.py), and the same model with the element index computed WRONGLY in one way (the fault models).

The definition (include/piquant_hip.h: "per-element mode indexes the global element"): element i of a tensor draws the threshold of the 64-bit
index index_base + i, so group g = [b, e) of the tensor is O.quantize_per_element(x[b:e], dt, qd, s_g, z_g, seed, index_base + b), the groups
laid end to end.  Everything else -- dequantize, the error-feedback steps, the reduce, quantize-dequantize -- is the composition the other
models use (tests/ef_model.py, tests/ef_f32r_model.py), with that quantize in the middle.  A batch is the list of its members' single models,
each from index_base + 0 ("in per-element mode every tensor indexes its own elements from 0").

A window [start, start + x.size) of a longer tensor is modelled with `start` (a multiple of the group size): the large-tensor tests copy only
windows to the host.

Fault models.  Each is an index map i -> 64-bit threshold index that a kernel or a host path could compute instead of index_base + i; the chunk
geometry (elements per vector, rows per lane, elements per chunk) is the restatement tests/extremum_positions.py keeps (GroupedTile), which
tests/test_extremum_positions_cpu.py checks against the headers:
  a  index_base ignored                                   i
  b  index relative to the group                          index_base + i mod G
  c  index relative to the chunk                          index_base + i mod chunk
  d  a batch member's index continued from the previous member: index_base + chunk_begin * chunk + i (chunk_begin: chunks of the members before it)
  e  the element index truncated to 32 bits before the base is added
  f  the sum truncated to 32 bits
  g  the key never switched at a multiple of 2^32: every element of a lane takes the upper half of the lane's FIRST index in the chunk
  h  the key switched by the lane's first row only: element e of row r takes the upper half of element e of the lane's row 0
  i  index off by one element
  j  index off by one vector (4 or 8 elements)
  k  index off by one row (64 vectors)
A fault APPLIES to a case when its map differs from the right one somewhere in the case; tests/test_per_element_model_cpu.py proves that every
fault that applies to a case of tests/per_element_cases.py changes the packed bytes, so a kernel with that fault fails the GPU tests.
"""
import numpy as np

import oracle as O
import ef_f32r_model
import ef_model
from ef_model import widen
from extremum_positions import GroupedTile
from grouped_model import PACK, dequantize_grouped, group_params_all, groups

BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
ESIZE = {O.F32: 4, O.BF16: 2}
FAULTS = tuple("abcdefghijk")
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


def tile(dt_tile, qd, G):
    """the streaming tile of the pair: dt_tile is the input's type, or float32 for a bfloat16 tensor with a float32 residual"""
    return GroupedTile(G, ESIZE[dt_tile], BITS[qd])


def unpack(q, qd, n):
    """packed bytes -> one code per element (low bits = lower element index)"""
    per, bits = PACK[qd], BITS[qd]
    c = (q[:, None] >> (np.arange(per, dtype=np.uint8) * bits)[None, :]) & np.uint8((1 << bits) - 1)
    return c.reshape(-1)[:n]


def pack(codes, qd):
    per, bits = PACK[qd], BITS[qd]
    c = np.zeros((codes.size + per - 1) // per * per, dtype=np.uint8)
    c[: codes.size] = codes
    out = np.zeros(c.size // per, dtype=np.uint8)
    for j in range(per):
        out |= c[j::per] << np.uint8(j * bits)
    return out


def index_map(n, index_base, t: GroupedTile, fault=None, start=0, chunk_begin=0):
    """uint64[n]: the threshold index of tensor elements start .. start + n - 1 -- the right one (fault None) or a fault model's"""
    i = np.arange(start, start + n, dtype=np.uint64)
    base = np.uint64(index_base & M64)
    right = base + i   # wraps modulo 2^64, as the kernels' uint64_t does
    if fault is None:
        return right
    if fault == "a":
        return i
    if fault == "b":
        return base + i % np.uint64(t.G)
    if fault == "c":
        return base + i % np.uint64(t.chunk)
    if fault == "d":
        return right + np.uint64(chunk_begin * t.chunk)
    if fault == "e":
        return base + (i & np.uint64(M32))
    if fault == "f":
        return right & np.uint64(M32)
    if fault in ("g", "h"):
        in_chunk = i % np.uint64(t.chunk)
        lane_first = i - in_chunk + (in_chunk // np.uint64(t.epv)) % np.uint64(64) * np.uint64(t.epv)   # element 0 of the lane's row 0
        src = base + lane_first + (in_chunk % np.uint64(t.epv) if fault == "h" else np.uint64(0))
        return (src >> np.uint64(32) << np.uint64(32)) | (right & np.uint64(M32))
    step = {"i": 1, "j": t.epv, "k": 64 * t.epv}[fault]
    return right + np.uint64(step)


def applies(n, index_base, t, fault, start=0, chunk_begin=0):
    """does the fault's index differ from the right one for some element of the case"""
    return bool(np.any(index_map(n, index_base, t, fault, start, chunk_begin) != index_map(n, index_base, t, None, start)))


def quantize(x, dt, qd, G, seed, index_base, params=None, fault=None, dt_tile=None, start=0, chunk_begin=0):
    """-> (packed bytes, scales, zero points) of quantize_grouped in per-element mode; `params` = (scales, zero_points) given instead of computed.
    fault None: the definition, group by group.  Otherwise the fault model's index map, run by run of consecutive indices."""
    assert start % G == 0
    n = x.size
    s, z = group_params_all(widen(x, dt), G, qd) if params is None else params
    if fault is None:
        parts = [O.quantize_per_element(x[b:e], dt, qd, float(s[g]), int(z[g]), seed, (index_base + start + b) & M64) for g, (b, e) in enumerate(groups(n, G))]
        return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), s, z
    idx = index_map(n, index_base, tile(dt if dt_tile is None else dt_tile, qd, G), fault, start, chunk_begin)
    cut = np.flatnonzero(idx[1:] != idx[:-1] + np.uint64(1)) + 1
    edges = np.unique(np.concatenate([np.arange(0, n, G), cut, [n]])) if n else np.zeros(1, dtype=np.int64)
    codes = np.empty(n, dtype=np.uint8)
    for a, b in zip(edges[:-1], edges[1:]):
        g = a // G
        codes[a:b] = unpack(O.quantize_per_element(x[a:b], dt, qd, float(s[g]), int(z[g]), seed, int(idx[a])), qd, b - a)
    return pack(codes, qd), s, z


def add_terms(acc, terms, dt, qd, G):
    """acc <- acc + d_i rounded to the accumulator's type, term by term: grouped dequantize ADD through the oracle"""
    acc = acc.copy()
    for q, s, z in terms:
        acc = dequantize_grouped(q, qd, dt, acc.size, G, s, z, O.ADD, prev=acc)
    return acc


def _rounding(dt, qd, G, seed, index_base, fault, start, chunk_begin):
    """the per-element quantize as the `quantize` of tests/ef_model.py's ef_step: (y, scales, zero points) -> packed bytes"""
    return lambda y, s, z: quantize(y, dt, qd, G, seed, index_base, (s, z), fault, start=start, chunk_begin=chunk_begin)[0]


def ef_step(x, r, dt, qd, G, seed, index_base, fault=None, start=0, chunk_begin=0):
    """quantize_grouped_ef with a residual of the tensor's type -> (packed bytes, scales, zero points, new residual): tests/ef_model.py's step
    with the per-element quantize in its middle"""
    return ef_model.ef_step(x, r, dt, qd, G, quantize=_rounding(dt, qd, G, seed, index_base, fault, start, chunk_begin))[:4]


def ef_f32r_step(x_bf16, r_f32, qd, G, seed, index_base, fault=None, start=0, chunk_begin=0):
    """quantize_grouped_ef of a bfloat16 tensor with a float32 residual: tests/ef_f32r_model.py's step with the per-element quantize in its middle"""
    return ef_f32r_model.ef_f32r_step(x_bf16, r_f32, qd, G, quantize=_rounding(O.F32, qd, G, seed, index_base, fault, start, chunk_begin))[:4]


def reduce(acc, terms, dt, qd, G, seed, index_base, fault=None, start=0):
    """reduce_quantize_grouped -> (packed bytes, scales, zero points)"""
    return quantize(add_terms(acc, terms, dt, qd, G), dt, qd, G, seed, index_base, fault=fault, start=start)


def reduce_ef(acc, r, terms, dt, qd, G, seed, index_base, fault=None, start=0):
    """reduce_quantize_grouped_ef, residual of the accumulator's type -> (packed bytes, scales, zero points, new residual)"""
    return ef_step(add_terms(acc, terms, dt, qd, G), r, dt, qd, G, seed, index_base, fault, start)


def reduce_ef_f32r_per_element_model(acc, r, terms, qd, G, seed, index_base, fault=None, start=0):
    """reduce_quantize_grouped_ef of a bfloat16 accumulator with a float32 residual -> (packed bytes, scales, zero points, new residual)"""
    return ef_f32r_step(add_terms(acc, terms, O.BF16, qd, G), r, qd, G, seed, index_base, fault, start)


def quantize_dequantize(x, dt, qd, G, seed, index_base, params=None, prev=None, fault=None, start=0, chunk_begin=0):
    """quantize_dequantize_grouped -> (out, scales, zero points); prev: the accumulator of ADD (copied), None: SET"""
    q, s, z = quantize(x, dt, qd, G, seed, index_base, params, fault, start=start, chunk_begin=chunk_begin)
    return dequantize_grouped(q, qd, dt, x.size, G, s, z, O.SET if prev is None else O.ADD, prev), s, z

