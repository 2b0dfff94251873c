"""Inputs, seeds and index bases of the per-element tests of the grouped kernels; numpy only.  tests/test_per_element_model_cpu.py proves on the
host that they separate every fault model of tests/per_element_model.py from the right model, tests/test_gpu_grouped_per_element.py runs them
on the device.

Data: normal with a magnitude that changes every 97 elements, a few outliers a hundred times larger and two NaNs.  The size of a single call is
3 chunks + G + 5 of the pair's tile: full chunks, a ragged last chunk and a ragged last group.  The bases put index 2^32 at every kind of
place of that tensor; the last one is far above 2^32 from the first element on and runs with a seed whose upper half is not zero."""
import functools

import numpy as np

import oracle as O
import per_element_model as M
from ef_model import add_t, widen
from grouped_model import PACK, QMAX, group_params_all

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
QDS = [O.UINT8, O.UINT4, O.UINT2]
GROUP_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
SOME_G = [32, 128, 4096]
SEED_LOW = 0x9E3779B9                 # upper half zero
SEED_FULL = 0xC0FFEE12_3456789B       # upper half not zero
BATCH = 19
REDUCE_TERMS = (0, 1, 7, 17)          # of reduce_quantize_grouped; 17 takes the surplus path
REDUCE_EF_TERMS = (1, 7)              # of reduce_quantize_grouped_ef
CAPTURE = (O.BF16, O.UINT4, 128)      # the pair and group size of the graph-capture test


# The ragged last chunk is G + 5 elements: where index 2^32 falls into it, a fault model of the key switch (g, h) changes the threshold of as few as
# one to seven elements, and a draw of the data can leave all their codes as they were.  The draws of these tiles (input type, quantized type,
# group size, elements per vector of the tile) take the first salt with which tests/test_per_element_model_cpu.py passes; every other tile takes 0.
SALTS = {(0, 4, 256, 4): 15, (0, 4, 512, 4): 14, (0, 3, 128, 4): 2, (0, 3, 256, 4): 12, (0, 3, 512, 4): 1, (0, 3, 1024, 4): 4, (0, 3, 2048, 4): 3,
         (0, 2, 256, 4): 5, (0, 2, 1024, 4): 3, (1, 4, 512, 8): 90, (1, 4, 1024, 8): 24, (1, 4, 2048, 8): 1, (1, 4, 4096, 8): 1, (1, 3, 512, 8): 28,
         (1, 2, 512, 8): 8, (1, 2, 1024, 8): 37, (1, 4, 512, 4): 2, (1, 3, 256, 4): 7, (1, 3, 512, 4): 2, (1, 2, 256, 4): 5, (1, 2, 512, 4): 8,
         (1, 2, 1024, 4): 5}


BATCH_SALTS = {(0, 4, 128, 4): 2, (0, 3, 128, 4): 1, (0, 2, 32, 4): 1, (1, 4, 32, 8): 1, (1, 3, 32, 8): 2}   # the same for the members of a batch


def size_of(t):
    return 3 * t.chunk + t.G + 5


def bases(t):
    """[(name, index_base, seed)] for a tensor of size_of(t) elements on tile t; check_bases asserts what the names say"""
    n, row = size_of(t), 64 * t.epv
    at = {"row 0": t.chunk + 5 * t.epv + 1,                             # chunk 1, row 0, lane 5, element 1 of the vector
          "last row": t.chunk + (t.NV - 1) * row + 9 * t.epv + 2,       # chunk 1, last row, lane 9, element 2
          "chunk boundary": 2 * t.chunk,
          "ragged chunk": n // t.chunk * t.chunk + 1}                   # element 1 of the ragged chunk's first vector
    return [(k, 2 ** 32 - x, SEED_LOW) for k, x in at.items()] + [("above", 2 ** 33 + 12345, SEED_FULL)]


def check_bases(t):
    n = size_of(t)
    full = n // t.chunk   # 3, or 4 where a chunk is a single group
    assert full == 3 + (t.NG == 1) and n % t.chunk == (t.G + 5) % t.chunk >= 5 and n % t.G == 5
    found = {}
    for name, base, seed in bases(t):
        x = 2 ** 32 - base          # the element whose index is 2^32
        if name == "above":
            assert base >> 32 == (base + n - 1) >> 32 == 2 and seed >> 32 != 0
            continue
        assert 0 < x < n and seed >> 32 == 0
        c = t.coords(x)
        found[name] = c
        if name == "row 0":
            assert c["chunk"] in (1, 2) and c["row"] == 0 and 0 < c["elem"] < t.epv
        elif name == "last row":
            assert c["chunk"] in (1, 2) and c["row"] == t.NV - 1 and 0 < c["elem"] < t.epv
        elif name == "chunk boundary":
            assert x % t.chunk == 0 and 0 < x // t.chunk <= 3
        else:
            assert c["chunk"] == full and x % t.chunk != 0
    assert len(found) == 4
    return found


def _narrow(xf, dt):
    return O.f32_to_bf16(xf) if dt == O.BF16 else xf


def make_input(n, dt, seed, nans=True):
    """-> (x, a second tensor of the same magnitude: an accumulator or, scaled down, a residual)"""
    rng = np.random.default_rng(seed)
    mag = np.repeat(rng.uniform(0.01, 50.0, n // 97 + 1), 97)[:n]
    xf = (rng.standard_normal(n) * mag).astype(np.float32)
    if n > 10:
        xf[rng.choice(n, max(1, n // 5000), replace=False)] *= 100.0
        if nans:
            xf[[7, n // 2 + 1]] = np.nan
    af = (rng.standard_normal(n) * mag * 0.7 + 0.3).astype(np.float32)
    return _narrow(xf, dt), _narrow(af, dt)


def make_terms(k, n, qd, G, seed):
    """k packed terms of random codes with their own per-group parameters; the bits behind the tensor's end are zero, as every quantize call leaves them"""
    rng = np.random.default_rng([seed, k, qd, G])
    ng = (n + G - 1) // G
    terms = []
    for _ in range(k):
        q = rng.integers(0, 256, O.packed_numel(n, qd)).astype(np.uint8)
        if n % PACK[qd]:
            q[-1] &= (1 << ((n % PACK[qd]) * M.BITS[qd])) - 1
        terms.append((q, rng.uniform(0.001, 0.5, ng).astype(np.float32), rng.integers(0, QMAX[qd] + 1, ng).astype(np.uint8)))
    return tuple(terms)


def residual_from(a, dt, kind):
    """a small residual out of the second tensor of make_input: of the tensor's type ("same") or float32 ("mixed")"""
    r32 = (widen(a, dt) * np.float32(0.01)).astype(np.float32)
    return _narrow(r32, dt) if kind == "same" else r32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def single(dt, qd, G, dt_tile=None):
    """-> (x, second tensor, n) of the single calls of the pair on the tile of dt_tile (None: dt)"""
    t = M.tile(dt if dt_tile is None else dt_tile, qd, G)
    n = size_of(t)
    x, a = _frozen(*make_input(n, dt, [G, qd, dt, n, SALTS.get((dt, qd, G, t.epv), 0)]))
    return x, a, n


@functools.lru_cache(maxsize=None)
def ef_inputs(kind, dt, qd, G):
    """kind "same": residual of the tensor's type; "mixed": dt is bfloat16 and the residual float32 -> (x, r, dt_tile)"""
    assert kind == "same" or dt == O.BF16
    dt_tile = dt if kind == "same" else O.F32
    x, a, n = single(dt, qd, G, dt_tile)
    r, = _frozen(residual_from(a, dt, kind))
    return x, r, dt_tile


@functools.lru_cache(maxsize=None)
def terms_for(dt, qd, G, k, dt_tile=None):
    n = single(dt, qd, G, dt_tile)[2]
    terms = make_terms(k, n, qd, G, 11)
    for t in terms:
        _frozen(*t)
    return terms


@functools.lru_cache(maxsize=None)
def given_params(dt, qd, G):
    """parameters to quantize with that are not the data's own: every scale a quarter larger (nothing saturates)"""
    x = single(dt, qd, G)[0]
    s, z = group_params_all(widen(x, dt), G, qd)
    return _frozen(s * np.float32(1.25), z)


def batch_numels(t):
    """19 members: an empty one (4), a one-element one (9), one of 5 chunks + 3 (2), the single calls' size (0); member 7 is the misaligned one"""
    c, G = t.chunk, t.G
    ns = [size_of(t), c, 5 * c + 3, G, 0, c + 1, 2 * G + 1, G + 3, c - 1, 1, 31, 2 * c, G - 1, 3 * G, c + G, 17, 2 * c + 5, 5 * G + 7, c // 2 + 1]
    assert len(ns) == BATCH
    return ns


MISALIGNED_MEMBER = 7


@functools.lru_cache(maxsize=None)
def batch_inputs(dt, qd, G, dt_tile=None):
    """-> [(x, second tensor)] of the batch's members"""
    t = M.tile(dt if dt_tile is None else dt_tile, qd, G)
    salt = BATCH_SALTS.get((dt, qd, G, t.epv), 0)
    return [_frozen(*make_input(n, dt, [G, qd, dt, i, 77, salt], nans=i % 3 == 0)) for i, n in enumerate(batch_numels(t))]


def batch_chunk_begins(t):
    """chunk_begin of every member as the host's launches see it: empty members and the misaligned one are not in a launch, and a launch takes 16"""
    out, chunks, count = [], 0, 0
    for i, n in enumerate(batch_numels(t)):
        if n == 0 or i == MISALIGNED_MEMBER:
            out.append(0)
            continue
        out.append(chunks)
        chunks += (n + t.chunk - 1) // t.chunk
        count += 1
        if count == 16:
            chunks = count = 0
    return out


def capture_replay_inputs():
    """-> (x, residual) that the graph-capture test replays on: fresh data of the captured call's size"""
    dt, qd, G = CAPTURE
    n = single(dt, qd, G)[2]
    x, a = make_input(n, dt, [n, 991])
    return x, residual_from(a, dt, "same")


def capture_stages():
    """the inputs of the quantize step of the two captured calls at replay, as quantize_stages yields them; they run with bases(t)[0] only"""
    dt, qd, G = CAPTURE
    x, r = capture_replay_inputs()
    yield "captured quantize_grouped", x, dt, dt, qd, G, None, 0
    yield "captured quantize_grouped_ef", add_t(x, r, dt), dt, dt, qd, G, None, 0


def quantize_stages(pairs=PAIRS, mixed_qds=QDS, group_sizes=GROUP_SIZES):
    """Every distinct input of the quantize step among the cases of tests/test_gpu_grouped_per_element.py (same-type calls of `pairs`, the
    bfloat16 calls with a float32 residual of `mixed_qds`): yields (what, y, type of y, tile's type, qd, G, given parameters or None, chunk_begin)"""
    for dt, qd in pairs:
        for G in group_sizes:
            x, r, _ = ef_inputs("same", dt, qd, G)
            yield f"ef same dt={dt} qd={qd} G={G}", add_t(x, r, dt), dt, dt, qd, G, None, 0
            x = single(dt, qd, G)[0]
            yield f"qdq dt={dt} qd={qd} G={G}", x, dt, dt, qd, G, None, 0
            yield f"qdq given dt={dt} qd={qd} G={G}", x, dt, dt, qd, G, given_params(dt, qd, G), 0
        for G in [g for g in SOME_G if g in group_sizes]:
            x, a, _ = single(dt, qd, G)
            r = ef_inputs("same", dt, qd, G)[1]
            for k in REDUCE_TERMS:
                acc = M.add_terms(x, terms_for(dt, qd, G, k), dt, qd, G)
                yield f"reduce dt={dt} qd={qd} G={G} k={k}", acc, dt, dt, qd, G, None, 0
                if k in REDUCE_EF_TERMS:
                    yield f"reduce ef same dt={dt} qd={qd} G={G} k={k}", add_t(acc, r, dt), dt, dt, qd, G, None, 0
            t = M.tile(dt, qd, G)
            for i, ((x, a), cb) in enumerate(zip(batch_inputs(dt, qd, G), batch_chunk_begins(t))):
                yield f"batch dt={dt} qd={qd} G={G} member {i}", x, dt, dt, qd, G, None, cb
                r = residual_from(a, dt, "same")
                yield f"ef batch dt={dt} qd={qd} G={G} member {i}", add_t(x, r, dt), dt, dt, qd, G, None, cb
    for qd in mixed_qds:
        for G in group_sizes:
            x, r, _ = ef_inputs("mixed", O.BF16, qd, G)
            yield f"ef mixed qd={qd} G={G}", add_t(widen(x, O.BF16), r, O.F32), O.F32, O.F32, qd, G, None, 0
        for G in [g for g in SOME_G if g in group_sizes]:
            x, r, _ = ef_inputs("mixed", O.BF16, qd, G)
            for k in REDUCE_EF_TERMS:
                acc = M.add_terms(x, terms_for(O.BF16, qd, G, k, O.F32), O.BF16, qd, G)
                yield f"reduce ef mixed qd={qd} G={G} k={k}", add_t(widen(acc, O.BF16), r, O.F32), O.F32, O.F32, qd, G, None, 0
            t = M.tile(O.F32, qd, G)
            for i, ((x, a), cb) in enumerate(zip(batch_inputs(O.BF16, qd, G, O.F32), batch_chunk_begins(t))):
                r = residual_from(a, O.BF16, "mixed")
                yield f"ef mixed batch qd={qd} G={G} member {i}", add_t(widen(x, O.BF16), r, O.F32), O.F32, O.F32, qd, G, None, cb
