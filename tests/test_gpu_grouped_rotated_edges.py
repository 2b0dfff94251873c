"""The rotated grouped calls on the MI355X at their edges: piquant.torch.hadamard_grouped / quantize_grouped_rotated / dequantize_grouped_rotated
against the CPU model (tests/rot_model.py), bit for bit -- NaN positions are compared, NaN payloads are not -- canaries around every buffer.

A  edge values (tests/rot_edge_cases.py; tests/test_rot_edge_cases_cpu.py proves what they notice): zeros of both signs, denormal inputs and results,
   exact cancellation, overflow to inf and to NaN, an impulse at every position of every group size -- through the streaming kernels (aligned
   buffers) and the guarded ones (every buffer one element off a 16-byte boundary), out of place and in place; the same tensors through
   quantize_grouped_rotated, whose min / max then meet +-0, denormals, +-inf and NaN made by the rotation itself; dequantize_grouped_rotated on
   caller-given parameters (negative, +-0, +-inf, NaN, denormal scales; bytes equal to the zero point), SET and ADD onto NaN, +-inf, -0.0 and ties
B  the guarded kernels beyond one grid: 2 * 64 * CUs + 3 groups and a ragged tail, so that every block makes a second trip round its grid-stride
   loop and three make a third, with index 2^32 of the per-element mode inside the third; group size 32, every result against the model over the
   whole tensor
C  mixed alignment: exactly one buffer off a 16-byte boundary, and parameter arrays 4 bytes / 1 byte off under the streaming kernels
"""
import functools

import numpy as np
import pytest

import oracle as O
import rot_edge_cases as E
import rot_model as R
from grouped_model import dequantize_grouped, quantize_grouped
from test_gpu_grouped_rotated import (ELEM_SEED, FDT, GROUP_SIZES, PAIR_IDS, PAIRS, QDT, SEED, THRESHOLD, canaries_intact, carve, data, dev, host, packed_nbytes,
                                      quantize_rotated, same, triple_same)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
QUANT_PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
QUANT_PAIR_IDS = ["f32-u8", "f32-u4", "bf16-u4", "bf16-u2"]
MIXED_SIZES = ((128, 128 * 9 + 77), (4096, 4096 * 2 + 1), (32, 31))   # those of test_gpu_grouped_rotated.test_misaligned_buffers_give_the_same_bytes
OPS = {"set": O.SET, "add": O.ADD}


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


def placed(a, tdtype, off):
    """host array (float32, bfloat16 bits or bytes) -> (buffer, tensor, first byte): a copy `off` elements behind a 16-byte boundary, canaries around it"""
    buf, t, first = carve(a.size, tdtype, off)
    if a.size:
        t.copy_(torch.from_numpy(np.array(a)).cuda() if tdtype in (torch.uint8, torch.float32) else dev(a, O.BF16))
    assert a.size == 0 or (t.data_ptr() % 16 != 0) == (off != 0)
    return buf, t, first


def intact(b, what):
    buf, t, first = b
    canaries_intact(buf, first, t.numel() * t.element_size(), what)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check(t, want, want_dev, what):
    """the tensor against the model's array; with want_dev (the same on the device, no NaN in it) the host copy is made only to report a difference"""
    if want_dev is not None and torch.equal(bits(t), bits(want_dev)):
        return
    same(host(t), want, what)


def run_hadamard(x, dt, G, inverse, want, off_in, off_out, what, on_device=False):
    """out of place, then in place on the input's own buffer; canaries of both buffers"""
    import piquant.torch as pt

    wd = dev(want, dt) if on_device else None
    xb = placed(x, FDT[dt], off_in)
    ob = carve(x.size, FDT[dt], off_out)
    assert pt.hadamard_grouped(xb[1], group_size=G, seed=SEED, inverse=inverse, out=ob[1]) is ob[1]
    torch.cuda.synchronize()
    intact(ob, what + ": out")
    intact(xb, what + ": the input's buffer")
    check(ob[1], want, wd, what + ": out of place")
    check(xb[1], x, dev(x, dt) if on_device else None, what + ": the input")
    assert pt.hadamard_grouped(xb[1], group_size=G, seed=SEED, inverse=inverse, out=xb[1]) is xb[1]
    torch.cuda.synchronize()
    intact(xb, what + ": in place")
    check(xb[1], want, wd, what + ": in place")


@functools.lru_cache(maxsize=None)
def want_hadamard(name, G, dt, inverse):
    w = R.hadamard_grouped(E.case(name, G, SEED, dt), dt, G, SEED, inverse)
    w.setflags(write=False)
    return w


# ---- A. edge values

@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "inverse"))
@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_hadamard_edge_values(ctx, G, dt, inverse):
    for name in E.SMALL:
        x, want = E.case(name, G, SEED, dt), want_hadamard(name, G, dt, inverse)
        for off, path in ((0, "streaming"), (1, "guarded")):
            run_hadamard(x, dt, G, inverse, want, off, off, f"{name}, G={G}, {'inverse' if inverse else 'forward'}, {path}")


IMPULSE_BLOCKS = [(G, first, count) for G in GROUP_SIZES for first, count in E.impulse_blocks(G)]


@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "inverse"))
@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("G,first,count", IMPULSE_BLOCKS, ids=[f"{G}-{first}" for G, first, _ in IMPULSE_BLOCKS])
def test_hadamard_impulse_at_every_position(ctx, G, first, count, dt, inverse):
    """group p is an impulse at position p, for every p: every element of the signed matrix c H diag(d) is read off.  The G groups of the larger group
    sizes (67 MB of float32 at 4096) run in blocks of 2^19 elements, each a tensor of its own with the ragged tail behind it."""
    x = E.impulse_block(G, dt, first, count)
    want = R.hadamard_grouped(x, dt, G, SEED, inverse)
    for off, path in ((0, "streaming"), (1, "guarded")):
        run_hadamard(x, dt, G, inverse, want, off, off, f"impulses {first} .. {first + count - 1}, G={G}, {'inverse' if inverse else 'forward'}, {path}",
                     on_device=True)


@pytest.mark.parametrize("pair", QUANT_PAIRS, ids=QUANT_PAIR_IDS)
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_quantize_rotated_edge_values(ctx, G, pair):
    import piquant.torch as pt

    dt, qd = pair
    ctx.set_stochastic_per_element(False)
    for name in E.SMALL:
        x = E.case(name, G, SEED, dt)
        rotated = pt.hadamard_grouped(dev(x, dt).float(), group_size=G, seed=SEED)
        for mode, threshold in (("nearest", None), ("stochastic", THRESHOLD)):
            ctx.set_stochastic_threshold(threshold)
            q, s, z = pt.quantize_grouped(rotated, dtype=QDT[qd], group_size=G, round_mode=mode)
            composition = (pt.packed_bytes(q).cpu().numpy(), s.cpu().numpy(), z.cpu().numpy())
            model = R.quantize_grouped_rotated(x, dt, qd, G, SEED, O.STOCHASTIC if threshold else O.NEAREST, threshold or 0.0)
            for off, path in ((0, "streaming"), (1, "guarded")):
                xb = placed(x, FDT[dt], off)
                got = quantize_rotated(xb[1], qd, G, SEED, mode, off=off)
                what = f"{name}, G={G}, {mode}, {path}"
                intact(xb, what + ": the input's buffer")
                same(host(xb[1]), x, what + ": the input")
                triple_same(got, model, what + ": model")
                triple_same(got, composition, what + ": composition")
    ctx.set_stochastic_threshold(None)


def float_tile_elems(qd, G):
    """elements of one wave's chunk on the FLOAT32 tile (GroupedQuantTile<DT_F32, BITS, G>::CHUNK_ELEMS), which every rotated kernel sits on"""
    ob = 4 * BITS[qd] // 8
    v = G // 4
    rpg = 1 if v < 64 else v // 64
    return max(rpg, min(v, max(16 // ob, 4))) * 64 * 4


def edge_params(n, qd, G, seed):
    """packed bytes and caller-given parameters on the host: per-group scales from {negative, 0, -0, +-inf, NaN, denormal, 2^-8, ordinary}, arbitrary
    zero points, random bytes -- and in every third group every code EQUAL to the zero point, so that 0 * scale (-0.0, or NaN for an infinite scale)
    is what the group holds before it is rotated back"""
    rng = np.random.default_rng(seed)
    ng, b = -(-n // G), BITS[qd]
    qmax, pack = (1 << b) - 1, 8 // b
    pool = np.array([-0.75, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-41, 2.0 ** -8, 0.0123, 3.5], dtype=np.float32)
    s = pool[(np.arange(ng) + seed) % pool.size].copy()
    z = rng.integers(0, qmax + 1, ng).astype(np.uint8)
    raw = rng.integers(0, 256, (n * b + 7) // 8).astype(np.uint8)
    for g in range(0, ng, 3):
        rep = 0
        for j in range(pack):
            rep |= int(z[g]) << (j * b)
        raw[g * G // pack: min((g + 1) * G, n + pack - 1) // pack] = rep
    if n % pack:
        raw[-1] &= (1 << ((n % pack) * b)) - 1
    return raw, s, z


def edge_accumulator(n, dt, seed):
    """an out to ADD onto: NaN, +-inf, -0.0, and 1.0 / 1.0078125, on which a term of 2^-8 makes a bfloat16 tie (to even: down / up)"""
    a = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 1.0, 1.0078125)):
        a[k::7] = v
    return a if dt == O.F32 else O.f32_to_bf16(a)


def run_dequantize_rotated(raw, s, z, qd, dt, n, G, op, prev, offs, what):
    """dequantize_grouped_rotated with the packed input, the parameters and out at offs = (input, scales, zero points, out) -> out on the host"""
    import piquant.torch as pt

    qb, sb, zb = placed(raw, torch.uint8, offs[0]), placed(s, torch.float32, offs[1]), placed(z, torch.uint8, offs[2])
    ob = placed(prev, FDT[dt], offs[3]) if op == "add" else carve(n, FDT[dt], offs[3])
    got = pt.dequantize_grouped_rotated(qb[1], sb[1], zb[1], dtype=FDT[dt], group_size=G, seed=SEED, reduce_op=op, out=ob[1], quant_dtype=QDT[qd], shape=(n,))
    assert got is ob[1]
    torch.cuda.synchronize()
    for b, name in ((qb, "packed input"), (sb, "scales"), (zb, "zero points"), (ob, "out")):
        intact(b, f"{what}: {name}")
    assert np.array_equal(qb[1].cpu().numpy(), raw) and np.array_equal(zb[1].cpu().numpy(), z), f"{what}: an input was modified"
    return host(ob[1])


@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("G", (32, 256, 4096))
def test_dequantize_rotated_edge_parameters(ctx, G, pair, op):
    import piquant.torch as pt

    dt, qd = pair
    n = 3 * float_tile_elems(qd, G) + G + 5
    raw, s, z = edge_params(n, qd, G, 5 + G)
    prev = edge_accumulator(n, dt, 17) if op == "add" else None
    want = R.dequantize_grouped_rotated(raw, qd, dt, n, G, s, z, SEED, OPS[op], prev)
    wf = R.widen(want, dt)
    assert np.isnan(wf).any() and np.isfinite(wf).any()
    rd, sd, zd = (torch.from_numpy(a).cuda() for a in (raw, s, z))
    zf = pt.hadamard_grouped(pt.dequantize_grouped(rd, sd, zd, dtype=torch.float32, group_size=G, quant_dtype=QDT[qd], shape=(n,)), group_size=G, seed=SEED,
                             inverse=True)
    comp = host(zf.to(FDT[dt]) if op == "set" else (dev(prev, dt).float() + zf).to(FDT[dt]))
    for off, path in ((0, "streaming"), (1, "guarded")):
        got = run_dequantize_rotated(raw, s, z, qd, dt, n, G, op, prev, (off,) * 4, f"G={G}, {op}, {path}")
        same(got, want, f"G={G}, {op}, {path}: model")
        same(got, comp, f"G={G}, {op}, {path}: composition")


# ---- B. the guarded kernels beyond one grid: every buffer one element off

def beyond_one_grid(G):
    """-> (elements, groups, the grid's cap): 2 * 64 * CUs + 3 whole groups and a ragged one of G - 1 elements"""
    cap = 64 * torch.cuda.get_device_properties(0).multi_processor_count
    ngroups = 2 * cap + 3
    assert ngroups > cap and ngroups - 3 >= 2 * cap, "the grid-stride loop of the guarded kernels must make a second and a third trip"
    return ngroups * G + G - 1, ngroups, cap


# The group sizes run: 32 only.  The group count is fixed by the grid's cap, and the model goes over the whole tensor one oracle call a group; at
# G = 256 (8.4 M elements) every one of these tests took several times as long as the slowest test of tests/test_gpu_grouped_rotated.py.
GRID_G = (32,)
GRID_PAIR = {32: (O.BF16, O.UINT4)}


@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "inverse"))
@pytest.mark.parametrize("G", GRID_G)
def test_guarded_hadamard_beyond_one_grid(ctx, G, inverse):
    n, _, _ = beyond_one_grid(G)
    dt = GRID_PAIR[G][0]
    x = data(n, dt, G, seed=9)
    run_hadamard(x, dt, G, inverse, R.hadamard_grouped(x, dt, G, SEED, inverse), 1, 1, f"G={G}, guarded, {n} elements", on_device=True)


@pytest.mark.parametrize("G,mode", [(G, "nearest") for G in GRID_G] + [(32, "per-element")])
def test_guarded_quantize_rotated_beyond_one_grid(ctx, G, mode):
    n, ngroups, cap = beyond_one_grid(G)
    dt, qd = GRID_PAIR[G]
    x = data(n, dt, G, seed=9)
    xb = placed(x, FDT[dt], 1)
    ctx.set_stochastic_threshold(None)
    if mode == "nearest":
        ctx.set_stochastic_per_element(False)
        want = R.quantize_grouped_rotated(x, dt, qd, G, SEED)
    else:
        at = (2 * cap + 1) * G + 1                    # the element whose index is 2^32: element 1 of the second group of the third trip
        assert 2 * cap * G < at < ngroups * G
        ctx.set_stochastic_per_element(True, seed=ELEM_SEED, index_base=2 ** 32 - at)
        want = R.quantize_grouped_rotated_per_element(x, dt, qd, G, SEED, ELEM_SEED, 2 ** 32 - at)
    got = quantize_rotated(xb[1], qd, G, SEED, "nearest" if mode == "nearest" else "stochastic", off=1)
    ctx.set_stochastic_per_element(False)
    intact(xb, "the input's buffer")
    triple_same(got, want, f"G={G}, guarded, {mode}, {n} elements")


@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("G", GRID_G)
def test_guarded_dequantize_rotated_beyond_one_grid(ctx, G, op):
    n, ngroups, _ = beyond_one_grid(G)
    dt, qd = GRID_PAIR[G]
    rng = np.random.default_rng(G)
    raw = rng.integers(0, 256, packed_nbytes(n, qd)).astype(np.uint8)
    if n * BITS[qd] % 8:
        raw[-1] &= (1 << (n * BITS[qd] % 8)) - 1
    s = (rng.uniform(0.001, 0.5, ngroups + 1) * (1 + np.arange(ngroups + 1) % 251)).astype(np.float32)   # every group its own magnitude
    z = rng.integers(0, 1 << BITS[qd], ngroups + 1).astype(np.uint8)
    prev = data(n, dt, G, seed=10) if op == "add" else None
    want = R.dequantize_grouped_rotated(raw, qd, dt, n, G, s, z, SEED, OPS[op], prev)
    same(run_dequantize_rotated(raw, s, z, qd, dt, n, G, op, prev, (1, 1, 1, 1), f"G={G}, {op}"), want, f"G={G}, guarded, {op}, {n} elements")


# ---- C. mixed alignment

@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
def test_hadamard_one_buffer_misaligned(ctx, dt):
    for G, n in MIXED_SIZES:
        x = data(n, dt, G, seed=7)
        for inverse in (False, True):
            want = R.hadamard_grouped(x, dt, G, SEED, inverse)
            for off_in, off_out, which in ((0, 0, "all aligned"), (1, 0, "only in off"), (0, 1, "only out off")):
                run_hadamard(x, dt, G, inverse, want, off_in, off_out, f"G={G}, n={n}, inverse={inverse}, {which}")


def quantize_rotated_at(x, qd, G, mode, offs):
    """quantize_grouped_rotated with (packed out, scales, zero points) at offs elements behind a 16-byte boundary -> the three on the host"""
    import piquant.torch as pt

    n, ng = x.numel(), (x.numel() + G - 1) // G
    qb, sb, zb = carve(packed_nbytes(n, qd), torch.uint8, offs[0]), carve(ng, torch.float32, offs[1]), carve(ng, torch.uint8, offs[2])
    pt.quantize_grouped_rotated(x, dtype=QDT[qd], group_size=G, seed=SEED, round_mode=mode, out=qb[1], out_scales=sb[1], out_zero_points=zb[1])
    torch.cuda.synchronize()
    for b, name in ((qb, "packed bytes"), (sb, "scales"), (zb, "zero points")):
        intact(b, name)
    return qb[1].cpu().numpy(), sb[1].cpu().numpy(), zb[1].cpu().numpy()


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_quantize_rotated_one_buffer_misaligned(ctx, pair):
    dt, qd = pair
    ctx.set_stochastic_per_element(False)
    for G, n in MIXED_SIZES:
        x = data(n, dt, G, seed=7)
        for mode, threshold in (("nearest", None), ("stochastic", THRESHOLD)):
            ctx.set_stochastic_threshold(threshold)
            model = R.quantize_grouped_rotated(x, dt, qd, G, SEED, O.STOCHASTIC if threshold else O.NEAREST, threshold or 0.0)
            aligned = None
            for off_x, offs, which in ((0, (0, 0, 0), "all aligned"), (1, (0, 0, 0), "only x off"), (0, (1, 0, 0), "only the packed out off"),
                                       (0, (0, 1, 1), "only the parameters off")):
                xb = placed(x, FDT[dt], off_x)
                got = quantize_rotated_at(xb[1], qd, G, mode, offs)
                what = f"G={G}, n={n}, {mode}, {which}"
                intact(xb, what + ": the input's buffer")
                aligned = got if aligned is None else aligned
                triple_same(got, model, what + ": model")
                triple_same(got, aligned, what + ": the all-aligned call")
    ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_dequantize_rotated_one_buffer_misaligned(ctx, pair, op):
    dt, qd = pair
    for G, n in MIXED_SIZES:
        raw, s, z = R.quantize_grouped_rotated(data(n, O.F32, G, seed=7), O.F32, qd, G, SEED)
        prev = data(n, dt, G, seed=8) if op == "add" else None
        want = R.dequantize_grouped_rotated(raw, qd, dt, n, G, s, z, SEED, OPS[op], prev)
        aligned = None
        for offs, which in (((0, 0, 0, 0), "all aligned"), ((1, 0, 0, 0), "only the packed input off"), ((0, 0, 0, 1), "only out off"),
                            ((0, 1, 1, 0), "only the parameters off")):
            got = run_dequantize_rotated(raw, s, z, qd, dt, n, G, op, prev, offs, f"G={G}, n={n}, {op}, {which}")
            aligned = got if aligned is None else aligned
            same(got, want, f"G={G}, n={n}, {op}, {which}: model")
            same(got, aligned, f"G={G}, n={n}, {op}, {which}: the all-aligned call")


@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_dequantize_sum_parameters_misaligned(ctx, pair, op):
    """three terms whose scales lie 4 bytes and whose zero points lie 1 byte behind a 16-byte boundary, bytes and out aligned: the streaming kernel"""
    import piquant.torch as pt

    dt, qd = pair
    for G, n in MIXED_SIZES:
        terms = [quantize_grouped(data(n, O.F32, G, seed=30 + i), O.F32, qd, G) for i in range(3)]
        prev = data(n, dt, G, seed=8) if op == "add" else None
        want = prev
        for i, (raw, s, z) in enumerate(terms):
            want = dequantize_grouped(raw, qd, dt, n, G, s, z, O.SET if (op == "set" and i == 0) else O.ADD, prev=want)
        results = []
        for off in (0, 1):
            bufs = [(placed(raw, torch.uint8, 0), placed(s, torch.float32, off), placed(z, torch.uint8, off)) for raw, s, z in terms]
            ob = placed(prev, FDT[dt], 0) if op == "add" else carve(n, FDT[dt], 0)
            pt.dequantize_sum_grouped([b[0][1] for b in bufs], [b[1][1] for b in bufs], [b[2][1] for b in bufs], dtype=FDT[dt], group_size=G, reduce_op=op,
                                      out=ob[1], quant_dtype=QDT[qd], shape=(n,))
            torch.cuda.synchronize()
            for b in [x for t in bufs for x in t] + [ob]:
                intact(b, f"G={G}, n={n}, {op}, parameters {off} off")
            results.append(host(ob[1]))
            same(results[-1], want, f"G={G}, n={n}, {op}, parameters {off} off: model")
        same(results[1], results[0], f"G={G}, n={n}, {op}: the all-aligned call")
