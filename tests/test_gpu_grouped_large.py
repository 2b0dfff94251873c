"""The grouped kernels where 32 bits run out: tensors of 2^32 + 40 037 bfloat16 and 2^31 + 40 037 float32 elements (8.6 GB each), and one
float32 -> uint8 quantize and one uint8 -> float32 dequantize of 2^32 + 40 037 elements; the rotated calls (hadamard_grouped, quantize_grouped_rotated,
dequantize_grouped_rotated) and the grouped dequantize-sum of two terms at the same sizes.  One case is one test.  Element indices cross 2^31 and 2^32, input byte offsets 2^31, 2^32 and 2^33, output byte
offsets 2^31 (and 2^32 for the uint8 term of the reduce and for the float outputs).  Gradient buckets of a few GB are the ordinary use of the
grouped all-reduce; a truncated 64-bit product, chunk table entry, ctypes argument or allocation size would corrupt them silently.

Every case gets two checks:
  windows  four chunks either side of element 0, 2^31 and 2^32, of every element at which the byte offset into an input or an output is 2^31, 2^32
           or 2^33, and of the ragged end, copied to the host and compared bit for bit with the CPU model (tests/per_element_model.py with `start`,
           tests/grouped_model.py); NaNs and outliers are planted in them
  shards   the same call on consecutive slices of at most 2^28 elements, cut at multiples of 4096 elements, each with index_base = cut, into a
           second set of outputs: everything written must be equal as integers.  Slices of that size stay in the range that
           tests/test_gpu_grouped_per_element.py pins against the CPU model, which makes them a reference and not the code under test twice.
The rounding mode is per-element stochastic with index_base 0 and a seed whose upper half is not zero (so that index 2^32 is crossed by the tensor
itself), and nearest in addition for quantize_grouped.  Every group has its own magnitude, so a kernel that read a neighbour's parameters shows."""
import time

import numpy as np
import pytest

import oracle as O
import per_element_model as M
import rot_model as R
from grouped_model import PACK, dequantize_grouped, quantize_grouped
from per_element_cases import SEED_FULL as SEED
from test_gpu_grouped_per_element import same_bytes, same_floats, same_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_BF = 2 ** 32 + 40_037
N_F = 2 ** 31 + 40_037
N_GUARDED = N_BF          # the guarded (element-by-element) kernels run at full size as long as one call takes at most GUARDED_BUDGET seconds,
GUARDED_BUDGET = 10.0     # which test_guarded_kernels asserts; a kernel that needs longer runs at 2^31 + 40 037 elements instead
SHARD = 2 ** 28
FDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
QDT = {O.UINT8: torch.uint8, O.UINT4: torch.quint4x2, O.UINT2: torch.quint2x4}
BPE = {O.F32: 4, O.BF16: 2, O.UINT8: 1, O.UINT4: 0.5, O.UINT2: 0.25}   # bytes per element


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    if torch.cuda.get_device_properties(0).total_memory < 80 * 2**30:
        pytest.skip("needs ~60 GB of HBM")
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


@pytest.fixture(autouse=True)
def restore_and_free(ctx):
    yield
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def windows(n, chunk, types):
    """[(a, b)]: chunk-aligned, merged, inside [0, n)"""
    points = {0, 2 ** 31, 2 ** 32, n}
    for t in types:
        points |= {int(off / BPE[t]) for off in (2 ** 31, 2 ** 32, 2 ** 33)}
    spans = sorted((max(0, p // chunk * chunk - 4 * chunk), min(n, p // chunk * chunk + 4 * chunk)) for p in points if p <= n)
    out = []
    for a, b in spans:
        if a >= b:
            continue
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(b, out[-1][1]))
        else:
            out.append((a, b))
    assert all(a % chunk == 0 for a, _ in out) and out[0][0] == 0 and out[-1][1] == n
    return out


def shards(n):
    cuts = list(range(0, n, SHARD)) + [n]
    assert all(c % 4096 == 0 for c in cuts[:-1]) and max(b - a for a, b in zip(cuts[:-1], cuts[1:])) <= SHARD
    return list(zip(cuts[:-1], cuts[1:]))


def filled(n, dt, G, seed, wins, shift=0):
    """n elements uniform in (-1, 1), group g scaled by 0.5 + g mod 251, a NaN and two outliers planted in every window; shift: the tensor starts
    that many elements behind a 16-byte boundary"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.empty(n + shift, dtype=FDT[dt], device="cuda")[shift:]
    assert x.data_ptr() % 16 == shift * x.element_size()
    x.uniform_(-1, 1, generator=g)
    m = n // G * G
    factor = (0.5 + (torch.arange(m // G, device="cuda") % 251)).to(FDT[dt])
    x[:m].view(-1, G).mul_(factor[:, None])
    del factor
    for a, b in wins:
        x[a + 5] = float("nan")
        x[a + G + 3] = 3000.0
        x[b - 2] = -2500.0
    return x


def host(t, a, b):
    """elements [a, b) of a device tensor as numpy (bfloat16: bit patterns)"""
    s = t[a:b]
    return s.view(torch.int16).cpu().numpy().view(np.uint16) if s.dtype == torch.bfloat16 else s.cpu().numpy()


def packed_host(q, qd, a, b):
    return q[a // PACK[qd]: (b + PACK[qd] - 1) // PACK[qd]].cpu().numpy()


def params_host(s, z, G, a, b):
    return s[a // G: (b + G - 1) // G].cpu().numpy(), z[a // G: (b + G - 1) // G].cpu().numpy()


def addr(t, elems=0):
    return t.data_ptr() + elems * t.element_size()


def ready(ctx, base=None):
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.set_stochastic_threshold(None)
    if base is None:
        ctx.set_stochastic_per_element(False)
    else:
        ctx.set_stochastic_per_element(True, seed=SEED, index_base=base)


def whole_then_shards(ctx, n, call, stochastic=True, budget=None):
    """call(lo, hi, k): the entry on elements [lo, hi) into output set k.  budget: the whole call is timed, printed and must take no longer (seconds)"""
    ready(ctx, 0 if stochastic else None)
    if budget is None:
        call(0, n, 0)
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(0, n, 0)
        torch.cuda.synchronize()
        took = time.perf_counter() - t0
        print(f"the whole call: {n} elements in {took:.3f} s")
        assert took <= budget, f"the whole call took {took:.2f} s: run it at 2^31 + 40 037 elements"
    for lo, hi in shards(n):
        ready(ctx, lo if stochastic else None)
        call(lo, hi, 1)
    torch.cuda.synchronize()


def equal_ints(a, b, what):
    assert a.dtype == b.dtype and a.numel() == b.numel()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.view(view), b.view(view)), f"{what}: the whole call and its shards differ"


def outputs(n, qd, G, shift=0):
    """-> (packed bytes, scales, zero points), the packed bytes `shift` bytes off a 16-byte boundary"""
    ng = (n + G - 1) // G
    return (torch.empty(O.packed_numel(n, qd) + shift, dtype=torch.uint8, device="cuda")[shift:], torch.empty(ng, dtype=torch.float32, device="cuda"),
            torch.empty(ng, dtype=torch.uint8, device="cuda"))


def quantize_into(ctx, x, dt, qd, G, lo, hi, out, given, mode):
    import piquant

    q, s, z = out
    ctx.quantize_grouped_ptr(addr(x, lo), piquant.DataType(dt), q.data_ptr() + lo // PACK[qd], piquant.DataType(qd), hi - lo, G, addr(s, lo // G), addr(z, lo // G),
                             given, piquant.RoundMode(mode), _device_ptrs=True)


# ---- 1. quantize_grouped: one case a test

def given_params(n, qd, G):
    """parameters that are not the data's own, every group its own: a scale that follows the group's magnitude (the outliers saturate) and a zero
    point around the middle of the range"""
    g = torch.arange((n + G - 1) // G, device="cuda")
    qmax = (1 << M.BITS[qd]) - 1
    return ((0.5 + g % 251) * (2.5 / qmax)).to(torch.float32), (qmax // 2 - 1 + g % 3).to(torch.uint8)


QUANTIZE_CASES = [(dt, qd, n, G, case) for dt, qd, n in ((O.BF16, O.UINT4, N_BF), (O.F32, O.UINT8, N_F)) for G in (128, 32, 4096)
                  for case in ("per-element", "given", "nearest") if G == 128 or case != "given"]
QUANTIZE_CASES.append((O.F32, O.UINT8, N_BF, 128, "per-element"))   # the float32 templates past element 2^32 (17 GB of input)


@pytest.mark.parametrize("dt,qd,n,G,case", QUANTIZE_CASES)
def test_quantize_grouped(ctx, dt, qd, n, G, case):
    """per-element: computed parameters, the whole call through piquant.torch, whose allocations are sized from numel; given: per-element with
    given parameters; nearest: computed parameters, no thresholds"""
    import piquant.torch as pt

    wins = windows(n, M.tile(dt, qd, G).chunk, [dt, qd])
    stochastic = case != "nearest"
    mode = O.STOCHASTIC if stochastic else O.NEAREST
    x = a = b = given = None
    try:
        x = filled(n, dt, G, 1, wins)
        b = outputs(n, qd, G)
        if case == "per-element":
            ready(ctx, 0)
            q, s, z = pt.quantize_grouped(x, dtype=QDT[qd], group_size=G, round_mode="stochastic")
            a = (pt.packed_bytes(q), s, z)
            del q, s, z
            assert a[0].numel() == O.packed_numel(n, qd) and a[1].numel() == a[2].numel() == (n + G - 1) // G
            for lo, hi in shards(n):
                ready(ctx, lo)
                quantize_into(ctx, x, dt, qd, G, lo, hi, b, False, mode)
            torch.cuda.synchronize()
        elif case == "given":
            given = given_params(n, qd, G)
            a, b = (outputs(n, qd, G)[0],) + given, (b[0],) + given
            whole_then_shards(ctx, n, lambda lo, hi, k: quantize_into(ctx, x, dt, qd, G, lo, hi, (a, b)[k], True, mode))
        else:
            a = outputs(n, qd, G)
            whole_then_shards(ctx, n, lambda lo, hi, k: quantize_into(ctx, x, dt, qd, G, lo, hi, (a, b)[k], False, mode), stochastic=False)
        for k, name in enumerate(("bytes", "scales", "zero points")):
            equal_ints(a[k], b[k], name)
        for lo, hi in wins:
            xw, what = host(x, lo, hi), f"window [{lo}, {hi})"
            if stochastic:
                want = M.quantize(xw, dt, qd, G, SEED, 0, params=params_host(given[0], given[1], G, lo, hi) if given else None, start=lo)
            else:
                want = quantize_grouped(xw, dt, qd, G)
            same_params(*params_host(a[1], a[2], G, lo, hi), want[1], want[2], what)
            same_bytes(packed_host(a[0], qd, lo, hi), want[0], qd, what)
    finally:
        del x, a, b, given
        torch.cuda.empty_cache()


# ---- 2. dequantize_grouped

def random_packed(n, qd, G, seed, shift=0):
    """random packed bytes (the bits behind the tensor's end zero; `shift` bytes off a 16-byte boundary) with a scale and a zero point of its own per group"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    nb, ng = O.packed_numel(n, qd), (n + G - 1) // G
    q = torch.empty(nb + shift, dtype=torch.uint8, device="cuda")[shift:].random_(0, 256, generator=g)
    if n % PACK[qd]:
        q[-1] &= (1 << ((n % PACK[qd]) * M.BITS[qd])) - 1
    s = torch.empty(ng, dtype=torch.float32, device="cuda").uniform_(0.001, 0.5, generator=g) * (1 + torch.arange(ng, device="cuda") % 251)
    z = torch.empty(ng, dtype=torch.uint8, device="cuda").random_(0, (1 << M.BITS[qd]), generator=g)
    return q, s, z


DEQUANTIZE_CASES = [(qd, dt, n, op) for qd, dt, n in ((O.UINT4, O.BF16, N_BF), (O.UINT8, O.F32, N_F)) for op in (O.SET, O.ADD)]
DEQUANTIZE_CASES.append((O.UINT8, O.F32, N_BF, O.SET))   # the float32 templates past element 2^32 (17 GB of output)


@pytest.mark.parametrize("qd,dt,n,op", DEQUANTIZE_CASES)
def test_dequantize_grouped(ctx, qd, dt, n, op):
    import piquant

    G = 128
    wins = windows(n, 2048 * PACK[qd], [dt, qd])
    t = prev = ya = yb = None
    try:
        t = random_packed(n, qd, G, 3)
        if op == O.ADD:
            prev = filled(n, dt, G, 4, wins)
            ya, yb = prev.clone(), prev.clone()
        else:
            ya, yb = (torch.empty(n, dtype=FDT[dt], device="cuda") for _ in range(2))

        def call(lo, hi, k):
            ctx.dequantize_grouped_ptr(t[0].data_ptr() + lo // PACK[qd], piquant.DataType(qd), addr((ya, yb)[k], lo), piquant.DataType(dt), hi - lo, G,
                                       addr(t[1], lo // G), addr(t[2], lo // G), piquant.ReduceOp(op), _device_ptrs=True)

        whole_then_shards(ctx, n, call, stochastic=False)
        equal_ints(ya, yb, f"op={op}")
        for lo, hi in wins:
            s, z = params_host(t[1], t[2], G, lo, hi)
            want = dequantize_grouped(packed_host(t[0], qd, lo, hi), qd, dt, hi - lo, G, s, z, op, host(prev, lo, hi) if op == O.ADD else None)
            same_floats(host(ya, lo, hi), want, dt, f"op={op}, window [{lo}, {hi})")
    finally:
        del t, prev, ya, yb
        torch.cuda.empty_cache()


# ---- 3. the fused reduce: a bfloat16 accumulator and one uint8 term, whose byte offsets cross 2^32

def made_term(ctx, n, dt, qd, G, seed, wins):
    """a packed term made by quantize_grouped (nearest) from a second tensor, which is freed"""
    import piquant.torch as pt

    y = filled(n, dt, G, seed, wins)
    ready(ctx)
    q, s, z = pt.quantize_grouped(y, dtype=QDT[qd], group_size=G)
    torch.cuda.synchronize()
    del y
    torch.cuda.empty_cache()
    return pt.packed_bytes(q), s, z


def test_reduce_quantize_grouped(ctx):
    import piquant

    dt, qd, G, n = O.BF16, O.UINT8, 128, N_BF
    DT = piquant.DataType
    wins = windows(n, M.tile(dt, qd, G).chunk, [dt, qd])
    term = acc = a = b = None
    try:
        term = made_term(ctx, n, dt, qd, G, 5, wins)
        acc = [filled(n, dt, G, 6, wins)]
        before = [host(acc[0], lo, hi) for lo, hi in wins]
        acc.append(acc[0].clone())   # acc is unspecified after a call: the shards get their own
        a, b = outputs(n, qd, G), outputs(n, qd, G)

        def call(lo, hi, k):
            q, s, z = (a, b)[k]
            ctx.reduce_quantize_grouped_ptr(addr(acc[k], lo), DT(dt), [term[0].data_ptr() + lo // PACK[qd]], [addr(term[1], lo // G)], [addr(term[2], lo // G)],
                                            q.data_ptr() + lo // PACK[qd], DT(qd), hi - lo, G, addr(s, lo // G), addr(z, lo // G), piquant.RoundMode.STOCHASTIC,
                                            _device_ptrs=True)

        whole_then_shards(ctx, n, call)
        for k, name in enumerate(("bytes", "scales", "zero points")):
            equal_ints(a[k], b[k], name)
        for (lo, hi), xw in zip(wins, before):
            tw = (packed_host(term[0], qd, lo, hi),) + params_host(term[1], term[2], G, lo, hi)
            want = M.reduce(xw, [tw], dt, qd, G, SEED, 0, start=lo)
            same_params(*params_host(a[1], a[2], G, lo, hi), want[1], want[2], f"window [{lo}, {hi})")
            same_bytes(packed_host(a[0], qd, lo, hi), want[0], qd, f"window [{lo}, {hi})")
    finally:
        del term, acc, a, b
        torch.cuda.empty_cache()


# ---- 4. error feedback

def ef_into(ctx, x, r, dt, dt_r, qd, G, lo, hi, out):
    import piquant

    q, s, z = out
    ctx.quantize_grouped_ef_ptr(addr(x, lo), piquant.DataType(dt), addr(r, lo), q.data_ptr() + lo // PACK[qd], piquant.DataType(qd), hi - lo, G, addr(s, lo // G),
                                addr(z, lo // G), piquant.RoundMode.STOCHASTIC, _device_ptrs=True, residual_dtype=None if dt_r == dt else piquant.DataType(dt_r))


@pytest.mark.parametrize("dt_r", [O.BF16, O.F32])
def test_quantize_grouped_ef(ctx, dt_r):
    dt, qd, G, n = O.BF16, O.UINT4, 128, N_BF
    wins = windows(n, M.tile(dt_r, qd, G).chunk, [dt, dt_r, qd])
    x = r = a = b = None
    try:
        x = filled(n, dt, G, 7, wins)
        r = [filled(n, dt_r, G, 8, wins).mul_(0.01)]
        before = [(host(x, lo, hi), host(r[0], lo, hi)) for lo, hi in wins]
        r.append(r[0].clone())
        a, b = outputs(n, qd, G), outputs(n, qd, G)
        whole_then_shards(ctx, n, lambda lo, hi, k: ef_into(ctx, x, r[k], dt, dt_r, qd, G, lo, hi, (a, b)[k]))
        for k, name in enumerate(("bytes", "scales", "zero points")):
            equal_ints(a[k], b[k], name)
        equal_ints(r[0], r[1], "residual")
        for (lo, hi), (xw, rw) in zip(wins, before):
            want = M.ef_step(xw, rw, dt, qd, G, SEED, 0, start=lo) if dt_r == dt else M.ef_f32r_step(xw, rw, qd, G, SEED, 0, start=lo)
            same_params(*params_host(a[1], a[2], G, lo, hi), want[1], want[2], f"window [{lo}, {hi})")
            same_bytes(packed_host(a[0], qd, lo, hi), want[0], qd, f"window [{lo}, {hi})")
            same_floats(host(r[0], lo, hi), want[3], dt_r, f"residual, window [{lo}, {hi})")
    finally:
        del x, r, a, b
        torch.cuda.empty_cache()


def test_reduce_quantize_grouped_ef_float32_residual(ctx):
    """a bfloat16 accumulator, a float32 residual and one uint4 term"""
    import piquant

    dt, dt_r, qd, G, n = O.BF16, O.F32, O.UINT4, 128, N_BF
    DT = piquant.DataType
    wins = windows(n, M.tile(dt_r, qd, G).chunk, [dt, dt_r, qd])
    term = acc = r = a = b = None
    try:
        term = made_term(ctx, n, dt, qd, G, 9, wins)
        acc = [filled(n, dt, G, 10, wins)]
        r = [filled(n, dt_r, G, 11, wins).mul_(0.01)]
        before = [(host(acc[0], lo, hi), host(r[0], lo, hi)) for lo, hi in wins]
        acc.append(acc[0].clone())
        r.append(r[0].clone())
        a, b = outputs(n, qd, G), outputs(n, qd, G)

        def call(lo, hi, k):
            q, s, z = (a, b)[k]
            ctx.reduce_quantize_grouped_ef_ptr(addr(acc[k], lo), DT(dt), addr(r[k], lo), [term[0].data_ptr() + lo // PACK[qd]], [addr(term[1], lo // G)],
                                               [addr(term[2], lo // G)], q.data_ptr() + lo // PACK[qd], DT(qd), hi - lo, G, addr(s, lo // G), addr(z, lo // G),
                                               piquant.RoundMode.STOCHASTIC, _device_ptrs=True, residual_dtype=DT(dt_r))

        whole_then_shards(ctx, n, call)
        for k, name in enumerate(("bytes", "scales", "zero points")):
            equal_ints(a[k], b[k], name)
        equal_ints(r[0], r[1], "residual")
        for (lo, hi), (xw, rw) in zip(wins, before):
            tw = (packed_host(term[0], qd, lo, hi),) + params_host(term[1], term[2], G, lo, hi)
            want = M.reduce_ef_f32r_per_element_model(xw, rw, [tw], qd, G, SEED, 0, start=lo)
            same_params(*params_host(a[1], a[2], G, lo, hi), want[1], want[2], f"window [{lo}, {hi})")
            same_bytes(packed_host(a[0], qd, lo, hi), want[0], qd, f"window [{lo}, {hi})")
            same_floats(host(r[0], lo, hi), want[3], dt_r, f"residual, window [{lo}, {hi})")
    finally:
        del term, acc, r, a, b
        torch.cuda.empty_cache()


# ---- 5. quantize-dequantize

def requant_into(ctx, x, out, dt, qd, G, lo, hi, add, s=None, z=None):
    import piquant

    ctx.quantize_dequantize_grouped_ptr(addr(x, lo), piquant.DataType(dt), addr(out, lo), piquant.DataType(qd), hi - lo, G, 0 if s is None else addr(s, lo // G),
                                        0 if z is None else addr(z, lo // G), False, piquant.RoundMode.STOCHASTIC,
                                        piquant.ReduceOp.ADD if add else piquant.ReduceOp.SET, _device_ptrs=True)


@pytest.mark.parametrize("dt,qd,n,add", [(O.BF16, O.UINT2, N_BF, False), (O.F32, O.UINT8, N_F, True)])
def test_quantize_dequantize_grouped(ctx, dt, qd, n, add):
    """bfloat16 through uint2 in place (SET, no parameter arrays); float32 through uint8, ADD onto an accumulator, the parameters written"""
    G = 128
    wins = windows(n, M.tile(dt, qd, G).chunk, [dt, qd])
    x = y = p = None
    try:
        x = [filled(n, dt, G, 12, wins)]
        before = [host(x[0], lo, hi) for lo, hi in wins]
        if add:
            prev = filled(n, dt, G, 13, wins)
            prev_before = [host(prev, lo, hi) for lo, hi in wins]
            y = [prev, prev.clone()]
            del prev
            ng = (n + G - 1) // G
            p = [(torch.empty(ng, dtype=torch.float32, device="cuda"), torch.empty(ng, dtype=torch.uint8, device="cuda")) for _ in range(2)]
            whole_then_shards(ctx, n, lambda lo, hi, k: requant_into(ctx, x[0], y[k], dt, qd, G, lo, hi, True, *p[k]))
            equal_ints(p[0][0], p[1][0], "scales")
            equal_ints(p[0][1], p[1][1], "zero points")
        else:
            x.append(x[0].clone())
            y = x
            whole_then_shards(ctx, n, lambda lo, hi, k: requant_into(ctx, x[k], x[k], dt, qd, G, lo, hi, False))
        equal_ints(y[0], y[1], "out")
        for i, (lo, hi) in enumerate(wins):
            want = M.quantize_dequantize(before[i], dt, qd, G, SEED, 0, prev=prev_before[i] if add else None, start=lo)
            if add:
                same_params(*params_host(p[0][0], p[0][1], G, lo, hi), want[1], want[2], f"window [{lo}, {hi})")
            same_floats(host(y[0], lo, hi), want[0], dt, f"window [{lo}, {hi})")
    finally:
        del x, y, p
        torch.cuda.empty_cache()


# ---- 6. a batch whose second member's chunks start behind 2^32 elements of chunks

def test_quantize_grouped_batch(ctx):
    import piquant

    dt, qd, G = O.BF16, O.UINT4, 128
    numels = [N_BF, 70_003]
    chunk = M.tile(dt, qd, G).chunk
    xs = a = b = None
    try:
        wins = [windows(n, chunk, [dt, qd]) for n in numels]
        xs = [filled(n, dt, G, 14 + i, w) for i, (n, w) in enumerate(zip(numels, wins))]
        a, b = [outputs(n, qd, G) for n in numels], [outputs(n, qd, G) for n in numels]
        ready(ctx, 0)
        ctx.quantize_grouped_batch_ptr([x.data_ptr() for x in xs], piquant.DataType(dt), [o[0].data_ptr() for o in a], piquant.DataType(qd), numels, G,
                                       [o[1].data_ptr() for o in a], [o[2].data_ptr() for o in a], False, piquant.RoundMode.STOCHASTIC, _device_ptrs=True)
        for i, n in enumerate(numels):   # every member indexes its own elements from index_base + 0
            for lo, hi in shards(n):
                ready(ctx, lo)
                quantize_into(ctx, xs[i], dt, qd, G, lo, hi, b[i], False, O.STOCHASTIC)
        torch.cuda.synchronize()
        for i, n in enumerate(numels):
            for k, name in enumerate(("bytes", "scales", "zero points")):
                equal_ints(a[i][k], b[i][k], f"member {i}, {name}")
            for lo, hi in wins[i]:
                want = M.quantize(host(xs[i], lo, hi), dt, qd, G, SEED, 0, start=lo)
                same_params(*params_host(a[i][1], a[i][2], G, lo, hi), want[1], want[2], f"member {i}, window [{lo}, {hi})")
                same_bytes(packed_host(a[i][0], qd, lo, hi), want[0], qd, f"member {i}, window [{lo}, {hi})")
    finally:
        del xs, a, b
        torch.cuda.empty_cache()


# ---- 7. the guarded (element-by-element) kernels: every buffer one element off a 16-byte boundary

@pytest.mark.parametrize("entry", ["quantize", "dequantize", "ef", "quantize_dequantize"])
def test_guarded_kernels(ctx, entry):
    import piquant

    dt, qd, G, n = O.BF16, O.UINT4, 128, N_GUARDED
    wins = windows(n, 4096, [dt, qd])
    x = r = a = b = t = y = None
    try:
        if entry == "dequantize":
            t = random_packed(n, qd, G, 20, shift=1)
            y = [torch.empty(n + 1, dtype=FDT[dt], device="cuda")[1:] for _ in range(2)]
            assert t[0].data_ptr() % 16 == 1 and y[0].data_ptr() % 16 == 2

            def call(lo, hi, k):
                ctx.dequantize_grouped_ptr(t[0].data_ptr() + lo // PACK[qd], piquant.DataType(qd), addr(y[k], lo), piquant.DataType(dt), hi - lo, G,
                                           addr(t[1], lo // G), addr(t[2], lo // G), piquant.ReduceOp.SET, _device_ptrs=True)

            whole_then_shards(ctx, n, call, stochastic=False, budget=GUARDED_BUDGET)
            equal_ints(y[0], y[1], "out")
            for lo, hi in wins:
                want = dequantize_grouped(packed_host(t[0], qd, lo, hi), qd, dt, hi - lo, G, *params_host(t[1], t[2], G, lo, hi))
                same_floats(host(y[0], lo, hi), want, dt, f"window [{lo}, {hi})")
            return
        x = [filled(n, dt, G, 21, wins, shift=1)]
        before = [host(x[0], lo, hi) for lo, hi in wins]
        if entry == "quantize_dequantize":
            x.append(torch.empty(n + 1, dtype=FDT[dt], device="cuda")[1:].copy_(x[0]))
            assert x[1].data_ptr() % 16 == 2
            whole_then_shards(ctx, n, lambda lo, hi, k: requant_into(ctx, x[k], x[k], dt, qd, G, lo, hi, False), budget=GUARDED_BUDGET)
            equal_ints(x[0], x[1], "out")
            for i, (lo, hi) in enumerate(wins):
                same_floats(host(x[0], lo, hi), M.quantize_dequantize(before[i], dt, qd, G, SEED, 0, start=lo)[0], dt, f"window [{lo}, {hi})")
            return
        a, b = outputs(n, qd, G, shift=1), outputs(n, qd, G, shift=1)
        assert a[0].data_ptr() % 16 == 1 and x[0].data_ptr() % 16 == 2
        if entry == "quantize":
            whole_then_shards(ctx, n, lambda lo, hi, k: quantize_into(ctx, x[0], dt, qd, G, lo, hi, (a, b)[k], False, O.STOCHASTIC), budget=GUARDED_BUDGET)
            model = lambda i, lo: M.quantize(before[i], dt, qd, G, SEED, 0, start=lo)
        else:
            r = [filled(n, dt, G, 22, wins, shift=1).mul_(0.01)]
            r_before = [host(r[0], lo, hi) for lo, hi in wins]
            r.append(torch.empty(n + 1, dtype=FDT[dt], device="cuda")[1:].copy_(r[0]))
            whole_then_shards(ctx, n, lambda lo, hi, k: ef_into(ctx, x[0], r[k], dt, dt, qd, G, lo, hi, (a, b)[k]), budget=GUARDED_BUDGET)
            equal_ints(r[0], r[1], "residual")
            model = lambda i, lo: M.ef_step(before[i], r_before[i], dt, qd, G, SEED, 0, start=lo)
        for k, name in enumerate(("bytes", "scales", "zero points")):
            equal_ints(a[k], b[k], name)
        for i, (lo, hi) in enumerate(wins):
            want = model(i, lo)
            same_params(*params_host(a[1], a[2], G, lo, hi), want[1], want[2], f"window [{lo}, {hi})")
            same_bytes(packed_host(a[0], qd, lo, hi), want[0], qd, f"window [{lo}, {hi})")
            if entry == "ef":
                same_floats(host(r[0], lo, hi), want[3], dt, f"residual, window [{lo}, {hi})")
    finally:
        del x, r, a, b, t, y
        torch.cuda.empty_cache()


# ---- 8. the randomized Hadamard rotation and the calls built on it: the streaming kernels (tests/test_gpu_grouped_rotated_edges.py takes the guarded
# ones round their grid-stride loop).  A multiple of 4096 is a group boundary for every group size, so a shard rotates as the whole tensor does
# ("every group, shard and chunk that starts on a group boundary uses the same d"): the shards pin that sentence of the contract too.  The windows are
# chunks of the FLOAT32 tile, which every rotated kernel sits on.

ROT_SEED = 0x9E37_79B9_7F4A_7C15   # 64 bits next to a size_t numel in the ctypes entries


@pytest.mark.parametrize("dt,n,G,inverse,in_place", [(O.BF16, N_BF, 128, False, True), (O.BF16, N_BF, 4096, True, True), (O.F32, N_F, 32, False, False)])
def test_hadamard_grouped(ctx, dt, n, G, inverse, in_place):
    """G = 4096 takes the stages between the rows one lane holds"""
    import piquant

    wins = windows(n, M.tile(O.F32, O.UINT8, G).chunk, [dt])
    x = y = None
    try:
        x = [filled(n, dt, G, 30, wins)]
        before = [host(x[0], lo, hi) for lo, hi in wins]
        if in_place:
            x.append(x[0].clone())
            y = x
        else:
            x.append(x[0])
            y = [torch.empty(n, dtype=FDT[dt], device="cuda") for _ in range(2)]

        def call(lo, hi, k):
            ctx.hadamard_grouped_ptr(addr(x[k], lo), piquant.DataType(dt), addr(y[k], lo), hi - lo, G, ROT_SEED, inverse, _device_ptrs=True)

        whole_then_shards(ctx, n, call, stochastic=False)
        equal_ints(y[0], y[1], "out")
        for (lo, hi), xw in zip(wins, before):
            same_floats(host(y[0], lo, hi), R.hadamard_grouped(xw, dt, G, ROT_SEED, inverse), dt, f"window [{lo}, {hi})")
    finally:
        del x, y
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dt,qd,n,G,case", [(O.BF16, O.UINT4, N_BF, 128, "per-element"), (O.F32, O.UINT8, N_F, 4096, "nearest")])
def test_quantize_grouped_rotated(ctx, dt, qd, n, G, case):
    import piquant

    wins = windows(n, M.tile(O.F32, qd, G).chunk, [dt, qd])
    stochastic = case == "per-element"
    x = a = b = None
    try:
        x = filled(n, dt, G, 31, wins)
        a, b = outputs(n, qd, G), outputs(n, qd, G)

        def call(lo, hi, k):
            q, s, z = (a, b)[k]
            ctx.quantize_grouped_rotated_ptr(addr(x, lo), piquant.DataType(dt), q.data_ptr() + lo // PACK[qd], piquant.DataType(qd), hi - lo, G, addr(s, lo // G),
                                             addr(z, lo // G), ROT_SEED, piquant.RoundMode(O.STOCHASTIC if stochastic else O.NEAREST), _device_ptrs=True)

        whole_then_shards(ctx, n, call, stochastic=stochastic)
        for k, name in enumerate(("bytes", "scales", "zero points")):
            equal_ints(a[k], b[k], name)
        for lo, hi in wins:
            xw, what = host(x, lo, hi), f"window [{lo}, {hi})"
            if stochastic:
                want = R.quantize_grouped_rotated_per_element(xw, dt, qd, G, ROT_SEED, SEED, 0, start=lo)
            else:
                want = R.quantize_grouped_rotated(xw, dt, qd, G, ROT_SEED)
            same_params(*params_host(a[1], a[2], G, lo, hi), want[1], want[2], what)
            same_bytes(packed_host(a[0], qd, lo, hi), want[0], qd, what)
    finally:
        del x, a, b
        torch.cuda.empty_cache()


def test_dequantize_grouped_rotated(ctx):
    """uint4 -> bfloat16, ADD"""
    import piquant

    qd, dt, n, G = O.UINT4, O.BF16, N_BF, 128
    wins = windows(n, M.tile(O.F32, qd, G).chunk, [dt, qd])
    t = prev = ya = yb = None
    try:
        t = random_packed(n, qd, G, 32)
        prev = filled(n, dt, G, 33, wins)
        ya, yb = prev.clone(), prev.clone()

        def call(lo, hi, k):
            ctx.dequantize_grouped_rotated_ptr(t[0].data_ptr() + lo // PACK[qd], piquant.DataType(qd), addr((ya, yb)[k], lo), piquant.DataType(dt), hi - lo, G,
                                               addr(t[1], lo // G), addr(t[2], lo // G), ROT_SEED, piquant.ReduceOp.ADD, _device_ptrs=True)

        whole_then_shards(ctx, n, call, stochastic=False)
        equal_ints(ya, yb, "out")
        for lo, hi in wins:
            s, z = params_host(t[1], t[2], G, lo, hi)
            want = R.dequantize_grouped_rotated(packed_host(t[0], qd, lo, hi), qd, dt, hi - lo, G, s, z, ROT_SEED, O.ADD, host(prev, lo, hi))
            same_floats(host(ya, lo, hi), want, dt, f"window [{lo}, {hi})")
    finally:
        del t, prev, ya, yb
        torch.cuda.empty_cache()


# ---- 9. the grouped dequantize-sum, two terms: the windows are chunks of the tile of the OUTPUT type

@pytest.mark.parametrize("qd,dt,n,op", [(O.UINT4, O.BF16, N_BF, O.ADD), (O.UINT8, O.F32, N_F, O.SET)])
def test_dequantize_sum_grouped(ctx, qd, dt, n, op):
    import piquant

    G = 128
    wins = windows(n, M.tile(dt, qd, G).chunk, [dt, qd])
    terms = prev = ya = yb = None
    try:
        terms = [random_packed(n, qd, G, 34 + i) for i in range(2)]
        if op == O.ADD:
            prev = filled(n, dt, G, 36, wins)
            ya, yb = prev.clone(), prev.clone()
        else:
            ya, yb = (torch.empty(n, dtype=FDT[dt], device="cuda") for _ in range(2))

        def call(lo, hi, k):
            ctx.dequantize_sum_grouped_ptr([t[0].data_ptr() + lo // PACK[qd] for t in terms], piquant.DataType(qd), [addr(t[1], lo // G) for t in terms],
                                           [addr(t[2], lo // G) for t in terms], addr((ya, yb)[k], lo), piquant.DataType(dt), hi - lo, G, piquant.ReduceOp(op),
                                           _device_ptrs=True)

        whole_then_shards(ctx, n, call, stochastic=False)
        equal_ints(ya, yb, f"op={op}")
        for lo, hi in wins:
            want = host(prev, lo, hi) if op == O.ADD else None
            for i, t in enumerate(terms):
                s, z = params_host(t[1], t[2], G, lo, hi)
                want = dequantize_grouped(packed_host(t[0], qd, lo, hi), qd, dt, hi - lo, G, s, z, op if i == 0 else O.ADD, want)
            same_floats(host(ya, lo, hi), want, dt, f"op={op}, window [{lo}, {hi})")
    finally:
        del terms, prev, ya, yb
        torch.cuda.empty_cache()
