"""The per-group clip search on the MI355X (piquant_hip_quantize_grouped_clipped, its batch and the piquant.torch wrappers): bytes, scales, zero
points and choices bit for bit against the CPU model (tests/clip_model.py), which tests/test_grouped_clip_cpu.py shows to notice a wrong sum
order, a wrong comparison and eight other faults on the committed cases (tests/clip_cases.py) -- all of which run here.

The spread of the choices.  The bit-for-bit comparison proves little where every group chooses k = 0, so every (pair, group size) also runs
tests/clip_cases.py's constructed grid groups, on which the model's choices are asserted to take at least three values on every wire -- uint8
from G = 2048 on, two values from G = 512, and none below: clip_cases.grid_min_choices has the arithmetic (clipping the extremes costs a uint8
candidate qmax^2 / 2 steps^2, a bulk element gains at most a quarter).  The Gaussian tensors spread on uint2 and, from G = 128, on uint4.
"""
import numpy as np
import pytest

import clip_cases as CC
import clip_model as M
import oracle as O
import per_element_model as PE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
ESIZE = CC.ESIZE


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context.get(0)
    yield c
    c.set_stochastic_threshold(None)
    c.set_stochastic_per_element(False)


class Buf:
    """`nbytes` device bytes at a 16-byte boundary plus `shift`, GUARD bytes of 0xAA on both sides."""

    def __init__(self, nbytes, shift=0, data=None):
        self.whole = torch.full((GUARD + shift + nbytes + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.n = GUARD + shift, nbytes
        self.view = self.whole[self.lo: self.lo + nbytes]
        if data is not None and nbytes:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()))

    @property
    def ptr(self):
        return self.view.data_ptr() if self.n else self.whole.data_ptr() + self.lo

    def guards_ok(self):
        return bool((self.whole[: self.lo] == 0xAA).all()) and bool((self.whole[self.lo + self.n:] == 0xAA).all())

    def get(self, dtype=np.uint8):
        return self.view.cpu().numpy().view(dtype)


def device_buffers(x, dt_in, qd, G, shifts=(0, 0, 0, 0, 0), choices=True):
    n = x.size
    ng = (n + G - 1) // G
    return (Buf(x.nbytes, shifts[0], x), Buf(O.packed_numel(n, qd), shifts[1]), Buf(4 * ng, shifts[2]), Buf(ng, shifts[3]),
            Buf(ng, shifts[4]) if choices else None)


def clipped(ctx, x, dt_in, qd, G, steps, mode=O.NEAREST, shifts=(0, 0, 0, 0, 0), choices=True):
    """-> (packed bytes, scales, zero points, choices or None) from the device, guard bytes around every buffer checked."""
    import piquant

    xb, ob, sb, zb, cb = device_buffers(x, dt_in, qd, G, shifts, choices)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_clipped_ptr(xb.ptr, piquant.DataType(dt_in), ob.ptr, piquant.DataType(qd), x.size, G, sb.ptr, zb.ptr, cb.ptr if cb else 0, steps,
                                     piquant.RoundMode(mode), _device_ptrs=True)
    torch.cuda.synchronize()
    for b, what in ((xb, "in"), (ob, "out"), (sb, "scales"), (zb, "zero_points"), (cb, "choices")):
        assert b is None or b.guards_ok(), f"wrote outside {what}"
    return ob.get(), sb.get(np.float32), zb.get(), cb.get() if cb else None


def plain(ctx, x, dt_in, qd, G, mode=O.NEAREST, given=None):
    """quantize_grouped on the device, parameters computed or given"""
    import piquant

    xb, ob, sb, zb, _ = device_buffers(x, dt_in, qd, G, choices=False)
    if given is not None:
        sb, zb = Buf(given[0].nbytes, 0, given[0]), Buf(given[1].nbytes, 0, given[1])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_ptr(xb.ptr, piquant.DataType(dt_in), ob.ptr, piquant.DataType(qd), x.size, G, sb.ptr, zb.ptr, given is not None,
                             piquant.RoundMode(mode), _device_ptrs=True)
    torch.cuda.synchronize()
    return ob.get(), sb.get(np.float32), zb.get()


def assert_same(got, want, what=""):
    q, s, z, c = got
    wq, ws, wz, wc = want
    if c is not None:
        assert np.array_equal(c, wc), f"{what}: choices differ at groups {np.flatnonzero(c != wc)[:8]}: {c[c != wc][:8]} for {wc[c != wc][:8]}"
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)), f"{what}: scales differ at groups {np.flatnonzero(s.view(np.uint32) != ws.view(np.uint32))[:8]}"
    assert np.array_equal(z, wz), f"{what}: zero points differ at groups {np.flatnonzero(z != wz)[:8]}"
    assert np.array_equal(q, wq), f"{what}: {np.count_nonzero(q != wq)} bytes differ, first at {np.flatnonzero(q != wq)[:8]}"


def spread_ok(choices, qd, G):
    need = {O.UINT2: 3, O.UINT4: 3 if G >= 128 else 2, O.UINT8: 1}[qd]   # Gaussian data; test_the_constructed_grid_groups covers the rest
    return np.unique(choices).size >= need


@pytest.mark.parametrize("G", CC.GROUP_SIZES)
@pytest.mark.parametrize("dt_in,qd", CC.PAIRS)
def test_bit_for_bit_against_the_model(ctx, dt_in, qd, G):
    chunk = CC.chunk_elems(dt_in, qd, G)
    seen = []
    per_chunk = chunk // G
    first = G * min(5, per_chunk - 1) if per_chunk > 1 else G + 3      # a handful of full groups in a partial chunk (G = 4096: one and a ragged one)
    for n in (first, 3 * chunk + G + 5):                               # ... and three full chunks, a full group and a ragged one
        x = CC.as_input(CC.spiky_gaussian(n, 100 + G, G), dt_in)
        want = M.quantize_grouped_clipped(x, dt_in, qd, G, 9)
        seen.append(want[3])
        assert_same(clipped(ctx, x, dt_in, qd, G, 9), want, f"n={n}")
    assert spread_ok(np.concatenate(seen), qd, G), np.bincount(np.concatenate(seen))


@pytest.mark.parametrize("G", CC.GROUP_SIZES)
@pytest.mark.parametrize("dt_in,qd", CC.PAIRS)
def test_the_constructed_grid_groups(ctx, dt_in, qd, G):
    """groups in which a chosen candidate wins on any wire: streaming (the single kernel and, as a batch of two, the batch kernel) and guarded"""
    import piquant

    x = CC.as_input(CC.grid_tensor(G, qd), dt_in)
    want = M.quantize_grouped_clipped(x, dt_in, qd, G, 9)
    assert np.unique(want[3]).size >= CC.grid_min_choices(qd, G), want[3]
    assert_same(clipped(ctx, x, dt_in, qd, G, 9), want, "streaming")
    assert_same(clipped(ctx, x, dt_in, qd, G, 9, shifts=(ESIZE[dt_in], 0, 0, 0, 0)), want, "guarded")
    bufs = [device_buffers(x, dt_in, qd, G) for _ in range(2)]
    ctx.quantize_grouped_clipped_batch_ptr([b[0].ptr for b in bufs], piquant.DataType(dt_in), [b[1].ptr for b in bufs], piquant.DataType(qd), [x.size] * 2, G,
                                           [b[2].ptr for b in bufs], [b[3].ptr for b in bufs], [b[4].ptr for b in bufs], 9, piquant.RoundMode.NEAREST,
                                           _device_ptrs=True)
    torch.cuda.synchronize()
    for b in bufs:
        assert all(u.guards_ok() for u in b)
        assert_same((b[1].get(), b[2].get(np.float32), b[3].get(), b[4].get()), want, "batch")


@pytest.mark.parametrize("steps", [1, 2, 9, 12])
@pytest.mark.parametrize("dt_in,qd,G", [(O.F32, O.UINT2, 128), (O.BF16, O.UINT4, 64), (O.F32, O.UINT4, 1024)])
def test_steps(ctx, dt_in, qd, G, steps):
    x = CC.as_input(CC.spiky_gaussian(CC.chunk_elems(dt_in, qd, G) + 3 * G + 7, 7, G), dt_in)
    got = clipped(ctx, x, dt_in, qd, G, steps)
    assert_same(got, M.quantize_grouped_clipped(x, dt_in, qd, G, steps), f"steps={steps}")
    if steps == 1:
        q, s, z = plain(ctx, x, dt_in, qd, G)
        assert_same(got, (q, s, z, np.zeros_like(got[3])), "steps=1 against quantize_grouped on the device")


@pytest.mark.parametrize("dt_in,qd,G", [(O.F32, O.UINT2, 128), (O.F32, O.UINT8, 32), (O.BF16, O.UINT4, 512), (O.BF16, O.UINT2, 4096)])
def test_stochastic_with_a_pinned_threshold(ctx, dt_in, qd, G):
    x = CC.as_input(CC.spiky_gaussian(2 * CC.chunk_elems(dt_in, qd, G) + G + 3, 8, G), dt_in)
    ctx.set_stochastic_threshold(0.3)
    try:
        got = clipped(ctx, x, dt_in, qd, G, 9, O.STOCHASTIC)
        assert_same(got, M.quantize_grouped_clipped(x, dt_in, qd, G, 9, O.STOCHASTIC, 0.3), "stochastic")
        q, _, _ = plain(ctx, x, dt_in, qd, G, O.STOCHASTIC, given=(got[1], got[2]))
        assert np.array_equal(got[0], q), "not quantize_grouped with the returned parameters given"
    finally:
        ctx.set_stochastic_threshold(None)


@pytest.mark.parametrize("guarded", [False, True], ids=["streaming", "guarded"])
@pytest.mark.parametrize("dt_in,qd,G", [(O.F32, O.UINT4, 128), (O.BF16, O.UINT2, 64), (O.F32, O.UINT2, 1024)])
def test_per_element_mode_indexes_the_global_element_across_2_to_the_32(ctx, dt_in, qd, G, guarded):
    n = 2 * CC.chunk_elems(dt_in, qd, G) + G + 3
    x = CC.as_input(CC.spiky_gaussian(n, 9, G), dt_in)
    seed, base = 0x1234_5678_9ABC_DEF0, (1 << 32) - n // 2   # 2^32 lies inside the tensor
    ctx.set_stochastic_per_element(True, seed=seed, index_base=base)
    try:
        got = clipped(ctx, x, dt_in, qd, G, 9, O.STOCHASTIC, shifts=(ESIZE[dt_in] if guarded else 0, 0, 0, 0, 0))
        s, z, c, _ = M.search(x, dt_in, qd, G, 9)
        assert_same(got, (PE.quantize(x, dt_in, qd, G, seed, base, params=(s, z))[0], s, z, c), "per-element")
        q, _, _ = plain(ctx, x, dt_in, qd, G, O.STOCHASTIC, given=(got[1], got[2]))
        assert np.array_equal(got[0], q), "not quantize_grouped with the returned parameters given"
    finally:
        ctx.set_stochastic_per_element(False)


@pytest.mark.parametrize("dt_in,qd", CC.PAIRS)
def test_edge_groups(ctx, dt_in, qd):
    names = [n for n, _ in CC.EDGE_GROUPS]
    x = CC.as_input(CC.edge_tensor(), dt_in)
    if qd == O.UINT2:
        M.assert_tie(x, dt_in, qd, 32, 9, names.index("tie"), CC.TIE_KS)
    if (dt_in, qd) == (O.F32, O.UINT8):
        M.assert_crosses_short_step_line(x, dt_in, qd, 32, 12, names.index("short_long_line_uint8"))
    for G, steps in ((32, 12), (32, 9), (64, 9)):
        want = M.quantize_grouped_clipped(x, dt_in, qd, G, steps)
        assert_same(clipped(ctx, x, dt_in, qd, G, steps), want, f"G={G} steps={steps}")
        assert_same(clipped(ctx, x, dt_in, qd, G, steps, shifts=(ESIZE[dt_in], 0, 0, 0, 0)), want, f"guarded G={G} steps={steps}")
        if G == 32:
            for n in ("all_nan", "constant", "signed_zeros", "plus_inf", "minus_inf"):
                assert want[3][names.index(n)] == 0
            assert want[3][-1] == 0   # the ragged group


CASES = CC.variant_cases()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_committed_cases(ctx, i):
    """the cases on which every wrong variant of tests/test_grouped_clip_cpu.py shows: streaming and guarded"""
    name, dt_in, qd, G, steps, v = CASES[i]
    x = CC.as_input(v, dt_in)
    want = M.quantize_grouped_clipped(x, dt_in, qd, G, steps)
    assert_same(clipped(ctx, x, dt_in, qd, G, steps), want, "streaming")
    assert_same(clipped(ctx, x, dt_in, qd, G, steps, shifts=(0, 1, 0, 0, 0)), want, "guarded")


@pytest.mark.parametrize("which", range(5), ids=["in", "out", "scales", "zero_points", "choices"])
@pytest.mark.parametrize("dt_in,qd,G", [(O.F32, O.UINT2, 256), (O.BF16, O.UINT4, 128), (O.BF16, O.UINT8, 2048)])
def test_every_buffer_alone_off_a_16_byte_boundary(ctx, dt_in, qd, G, which):
    x = CC.as_input(CC.spiky_gaussian(CC.chunk_elems(dt_in, qd, G) + 2 * G + 11, 21, G), dt_in)
    want = M.quantize_grouped_clipped(x, dt_in, qd, G, 9)
    shifts = [0] * 5
    shifts[which] = (ESIZE[dt_in], 1, 4, 1, 1)[which]
    assert_same(clipped(ctx, x, dt_in, qd, G, 9, shifts=tuple(shifts)), want)


def test_the_guarded_kernel_over_three_trips_of_its_grid_stride_loop(ctx):
    """more groups than two grids of the guarded launch (16 blocks of four waves per CU): the same bytes as the streaming kernel, which the other
    tests pin against the model -- a model run of 10^5 groups would take longer than the rest of this file"""
    num_cu = max(torch.cuda.get_device_properties(0).multi_processor_count, 256)   # the launch assumes 256 CUs where the context knows no count
    G = 32
    n = G * (2 * 16 * 4 * num_cu + 300) + 9
    x = CC.as_input(CC.spiky_gaussian(n, 22, G), O.F32)
    want = clipped(ctx, x, O.F32, O.UINT2, G, 9)
    assert spread_ok(want[3], O.UINT2, G)
    assert_same(clipped(ctx, x, O.F32, O.UINT2, G, 9, shifts=(4, 0, 0, 0, 0)), want)


def test_choices_omitted(ctx):
    x = CC.as_input(CC.spiky_gaussian(5000, 23, 128), O.F32)
    want = M.quantize_grouped_clipped(x, O.F32, O.UINT2, 128, 9)
    for shifts in ((0, 0, 0, 0, 0), (0, 1, 0, 0, 0)):
        q, s, z, c = clipped(ctx, x, O.F32, O.UINT2, 128, 9, shifts=shifts, choices=False)
        assert c is None
        assert_same((q, s, z, None), want)


def test_graph_capture_replayed_on_changed_data(ctx):
    import piquant.torch as pt

    n, G = 20_000 + 77, 128
    a, b = CC.spiky_gaussian(n, 24, G), CC.spiky_gaussian(n, 25, G)
    x = torch.from_numpy(a).cuda()
    pt.quantize_grouped_clipped(x, dtype=torch.quint2x4, group_size=G, return_choices=True)   # eager warm-up (context, code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gq, gs, gz, gc = pt.quantize_grouped_clipped(x, dtype=torch.quint2x4, group_size=G, return_choices=True)
    for v in (b, a):
        x.copy_(torch.from_numpy(v).cuda())
        gs.zero_()
        gc.fill_(99)
        graph.replay()
        torch.cuda.synchronize()
        got = (pt.packed_bytes(gq).cpu().numpy(), gs.cpu().numpy(), gz.cpu().numpy(), gc.cpu().numpy())
        assert_same(got, M.quantize_grouped_clipped(v, O.F32, O.UINT2, G, 9), "replay")


@pytest.mark.parametrize("count", [1, 2, 16, 17])
@pytest.mark.parametrize("dt_in,qd,G", [(O.F32, O.UINT2, 128), (O.BF16, O.UINT4, 32)])
def test_batch_members_equal_the_single_call(ctx, dt_in, qd, G, count):
    """members of different sizes, an empty one, one without choices, one misaligned (it runs alone through the guarded kernel); 17 members are two
    launches"""
    import piquant

    chunk = CC.chunk_elems(dt_in, qd, G)
    sizes = [(chunk + 3 * G + 5, 2 * G, 0, 3 * chunk, G + 1, 7)[i % 6] for i in range(count)]
    if count == 1:
        sizes = [chunk + 3 * G + 5]
    xs = [CC.as_input(CC.spiky_gaussian(n, 30 + i, G), dt_in) for i, n in enumerate(sizes)]
    bufs = [device_buffers(x, dt_in, qd, G, shifts=((ESIZE[dt_in], 0, 0, 0, 0) if i == 4 else (0,) * 5), choices=i != 1) for i, x in enumerate(xs)]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)
    ctx.quantize_grouped_clipped_batch_ptr([b[0].ptr for b in bufs], piquant.DataType(dt_in), [b[1].ptr for b in bufs], piquant.DataType(qd), sizes, G,
                                           [b[2].ptr for b in bufs], [b[3].ptr for b in bufs], [b[4].ptr if b[4] else 0 for b in bufs], 9,
                                           piquant.RoundMode.NEAREST, _device_ptrs=True)
    torch.cuda.synchronize()
    for i, (x, b) in enumerate(zip(xs, bufs)):
        assert all(u is None or u.guards_ok() for u in b), f"member {i}: wrote outside a buffer"
        if x.size == 0:
            continue
        got = (b[1].get(), b[2].get(np.float32), b[3].get(), b[4].get() if b[4] else None)
        assert_same(got, M.quantize_grouped_clipped(x, dt_in, qd, G, 9), f"member {i}")


def test_torch_batch_and_argument_checks(ctx):
    import piquant.torch as pt

    G = 64
    vs = [CC.spiky_gaussian(n, 40 + i, G) for i, n in enumerate((3000, 129, 64 * 40))]
    ts = [torch.from_numpy(v).cuda().to(torch.bfloat16) for v in vs]
    outs, scales, zps, choices = pt.quantize_grouped_clipped_batch(ts, dtype=torch.quint4x2, group_size=G, steps=12, return_choices=True)
    for t, o, s, z, c in zip(ts, outs, scales, zps, choices):
        x = t.view(torch.int16).cpu().numpy().view(np.uint16)
        got = (pt.packed_bytes(o).cpu().numpy(), s.cpu().numpy(), z.cpu().numpy(), c.cpu().numpy())
        assert_same(got, M.quantize_grouped_clipped(x, O.BF16, O.UINT4, G, 12))
        single = pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, steps=12)
        assert len(single) == 3 and torch.equal(pt.packed_bytes(single[0]), pt.packed_bytes(o)) and torch.equal(single[1], s)
    t = ts[0]
    ng = pt.num_groups(t.numel(), G)
    for bad in (0, 13, -1, 2.0, True, None, "9"):
        with pytest.raises(ValueError, match="steps"):
            pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, steps=bad)
        with pytest.raises(ValueError, match="steps"):
            pt.quantize_grouped_clipped_batch(ts, dtype=torch.quint4x2, group_size=G, steps=bad)
    with pytest.raises(ValueError, match="out_choices"):
        pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, out_choices=torch.empty(ng + 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out_choices"):
        pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, out_choices=torch.empty(ng, dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError, match="out_choices"):
        pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, out_choices=torch.empty(ng, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out_scales and out_zero_points"):
        pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, out_scales=torch.empty(ng, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="scales"):
        pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, out_scales=torch.empty(ng + 1, dtype=torch.float32, device="cuda"),
                                    out_zero_points=torch.empty(ng, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="group_size"):
        pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=48)
    with pytest.raises(ValueError):
        pt.quantize_grouped_clipped(t.cpu(), dtype=torch.quint4x2, group_size=G)
    own = torch.empty(ng, dtype=torch.uint8, device="cuda")
    r = pt.quantize_grouped_clipped(t, dtype=torch.quint4x2, group_size=G, steps=12, out_choices=own)
    assert len(r) == 3 and torch.equal(own, choices[0])


@pytest.mark.parametrize("qd,wire", [(O.UINT2, "uint2"), (O.UINT4, "uint4")])
def test_accuracy_on_the_seeded_gaussian(ctx, qd, wire):
    """device round-trip MSE through dequantize_grouped, G = 128: at most the unclipped call's, and the model's value"""
    import piquant

    G, n = 128, 1 << 15
    x = np.random.default_rng(0).standard_normal(n).astype(np.float32)

    def mse(q, s, z):
        qb, sb, zb, ob = Buf(q.nbytes, 0, q), Buf(s.nbytes, 0, s), Buf(z.nbytes, 0, z), Buf(4 * n)
        ctx.dequantize_grouped_ptr(qb.ptr, piquant.DataType(qd), ob.ptr, piquant.DataType.F32, n, G, sb.ptr, zb.ptr, piquant.ReduceOp.SET, _device_ptrs=True)
        torch.cuda.synchronize()
        return float(np.mean((x.astype(np.float64) - ob.get(np.float32).astype(np.float64)) ** 2))

    q1, s1, z1, _ = clipped(ctx, x, O.F32, qd, G, 9)
    q0, s0, z0 = plain(ctx, x, O.F32, qd, G)
    with_search, without = mse(q1, s1, z1), mse(q0, s0, z0)
    print(f"\nclip search, N(0,1), {wire}, G = {G}: round-trip MSE {with_search:.6g} / {without:.6g} = {with_search / without:.3f}")
    assert with_search <= without
    wq, ws, wz, _ = M.quantize_grouped_clipped(x, O.F32, qd, G, 9)
    assert with_search == M.round_trip_mse(x, O.F32, qd, G, wq, ws, wz)
