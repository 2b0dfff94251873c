"""GPU: the one minimum and the one maximum swept through every position class of each min/max reduction, bit for bit.

The tensor is a seeded background inside (-1, 1) with -3 and +5 planted (tests/extremum_positions.py says where, and names each place in the
kernel's own terms: block, round, slot, wave, lane, element), so the expected keys, records and per-group parameters are the same for every
place: the oracle's from [-3, 5].  The places move, the call runs, the results collect in device arrays and come down once per sweep.  Every
launch plants the minimum and the maximum at different places and both roles visit every place (lo and hi are separate chains).

Besides positions, the sweeps execute code nothing else in the suite does: minmax_scalar_kernel (a pointer that is not element-aligned), with it
the large-grid branch of minmax_block_end_gather (2048 blocks), and the LDS-resident rounds 14 to 18 of the fused reduce variant.
One process, one stream; sizes derive from the device's CU count.
"""
import struct

import numpy as np
import pytest

import extremum_positions as X
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QMAX = {O.UINT8: 255, O.UINT4: 15, O.UINT2: 3}
BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
TDT = {O.F32: torch.float32, O.BF16: torch.bfloat16}
ESIZE = {O.F32: 4, O.BF16: 2}
PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
GROUP_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import piquant

    torch.cuda.set_device(0)
    c = piquant.Context()
    c.set_reference_layout(False)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_blocking(False)
    return c


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def DT(code):
    import piquant

    return piquant.DataType(code)


def NEAREST():
    import piquant

    return piquant.RoundMode(O.NEAREST)


def want_params(qd):
    """the one expected (scale, zero point): the oracle's from [-3, 5]"""
    return O.compute_quant_params(np.array([X.LO, X.HI], dtype=np.float32), O.F32, qd)


def want_record(qd):
    scale, zp = want_params(qd)
    return struct.pack("<ffq", scale, float(np.float32(1.0) / np.float32(scale)), zp)


def device_background(n, dt, seed):
    """seeded values inside (-1, 1), all bfloat16-representable, made on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float32) * 1.9375 - 0.96875
    x = (x.view(torch.int32) & -65536).view(torch.float32)
    return x.to(TDT[dt])


class Planted:
    """`n` elements of type dt at `offset` bytes behind a 256-byte boundary, as rows of bytes (so that a tensor that is not element-aligned can be
    written too); plant(i) moves the two extremes to pair i with ONE device-side write, which also restores the previous pair's background."""

    def __init__(self, n, dt, offset, seed, pairs):
        self.n, self.dt, es = n, dt, ESIZE[dt]
        self.buf = torch.zeros(n * es + offset + 256, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.flat = self.buf[offset: offset + n * es]
        self.rows = self.flat.view(n, es)
        self.rows.copy_(device_background(n, dt, seed).view(torch.uint8).view(n, es))
        self.ptr = self.flat.data_ptr()
        self.pairs = np.asarray(pairs, dtype=np.int64)
        P = len(self.pairs)
        idx = np.concatenate([np.roll(self.pairs, 1, axis=0), self.pairs], axis=1)      # previous lo, previous hi, lo, hi
        assert all(len(set(row)) == 4 for row in idx.tolist()), "one write restores the previous pair and plants the next: the four places must differ"
        self.idx = torch.from_numpy(idx).cuda()
        extremes = torch.tensor([float(X.LO), float(X.HI)], dtype=TDT[dt], device="cuda").view(torch.uint8).view(1, 2, es).expand(P, 2, es)
        self.vals = torch.cat([self.rows[self.idx[:, :2].reshape(-1)].view(P, 2, es), extremes], dim=1).contiguous()

    def typed(self):
        return self.flat.view(TDT[self.dt])

    def plant(self, i):
        self.rows.index_copy_(0, self.idx[i], self.vals[i])


def assert_all_rows(got, want_bytes, pairs, describe, what):
    """got: uint8[P, k] downloaded results, one row per launch; every row must equal want_bytes"""
    want = np.frombuffer(want_bytes, dtype=np.uint8)
    bad = np.flatnonzero((got != want[None, :]).any(axis=1))
    if bad.size:
        a, b = (int(v) for v in pairs[bad[0]])
        raise AssertionError(f"{what}: {bad.size} of {len(pairs)} launches differ from the result for [-3, 5]; first: launch {bad[0]}, got {got[bad[0]].tobytes().hex()} "
                             f"want {want_bytes.hex()}\n  minimum at {describe(a)}\n  maximum at {describe(b)}")


def keys_of_extremes():
    """the key pair of (min, max) = (-3, 5): an order-preserving int32 image of the float, of -max for the maximum (csrc/device_math.hpp)"""
    import piquant

    def key(f):
        u = int(np.float32(f).view(np.uint32))
        k = (u ^ 0x7FFFFFFF) if u & 0x80000000 else u
        return k - (1 << 32) if k >= (1 << 31) else k

    k = (key(-3.0), key(-5.0))
    assert piquant.decode_minmax_keys(*k) == O.minmax(np.array([X.LO, X.HI], dtype=np.float32), O.F32) == (-3.0, 5.0), "the test's key function is wrong"
    return struct.pack("<ii", *k)


def sweep_scan(ctx, n, dt, offset, pairs, describe, what, seed=1):
    t = Planted(n, dt, offset, seed, pairs)
    keys = torch.zeros(len(pairs), 2, dtype=torch.int32, device="cuda")
    base = keys.data_ptr()
    for i in range(len(pairs)):
        t.plant(i)
        ctx.minmax_keys_ptr(t.ptr, DT(dt), n, base + 8 * i, init=True, _device_ptrs=True)
    got = keys.cpu().numpy().view(np.uint8).reshape(len(pairs), 8)
    assert_all_rows(got, keys_of_extremes(), t.pairs, describe, what)
    return t


# ---- 1. the per-tensor scan

@pytest.mark.parametrize("dt", [O.F32, O.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("blocks", [1, 2])
def test_scan_every_position_of_one_and_two_blocks(ctx, cus, dt, blocks):
    """just under `blocks` x 2048 vectors, a pointer one element behind a 16-byte boundary (a head of 3 or 7 elements) and a ragged tail: every
    element in both roles"""
    es, epv = ESIZE[dt], X.EPV[ESIZE[dt]]
    head = 16 // es - 1
    n = head + epv * (blocks * X.BLOCK * X.U - 1) + epv - 1
    g = X.ScanGeometry(n, es, head, cus)
    assert g.grid == blocks and g.head == head and g.tail == epv - 1
    sweep_scan(ctx, n, dt, es, X.pair_up(g.every_position()), g.describe, f"scan of {n} elements, {blocks} block(s)")


@pytest.mark.parametrize("dt", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_scan_multi_round_classes_every_block_and_parameters(ctx, cus, dt):
    """a whole first round, a refilled whole round and a ragged round on the full grid: the classes, then every block, then the two epilogues that
    make parameters (the device record and the synchronous call's mailbox)"""
    import piquant

    es, epv = ESIZE[dt], X.EPV[ESIZE[dt]]
    head = 16 // es - 1
    n = X.scan_size_with_every_round_class(es, cus, head=head, tail=epv - 1)
    g = X.ScanGeometry(n, es, head, cus)
    assert g.grid == cus * X.BLOCKS_PER_CU and g.whole == 2 and g.start <= g.last and g.last % 64 != 63
    offset = 16 - head * es
    sweep_scan(ctx, n, dt, offset, X.pair_up(g.class_positions()), g.describe, f"multi-round scan of {n} elements, classes")
    t = sweep_scan(ctx, n, dt, offset, X.pair_up(g.block_positions()), g.describe, f"multi-round scan of {n} elements, every block")
    # parameters: the end of the scan does not depend on the position -- first block, last block, tail, each in both roles
    b_last = g.coords(g.head + g.last * epv)["block"]
    places = [g.element("first", 1, 0, 2, 5, 1), g.element("ragged", 0, b_last, 0, 0, 2), n - 1, g.element("first", 2, 0, 5, 9, 0), g.element("ragged", 0, b_last, 0, 1, 3), n - 2]
    assert g.coords(n - 1)["part"] == g.coords(n - 2)["part"] == "tail"
    pairs = X.pair_up(places)
    t = Planted(n, dt, offset, 2, pairs)
    for qd in (O.UINT8, O.UINT4, O.UINT2):
        recs = torch.zeros(len(pairs), 16, dtype=torch.uint8, device="cuda")
        for i in range(len(pairs)):
            t.plant(i)
            ctx.compute_quant_params_device_ptr(t.ptr, DT(dt), n, DT(qd), recs.data_ptr() + 16 * i, _device_ptrs=True)
        assert_all_rows(recs.cpu().numpy(), want_record(qd), pairs, g.describe, f"compute_quant_params_device, {n} elements, target {qd}")
    for i in range(len(pairs)):
        t.plant(i)
        got = piquant.torch.compute_quant_params(t.typed(), dtype=torch.quint8)
        assert got == want_params(O.UINT8), f"compute_quant_params: {got}\n  minimum at {g.describe(int(pairs[i][0]))}\n  maximum at {g.describe(int(pairs[i][1]))}"
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blocking(False)


@pytest.mark.parametrize("dt", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_scan_of_a_pointer_that_is_not_element_aligned(ctx, cus, dt):
    """minmax_scalar_kernel, one byte off: 8 blocks per CU (2048 on an MI355X: the large-grid gather) with half a grid-stride pass beyond, the
    extremes through every block; then a grid that one wave sweeps"""
    grid = X.SCALAR_BLOCKS_PER_CU * cus
    n = X.scalar_scan_size(grid, cus, beyond=grid * X.BLOCK // 2 + 77)
    g = X.ScalarScanGeometry(n, cus)
    assert g.grid == grid and n > g.nthreads
    sweep_scan(ctx, n, dt, 1, X.pair_up(g.block_positions()), g.describe, f"scalar scan of {n} elements")
    small = min(300, grid)
    n = X.scalar_scan_size(small, cus)
    g = X.ScalarScanGeometry(n, cus)
    assert 2 <= g.grid == small <= X.GATHER_ONE_WAVE + 1
    sweep_scan(ctx, n, dt, 1, X.pair_up(g.block_positions()), g.describe, f"scalar scan of {n} elements")


# ---- 2. the fused quantize_dynamic

def codes_at(out, idx, qd):
    """the codes of elements idx (device int64) in the packed bytes `out`"""
    per = 8 // BITS[qd]
    return (out[idx // per].to(torch.int32) >> ((idx % per) * BITS[qd]).to(torch.int32)) & QMAX[qd]


def assert_planted_codes(codes, qd, pairs, describe, what):
    """codes: int[P, 2], the output codes at the minimum (want 0) and the maximum (want qmax) of each launch"""
    bad = np.flatnonzero((codes[:, 0] != 0) | (codes[:, 1] != QMAX[qd]))
    if bad.size:
        a, b = (int(v) for v in pairs[bad[0]])
        raise AssertionError(f"{what}: the codes at the planted places are wrong in {bad.size} launches; first: launch {bad[0]}, got {tuple(codes[bad[0]])} want (0, {QMAX[qd]})\n"
                             f"  minimum at {describe(a)}\n  maximum at {describe(b)}")


@pytest.mark.parametrize("dt,qd", PAIRS)
def test_fused_batch_of_16_every_round_wave_and_tail(ctx, cus, dt, qd):
    """one member with 27 resident rounds plus a ragged streamed batch per block of its sub-grid, 15 tiny ones"""
    es = ESIZE[dt]
    n, G = X.fused_batch_big_numel(es, cus)
    g = X.FusedGeometry(n, es, G)
    assert min(g.rounds_of(b) for b in range(G)) >= X.F_REG + X.F_LDS + 2 and g.tail == 3
    full = (dt, qd) in ((O.F32, O.UINT8), (O.BF16, O.UINT4))
    positions = g.class_positions() if full else g.class_positions(waves=[5], lanes=[29])
    t = Planted(n, dt, 0, 3, X.pair_up(positions))
    P = len(t.pairs)
    rng = np.random.default_rng(7)
    fillers = [rng.uniform(-2, 2, int(m)).astype(np.float32) for m in rng.integers(100, 3000, 15)]
    fillers = [f if dt == O.F32 else O.f32_to_bf16(f) for f in fillers]
    fdev = [torch.from_numpy(f.view(np.uint8).copy()).cuda() for f in fillers]
    outs = [torch.zeros(O.packed_numel(n, qd), dtype=torch.uint8, device="cuda")] + [torch.zeros(O.packed_numel(f.size, qd), dtype=torch.uint8, device="cuda") for f in fillers]
    recs = torch.zeros(P, 16, 16, dtype=torch.uint8, device="cuda")
    codes = torch.zeros(P, 2, dtype=torch.int32, device="cuda")
    ptrs_in = [t.ptr] + [f.data_ptr() for f in fdev]
    ptrs_out = [o.data_ptr() for o in outs]
    numels = [n] + [f.size for f in fillers]
    assert all(p % 16 == 0 for p in ptrs_in + ptrs_out)
    for i in range(P):
        t.plant(i)
        ctx.quantize_dynamic_batch_ptr(ptrs_in, DT(dt), ptrs_out, DT(qd), numels, [recs.data_ptr() + (16 * i + m) * 16 for m in range(16)], NEAREST(), _device_ptrs=True)
        codes[i] = codes_at(outs[0], t.idx[i, 2:], qd)
    got = recs.cpu().numpy()
    what = f"quantize_dynamic_batch {dt} -> {qd}, member 0 of {n} elements"
    assert_all_rows(got[:, 0], want_record(qd), t.pairs, g.describe, what)
    assert_planted_codes(codes.cpu().numpy(), qd, t.pairs, g.describe, what)
    for m, f in enumerate(fillers, 1):
        scale, zp = O.compute_quant_params(f, dt, qd)
        rec = struct.pack("<ffq", scale, float(np.float32(1.0) / np.float32(scale)), zp)
        assert_all_rows(got[:, m], rec, t.pairs, g.describe, f"{what}: the record of filler {m}")
    assert ctx.barrier_bailouts() == 0


def test_fused_single_call_at_the_full_chip_size(ctx, cus):
    n = (X.F_REG + X.F_LDS) * X.FBLOCK * cus * 4 + 4
    G = X.fused_blocks_per_group(n, 4, 1, cus)
    g = X.FusedGeometry(n, 4, G)
    assert G == cus
    t = Planted(n, O.F32, 0, 4, X.pair_up(g.class_positions(waves=[9], lanes=[40])))
    P = len(t.pairs)
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(P, 16, dtype=torch.uint8, device="cuda")
    codes = torch.zeros(P, 2, dtype=torch.int32, device="cuda")
    for i in range(P):
        t.plant(i)
        ctx.quantize_dynamic_ptr(t.ptr, DT(O.F32), out.data_ptr(), DT(O.UINT8), n, recs.data_ptr() + 16 * i, NEAREST(), _device_ptrs=True)
        codes[i] = codes_at(out, t.idx[i, 2:], O.UINT8)
    what = f"quantize_dynamic float32 -> uint8 of {n} elements"
    assert_all_rows(recs.cpu().numpy(), want_record(O.UINT8), t.pairs, g.describe, what)
    assert_planted_codes(codes.cpu().numpy(), O.UINT8, t.pairs, g.describe, what)
    assert ctx.barrier_bailouts() == 0


@pytest.mark.parametrize("dt", [O.F32, O.BF16], ids=["f32", "bf16"])
def test_fused_reduce_every_resident_round(ctx, cus, dt):
    """19 rounds per block: register rounds 0 to 9 and LDS rounds 10 to 18 of the reduce variant.  The extremes come from the TERM: codes equal to
    the zero point (3) everywhere but 0 and 8 at the planted places, scale 1, and an accumulator that is exactly 0 there"""
    es, epv = ESIZE[dt], X.EPV[ESIZE[dt]]
    n = 19 * X.FBLOCK * cus * epv
    G = X.fused_blocks_per_group(n, es, 1, cus)
    g = X.FusedGeometry(n, es, G, X.F_RED_REG)
    assert G == cus and {g.rounds_of(b) for b in range(G)} == {19} and g.kind(18) == "LDS"
    pairs = X.pair_up(g.class_positions(waves=[9], lanes=[40]))
    P = len(pairs)
    acc0 = device_background(n, dt, 5)
    acc = torch.empty_like(acc0)
    term = torch.full((n,), 3, dtype=torch.uint8, device="cuda")
    idx = torch.from_numpy(np.concatenate([np.roll(pairs, 1, axis=0), pairs], axis=1)).cuda()
    vals = torch.tensor([3, 3, 0, 8], dtype=torch.uint8, device="cuda")
    term_rec = torch.from_numpy(np.frombuffer(struct.pack("<ffq", 1.0, 1.0, 3), dtype=np.uint8).copy()).cuda()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(P, 16, dtype=torch.uint8, device="cuda")
    codes = torch.zeros(P, 2, dtype=torch.int32, device="cuda")
    for i in range(P):
        acc.copy_(acc0)   # the call leaves the accumulator unspecified
        acc.index_fill_(0, idx[i, 2:], 0.0)
        term.index_copy_(0, idx[i], vals)
        ctx.reduce_quantize_dynamic_ptr(acc.data_ptr(), DT(dt), [term.data_ptr()], [term_rec.data_ptr()], out.data_ptr(), DT(O.UINT8), n, recs.data_ptr() + 16 * i, NEAREST(),
                                        _device_ptrs=True)
        codes[i] = codes_at(out, idx[i, 2:], O.UINT8)
    what = f"reduce_quantize_dynamic {dt} -> uint8 of {n} elements, one term"
    assert_all_rows(recs.cpu().numpy(), want_record(O.UINT8), pairs, g.describe, what)
    assert_planted_codes(codes.cpu().numpy(), O.UINT8, pairs, g.describe, what)
    assert torch.equal(acc.view(torch.uint8), acc0.index_fill(0, idx[P - 1, 2:], 0.0).view(torch.uint8)), "the one-launch reduce does not write the accumulator: was it taken?"


# ---- 3. the grouped kernels

def pack_codes(codes, qd, n):
    """device uint8 codes[n] -> packed bytes (bits behind the tensor's end zero)"""
    per = 8 // BITS[qd]
    padded = torch.zeros(O.packed_numel(n, qd) * per, dtype=torch.uint8, device="cuda")
    padded[:n] = codes
    q = torch.zeros(padded.numel() // per, dtype=torch.uint8, device="cuda")
    for j in range(per):
        q |= padded[j::per] << (j * BITS[qd])
    return q


class GroupedCase:
    def __init__(self, G, dt, seed):
        self.G, self.dt = G, dt
        self.n, lo, hi = X.grouped_sweep(G)
        self.ng = 2 * G + 1
        self.lo, self.hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
        self.lo_h, self.hi_h = lo, hi
        self.bg = device_background(self.n, dt, seed)
        self.x = self.bg.clone()
        self.x[self.lo], self.x[self.hi] = float(X.LO), float(X.HI)

    def shifted(self, t):
        """a copy of t that starts one element behind a 16-byte boundary"""
        buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda")
        v = buf[1: 1 + t.numel()]
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size()
        return v

    def check(self, scales, zps, out, qd, tile_esize, what):
        """every group's parameters equal the one expected pair; the codes at the planted places are 0 and qmax"""
        tile = X.GroupedTile(self.G, tile_esize, BITS[qd])
        ws, wz = want_params(qd)
        s, z = scales.cpu().numpy(), zps.cpu().numpy()
        bad = np.flatnonzero((s.view(np.uint32) != np.float32(ws).view(np.uint32)) | (z != wz))
        if bad.size:
            b = int(bad[0])
            raise AssertionError(f"{what}: the parameters of {bad.size} of {self.ng} groups differ from ({ws!r}, {wz}); first: group {b} got ({s[b]!r}, {z[b]})\n"
                                 f"  minimum at {tile.describe(int(self.lo_h[b]))}\n  maximum at {tile.describe(int(self.hi_h[b]))}")
        if out is not None:
            c = torch.stack([codes_at(out, self.lo, qd), codes_at(out, self.hi, qd)], dim=1).cpu().numpy()
            assert_planted_codes(c, qd, np.stack([self.lo_h, self.hi_h], axis=1), tile.describe, what)

    def buffers(self, qd, shift_out=0):
        nb = O.packed_numel(self.n, qd)
        obuf = torch.zeros(nb + 32, dtype=torch.uint8, device="cuda")
        return obuf[shift_out: shift_out + nb], torch.zeros(self.ng, dtype=torch.float32, device="cuda"), torch.full((self.ng,), 77, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_grouped_every_position_of_a_group(ctx, G):
    """2 G whole groups and a ragged one; group g has its minimum at g mod G and its maximum at (g + G / 2) mod G.  quantize_grouped (streaming and
    guarded), quantize_dequantize_grouped, quantize_grouped_ef (extremes in x, then in the residual), reduce_quantize_grouped and its _ef form
    (extremes produced by a term), all six pairs"""
    rm = NEAREST()
    for dt in (O.F32, O.BF16):
        es = ESIZE[dt]
        c = GroupedCase(G, dt, G + dt)
        n, x = c.n, c.x
        x_off = c.shifted(x)
        for qd in (O.UINT8, O.UINT4, O.UINT2):
            what = f"G={G} {dt} -> {qd}"
            out, s, z = c.buffers(qd)
            ctx.quantize_grouped_ptr(x.data_ptr(), DT(dt), out.data_ptr(), DT(qd), n, G, s.data_ptr(), z.data_ptr(), False, rm, _device_ptrs=True)
            c.check(s, z, out, qd, es, what + " quantize_grouped")
            out, s, z = c.buffers(qd, shift_out=1)
            ctx.quantize_grouped_ptr(x_off.data_ptr(), DT(dt), out.data_ptr(), DT(qd), n, G, s.data_ptr(), z.data_ptr(), False, rm, _device_ptrs=True)
            c.check(s, z, out, qd, es, what + " quantize_grouped, guarded kernel")
            # quantize-dequantize: parameters returned, the planted places come back as dequantize(0) and dequantize(qmax)
            _, s, z = c.buffers(qd)
            y = torch.zeros_like(x)
            ctx.quantize_dequantize_grouped_ptr(x.data_ptr(), DT(dt), y.data_ptr(), DT(qd), n, G, s.data_ptr(), z.data_ptr(), False, rm, _set_op(), _device_ptrs=True)
            c.check(s, z, None, qd, es, what + " quantize_dequantize_grouped")
            ws, wz = want_params(qd)
            ends = O.dequantize(np.array([QMAX[qd] << BITS[qd]] if qd != O.UINT8 else [0, 255], dtype=np.uint8), qd, dt, 2, ws, wz)
            ends_d = torch.from_numpy(ends.view(np.uint8).copy()).cuda().view(TDT[dt])
            assert torch.equal(y[c.lo].view(torch.uint8), ends_d[0].expand(c.ng).contiguous().view(torch.uint8)), what + " quantize_dequantize_grouped: values at the minima"
            assert torch.equal(y[c.hi].view(torch.uint8), ends_d[1].expand(c.ng).contiguous().view(torch.uint8)), what + " quantize_dequantize_grouped: values at the maxima"
            # error feedback: kinds f32 / bf16 (residual of the tensor's type) and mixed (bfloat16 tensor, float32 residual)
            for rdt in ((O.F32,) if dt == O.F32 else (O.BF16, O.F32)):
                kind = "mixed" if rdt != dt else ("f32" if dt == O.F32 else "bf16")
                for carrier in ("x", "residual"):
                    if carrier == "x":
                        xin, r = x, torch.zeros(n, dtype=TDT[rdt], device="cuda")
                    else:   # x = 0.5 at the planted places, the residual carries -3.5 and 4.5: x + r is exact
                        xin, r = c.bg.clone(), torch.zeros(n, dtype=TDT[rdt], device="cuda")
                        xin[c.lo], xin[c.hi] = 0.5, 0.5
                        r[c.lo], r[c.hi] = -3.5, 4.5
                    out, s, z = c.buffers(qd)
                    ctx.quantize_grouped_ef_ptr(xin.data_ptr(), DT(dt), r.data_ptr(), out.data_ptr(), DT(qd), n, G, s.data_ptr(), z.data_ptr(), rm, _device_ptrs=True,
                                                residual_dtype=DT(rdt) if rdt != dt else None)
                    c.check(s, z, out, qd, ESIZE[rdt], what + f" quantize_grouped_ef ({kind}), extremes carried by {carrier}")
            # the reduce: term codes 1 (the zero point) everywhere, 0 and 2 at the planted places, scale 4; the accumulator is 1 there: -4 + 1 and 4 + 1
            codes = torch.ones(n, dtype=torch.uint8, device="cuda")
            codes[c.lo], codes[c.hi] = 0, 2
            tq = pack_codes(codes, qd, n)
            ts, tz = torch.full((c.ng,), 4.0, dtype=torch.float32, device="cuda"), torch.ones(c.ng, dtype=torch.uint8, device="cuda")
            acc0 = c.bg.clone()
            acc0[c.lo], acc0[c.hi] = 1.0, 1.0
            acc = acc0.clone()
            out, s, z = c.buffers(qd)
            ctx.reduce_quantize_grouped_ptr(acc.data_ptr(), DT(dt), [tq.data_ptr()], [ts.data_ptr()], [tz.data_ptr()], out.data_ptr(), DT(qd), n, G, s.data_ptr(), z.data_ptr(), rm,
                                            _device_ptrs=True)
            c.check(s, z, out, qd, es, what + " reduce_quantize_grouped, one term")
            for rdt in ((O.F32,) if dt == O.F32 else (O.BF16, O.F32)):
                acc = acc0.clone()
                r = torch.zeros(n, dtype=TDT[rdt], device="cuda")
                out, s, z = c.buffers(qd)
                ctx.reduce_quantize_grouped_ef_ptr(acc.data_ptr(), DT(dt), r.data_ptr(), [tq.data_ptr()], [ts.data_ptr()], [tz.data_ptr()], out.data_ptr(), DT(qd), n, G, s.data_ptr(),
                                                   z.data_ptr(), rm, _device_ptrs=True, residual_dtype=DT(rdt) if rdt != dt else None)
                c.check(s, z, out, qd, ESIZE[rdt], what + f" reduce_quantize_grouped_ef, residual {rdt}, one term")


def _set_op():
    import piquant

    return piquant.ReduceOp(O.SET)


@pytest.mark.parametrize("G", [64, 512])
def test_grouped_batch_of_17(ctx, G):
    """17 members (two launches), each the whole sweep with its own background"""
    for dt, qd in ((O.F32, O.UINT8), (O.BF16, O.UINT4)):
        cases = [GroupedCase(G, dt, 100 + m) for m in range(17)]
        bufs = [c.buffers(qd) for c in cases]
        ctx.quantize_grouped_batch_ptr([c.x.data_ptr() for c in cases], DT(dt), [b[0].data_ptr() for b in bufs], DT(qd), [c.n for c in cases], G, [b[1].data_ptr() for b in bufs],
                                       [b[2].data_ptr() for b in bufs], False, NEAREST(), _device_ptrs=True)
        for m, (c, (out, s, z)) in enumerate(zip(cases, bufs)):
            c.check(s, z, out, qd, ESIZE[dt], f"G={G} {dt} -> {qd} quantize_grouped_batch member {m}")
