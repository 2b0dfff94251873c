"""The batched rotated grouped launches on the MI355X: piquant.torch.quantize_grouped_rotated_batch / dequantize_grouped_rotated_batch /
quantize_grouped_rotated_ef_batch against the CPU models (tests/rot_model.py, tests/rot_ef_model.py) and against the single rotated call on every
member, bit for bit -- NaN positions are compared, NaN payloads are not -- and piquant.distributed._DeviceOps on them.

A batch is its members, not their concatenation: member sizes come from either side of every chunk size of the float32 tile (1 024, 2 048 and
4 096 elements), from the group size's own edges (0, 1, G - 1, G, G + 1, 3 G + 5) and from two sizes of several chunks (10 007, 40 037); from four
members on, member 2 sits one element off a 16-byte boundary, so the guarded single launch runs in its place in the sequence.  Every output, scale,
zero-point and residual buffer is carved from canary-filled storage."""
import functools

import numpy as np
import pytest

import oracle as O
import rot_ef_model as RE
import rot_model as R
import test_gpu_grouped_rotated as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ctx = T.ctx   # the module's context fixture: threshold and per-element mode restored at the end

SEED = T.SEED
INDEX_BASE = (1 << 32) - 5   # the per-element index crosses 2^32 inside every member of six elements or more, and restarts in each member
GROUPS_GRID = (32, 128, 4096)
WIDTH_PAIRS = [(O.F32, O.UINT8), (O.BF16, O.UINT4), (O.F32, O.UINT2)]
WIDTH_IDS = ["f32-u8", "bf16-u4", "f32-u2"]
MISALIGNED = 2               # the member that is one element off a 16-byte boundary, in batches of four members or more
MODES = ("nearest", "stochastic", "per element")


def member_sizes(count, G):
    """the first `count` of: several chunks, empty, a ragged end behind whole groups, the sizes around G and around every chunk size"""
    pool = [40037, 0, 3 * G + 5, G - 1, 4097, 1, 1024, G, 2049, 4095, G + 1, 1023, 2048, 10007, 1025, 2047, 4096]
    assert count <= len(pool)
    return pool[:count]


def offsets(count):
    return [1 if count >= 4 and i == MISALIGNED else 0 for i in range(count)]


def arm(ctx, mode):
    """-> the call's round_mode"""
    ctx.set_stochastic_per_element(False)
    ctx.set_stochastic_threshold(None)
    if mode == "stochastic":
        ctx.set_stochastic_threshold(T.THRESHOLD)
    elif mode == "per element":
        ctx.set_stochastic_per_element(True, seed=T.ELEM_SEED, index_base=INDEX_BASE)
    return "nearest" if mode == "nearest" else "stochastic"


def restore(ctx):
    ctx.set_stochastic_threshold(None)
    ctx.set_stochastic_per_element(False)


def member_data(i, n, dt, G):
    return T.data(n, dt, G, seed=10 + i)   # different per member


@functools.lru_cache(maxsize=None)
def model_quantize(i, n, dt, qd, G, mode):
    x = member_data(i, n, dt, G)
    if mode == "nearest":
        return R.quantize_grouped_rotated(x, dt, qd, G, SEED)
    if mode == "stochastic":
        return R.quantize_grouped_rotated(x, dt, qd, G, SEED, O.STOCHASTIC, T.THRESHOLD)
    return R.quantize_grouped_rotated_per_element(x, dt, qd, G, SEED, T.ELEM_SEED, INDEX_BASE, start=0)


def residual_of(i, n, G):
    """a non-zero float32 residual of the size one step leaves: a hundredth of heavy-tailed values"""
    return (np.array(T.data(n, O.F32, G, seed=40 + i)) * np.float32(0.01)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model_ef(i, n, dt, qd, G, mode):
    x, r = member_data(i, n, dt, G), residual_of(i, n, G)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "nearest":
            return RE.quantize_grouped_rotated_ef(x, dt, r, qd, G, SEED)
        if mode == "stochastic":
            return RE.quantize_grouped_rotated_ef(x, dt, r, qd, G, SEED, O.STOCHASTIC, T.THRESHOLD)
        return RE.reduce_quantize_grouped_rotated_ef_per_element(x, dt, r, [], qd, G, SEED, T.ELEM_SEED, INDEX_BASE)


def put(a, tdtype, off=0):
    """a host array in a carved device buffer, `off` elements behind a 16-byte boundary -> (buffer, tensor, first byte)"""
    buf, t, first = T.carve(a.size, tdtype, off)
    if a.size:
        h = torch.from_numpy(np.array(a))   # a copy: the cached inputs are read-only
        t.copy_(h.view(tdtype) if tdtype == torch.bfloat16 else h)
    return buf, t, first


def put_float(x, dt, off=0):
    return put(x.view(np.int16) if dt == O.BF16 else x, T.FDT[dt], off)


class Carved:
    """the output buffers of one batch: packed bytes, scales, zero points per member, each in canary-filled storage of its own"""

    def __init__(self, sizes, qd, G, offs):
        self.sizes, self.qd, self.G = sizes, qd, G
        self.q = [T.carve(T.packed_nbytes(n, qd), torch.uint8, off) for n, off in zip(sizes, offs)]
        self.s = [T.carve((n + G - 1) // G, torch.float32) for n in sizes]
        self.z = [T.carve((n + G - 1) // G, torch.uint8) for n in sizes]

    def kw(self):
        return dict(outs=[c[1] for c in self.q], out_scales=[c[1] for c in self.s], out_zero_points=[c[1] for c in self.z])

    def check(self, what):
        for i, n in enumerate(self.sizes):
            ng = (n + self.G - 1) // self.G
            T.canaries_intact(self.q[i][0], self.q[i][2], T.packed_nbytes(n, self.qd), f"{what}: packed bytes of member {i}")
            T.canaries_intact(self.s[i][0], self.s[i][2], ng * 4, f"{what}: scales of member {i}")
            T.canaries_intact(self.z[i][0], self.z[i][2], ng, f"{what}: zero points of member {i}")

    def host(self, i):
        return self.q[i][1].cpu().numpy(), self.s[i][1].cpu().numpy(), self.z[i][1].cpu().numpy()


def quantize_batch(xs, sizes, qd, G, round_mode, offs_out=None):
    """quantize_grouped_rotated_batch into carved buffers -> [(bytes, scales, zero points)] on the host, canaries checked"""
    import piquant.torch as pt

    c = Carved(sizes, qd, G, offs_out or [0] * len(sizes))
    got = pt.quantize_grouped_rotated_batch(xs, dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode=round_mode, **c.kw())
    torch.cuda.synchronize()
    assert all(a is b[1] for a, b in zip(got[0], c.q)) and all(a is b[1] for a, b in zip(got[1], c.s)) and all(a is b[1] for a, b in zip(got[2], c.z))
    c.check("quantize_grouped_rotated_batch")
    return [c.host(i) for i in range(len(sizes))]


def ef_batch(xs, rs_host, sizes, qd, G, round_mode, offs_res=None):
    """quantize_grouped_rotated_ef_batch into carved buffers, the residuals in carved buffers of their own -> [(bytes, scales, zero points,
    residual)] on the host, canaries checked"""
    import piquant.torch as pt

    offs_res = offs_res or [0] * len(sizes)
    c = Carved(sizes, qd, G, [0] * len(sizes))
    rs = [put(r, torch.float32, off) for r, off in zip(rs_host, offs_res)]
    pt.quantize_grouped_rotated_ef_batch(xs, [r[1] for r in rs], dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode=round_mode, **c.kw())
    torch.cuda.synchronize()
    c.check("quantize_grouped_rotated_ef_batch")
    for i, n in enumerate(sizes):
        T.canaries_intact(rs[i][0], rs[i][2], n * 4, f"residual of member {i}")
    return [c.host(i) + (rs[i][1].cpu().numpy(),) for i in range(len(sizes))]


def ef_single(x, r_host, qd, G, round_mode):
    import piquant.torch as pt

    r = torch.from_numpy(r_host.copy()).cuda()
    q, s, z = pt.quantize_grouped_rotated_ef(x, r, dtype=T.QDT[qd], group_size=G, seed=SEED, round_mode=round_mode)
    return (pt.packed_bytes(q).cpu().numpy() if x.numel() else np.zeros(0, dtype=np.uint8)), s.cpu().numpy(), z.cpu().numpy(), r.cpu().numpy()


def quad_same(got, want, what):
    T.triple_same(got[:3], want[:3], what)
    T.same(got[3], np.asarray(want[3], dtype=np.float32), what + ": residual")


# ---- 1. quantize_grouped_rotated_batch

def check_quantize(ctx, dt, qd, G, count):
    sizes, offs = member_sizes(count, G), offsets(count)
    ins = [put_float(member_data(i, n, dt, G), dt, off) for i, (n, off) in enumerate(zip(sizes, offs))]
    xs = [t[1] for t in ins]
    assert count < 4 or xs[MISALIGNED].data_ptr() % 16 != 0
    try:
        for mode in MODES:
            round_mode = arm(ctx, mode)
            got = quantize_batch(xs, sizes, qd, G, round_mode)
            for i, n in enumerate(sizes):
                T.triple_same(got[i], model_quantize(i, n, dt, qd, G, mode), f"{mode}, member {i} (n={n}): model")
                T.triple_same(got[i], T.quantize_rotated(T.dev(member_data(i, n, dt, G), dt), qd, G, SEED, round_mode), f"{mode}, member {i} (n={n}): single call")
    finally:
        restore(ctx)
    for i, (n, (buf, t, first)) in enumerate(zip(sizes, ins)):
        T.same(T.host(t), member_data(i, n, dt, G), f"the input of member {i}")
        T.canaries_intact(buf, first, n * t.element_size(), f"the input of member {i}")


@pytest.mark.parametrize("count", (1, 2, 5, 16, 17))
@pytest.mark.parametrize("G", GROUPS_GRID)
@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_quantize_batch(ctx, pair, G, count):
    check_quantize(ctx, pair[0], pair[1], G, count)


@pytest.mark.parametrize("G", T.GROUP_SIZES)
@pytest.mark.parametrize("pair", WIDTH_PAIRS, ids=WIDTH_IDS)
def test_quantize_batch_every_group_size(ctx, pair, G):
    check_quantize(ctx, pair[0], pair[1], G, 3)


# ---- 2. dequantize_grouped_rotated_batch

def check_dequantize(ctx, dt, qd, G, count, op, raw):
    import piquant.torch as pt

    restore(ctx)
    sizes, offs = member_sizes(count, G), offsets(count)
    recs = [model_quantize(i, n, O.F32, qd, G, "nearest") for i, n in enumerate(sizes)]
    prevs = [T.data(n, dt, G, seed=70 + i) for i, n in enumerate(sizes)]   # ADD: the accumulators hold other data
    if raw:   # raw uint8 buffers of the packed bytes, with quant_dtype= and shapes=
        qs = [torch.from_numpy(np.asarray(q, dtype=np.uint8)).cuda() for q, _, _ in recs]
        kw = dict(quant_dtype=T.QDT[qd], shapes=[(n,) for n in sizes])
    else:     # packed tensors
        qs = []
        for (q, _, _), n in zip(recs, sizes):
            t = torch.empty(n, dtype=T.QDT[qd], device="cuda")
            if n:
                pt.packed_bytes(t).copy_(torch.from_numpy(np.asarray(q, dtype=np.uint8)))
            qs.append(t)
        kw = {}
    ss = [torch.from_numpy(np.asarray(s, dtype=np.float32)).cuda() for _, s, _ in recs]
    zs = [torch.from_numpy(np.asarray(z, dtype=np.uint8)).cuda() for _, _, z in recs]
    outs = [put_float(p, dt, off) for p, off in zip(prevs, offs)]
    assert count < 4 or outs[MISALIGNED][1].data_ptr() % 16 != 0
    got = pt.dequantize_grouped_rotated_batch(qs, ss, zs, dtype=T.FDT[dt], group_size=G, seed=SEED, reduce_op=op, outs=[o[1] for o in outs], **kw)
    torch.cuda.synchronize()
    assert all(a is b[1] for a, b in zip(got, outs))
    for i, (n, (q, s, z)) in enumerate(zip(sizes, recs)):
        T.canaries_intact(outs[i][0], outs[i][2], n * outs[i][1].element_size(), f"out of member {i}")
        want = R.dequantize_grouped_rotated(q, qd, dt, n, G, s, z, SEED, O.ADD if op == "add" else O.SET, prevs[i])
        T.same(T.host(outs[i][1]), want, f"{op}, member {i} (n={n}): model")
        single = T.dev(prevs[i], dt)
        pt.dequantize_grouped_rotated(qs[i], ss[i], zs[i], dtype=T.FDT[dt], group_size=G, seed=SEED, reduce_op=op, out=single,
                                      **(dict(quant_dtype=T.QDT[qd], shape=(n,)) if raw else {}))
        T.same(T.host(outs[i][1]), T.host(single), f"{op}, member {i} (n={n}): single call")
    if op == "set":   # allocated outputs have the members' shapes
        fresh = pt.dequantize_grouped_rotated_batch(qs, ss, zs, dtype=T.FDT[dt], group_size=G, seed=SEED, **kw)
        for i, n in enumerate(sizes):
            assert fresh[i].shape == (n,)
            T.same(T.host(fresh[i]), T.host(outs[i][1]), f"allocated out of member {i}")


@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("count", (1, 3, 16, 17))
@pytest.mark.parametrize("G", GROUPS_GRID)
@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_dequantize_batch(ctx, pair, G, count, op):
    check_dequantize(ctx, pair[0], pair[1], G, count, op, raw=(count % 2 == 1))   # raw buffers and packed tensors, by turns


@pytest.mark.parametrize("op", ("set", "add"))
@pytest.mark.parametrize("G", T.GROUP_SIZES)
@pytest.mark.parametrize("pair", WIDTH_PAIRS, ids=WIDTH_IDS)
def test_dequantize_batch_every_group_size(ctx, pair, G, op):
    check_dequantize(ctx, pair[0], pair[1], G, 3, op, raw=(op == "set"))


# ---- 3. quantize_grouped_rotated_ef_batch

def check_ef(ctx, dt, qd, G, count):
    sizes, offs = member_sizes(count, G), offsets(count)
    xs = [T.dev(member_data(i, n, dt, G), dt) for i, n in enumerate(sizes)]
    rs = [residual_of(i, n, G) for i, n in enumerate(sizes)]
    try:
        for mode in MODES:
            round_mode = arm(ctx, mode)
            got = ef_batch(xs, rs, sizes, qd, G, round_mode, offs)
            for i, n in enumerate(sizes):
                quad_same(got[i], model_ef(i, n, dt, qd, G, mode), f"{mode}, member {i} (n={n}): model")
                quad_same(got[i], ef_single(xs[i], rs[i], qd, G, round_mode), f"{mode}, member {i} (n={n}): single call")
    finally:
        restore(ctx)
    for i, n in enumerate(sizes):
        T.same(T.host(xs[i]), member_data(i, n, dt, G), f"the tensor of member {i} is only read")


@pytest.mark.parametrize("count", (1, 2, 5, 16, 17))
@pytest.mark.parametrize("G", GROUPS_GRID)
@pytest.mark.parametrize("pair", T.PAIRS, ids=T.PAIR_IDS)
def test_ef_batch(ctx, pair, G, count):
    check_ef(ctx, pair[0], pair[1], G, count)


@pytest.mark.parametrize("G", T.GROUP_SIZES)
@pytest.mark.parametrize("pair", WIDTH_PAIRS, ids=WIDTH_IDS)
def test_ef_batch_every_group_size(ctx, pair, G):
    check_ef(ctx, pair[0], pair[1], G, 3)


@pytest.mark.parametrize("pair", WIDTH_PAIRS, ids=WIDTH_IDS)
def test_two_chained_ef_batches(ctx, pair):
    """the first batch's residuals feed the second: the same as two chained rounds of single calls"""
    import piquant.torch as pt

    dt, qd = pair
    G, sizes = 128, member_sizes(5, 128)
    restore(ctx)
    steps = [[T.dev(T.data(n, dt, G, seed=80 + 10 * step + i), dt) for i, n in enumerate(sizes)] for step in range(2)]
    batch_r = [put(residual_of(i, n, G), torch.float32) for i, n in enumerate(sizes)]
    single_r = [torch.from_numpy(residual_of(i, n, G).copy()).cuda() for i, n in enumerate(sizes)]
    for step, xs in enumerate(steps):
        c = Carved(sizes, qd, G, [0] * len(sizes))
        pt.quantize_grouped_rotated_ef_batch(xs, [r[1] for r in batch_r], dtype=T.QDT[qd], group_size=G, seed=SEED, **c.kw())
        torch.cuda.synchronize()
        c.check(f"step {step}")
        for i, n in enumerate(sizes):
            q, s, z = pt.quantize_grouped_rotated_ef(xs[i], single_r[i], dtype=T.QDT[qd], group_size=G, seed=SEED)
            want = (pt.packed_bytes(q).cpu().numpy() if n else np.zeros(0, dtype=np.uint8)), s.cpu().numpy(), z.cpu().numpy(), single_r[i].cpu().numpy()
            quad_same(c.host(i) + (batch_r[i][1].cpu().numpy(),), want, f"step {step}, member {i} (n={n})")
            T.canaries_intact(batch_r[i][0], batch_r[i][2], n * 4, f"step {step}: residual of member {i}")
    assert any(np.any(r.cpu().numpy() != residual_of(i, n, G)) for i, (n, r) in enumerate(zip(sizes, single_r)) if n)


# ---- more streaming members than one launch takes: a launch per sixteen

@pytest.mark.parametrize("pair", WIDTH_PAIRS, ids=WIDTH_IDS)
def test_more_than_sixteen_streaming_members(ctx, pair):
    """nineteen aligned, non-empty members: sixteen go out in the first launch and three in the second"""
    import piquant.torch as pt

    dt, qd = pair
    G = 128
    sizes = [G * (i % 5) + 7 * i + 1 for i in range(19)]
    restore(ctx)
    xs = [T.dev(member_data(i, n, dt, G), dt) for i, n in enumerate(sizes)]
    got = quantize_batch(xs, sizes, qd, G, "nearest")
    for i, n in enumerate(sizes):
        T.triple_same(got[i], model_quantize(i, n, dt, qd, G, "nearest"), f"quantize, member {i} (n={n})")
    rs = [residual_of(i, n, G) for i, n in enumerate(sizes)]
    for i, quad in enumerate(ef_batch(xs, rs, sizes, qd, G, "nearest")):
        quad_same(quad, model_ef(i, sizes[i], dt, qd, G, "nearest"), f"error feedback, member {i} (n={sizes[i]})")
    outs = [T.carve(n, T.FDT[dt]) for n in sizes]
    pt.dequantize_grouped_rotated_batch([torch.from_numpy(np.asarray(g[0], dtype=np.uint8)).cuda() for g in got], [torch.from_numpy(g[1]).cuda() for g in got],
                                        [torch.from_numpy(g[2]).cuda() for g in got], dtype=T.FDT[dt], group_size=G, seed=SEED, outs=[o[1] for o in outs],
                                        quant_dtype=T.QDT[qd], shapes=[(n,) for n in sizes])
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        T.canaries_intact(outs[i][0], outs[i][2], n * outs[i][1].element_size(), f"out of member {i}")
        T.same(T.host(outs[i][1]), R.dequantize_grouped_rotated(got[i][0], qd, dt, n, G, got[i][1], got[i][2], SEED), f"dequantize, member {i} (n={n})")


# ---- 4. a batch is its members, not their concatenation

@pytest.mark.parametrize("pair", WIDTH_PAIRS, ids=WIDTH_IDS)
@pytest.mark.parametrize("G", GROUPS_GRID)
def test_a_batch_is_its_members(ctx, pair, G):
    dt, qd = pair
    restore(ctx)
    n = 2 * G + G // 2
    hosts = [member_data(i, n, dt, G) for i in range(2)]
    got = quantize_batch([T.dev(h, dt) for h in hosts], [n, n], qd, G, "nearest")
    for i in range(2):
        T.triple_same(got[i], model_quantize(i, n, dt, qd, G, "nearest"), f"two members of 2 G + G / 2: member {i}")
    # spelled out: the last half group of EACH member has the parameters of its plain, un-rotated values, member 1's first group those of a
    # rotated group -- the concatenation would rotate member 0's half group together with the first half of member 1's first group
    for i in range(2):
        tail = R.GM.quantize_grouped(R.widen(hosts[i], dt)[2 * G:], O.F32, qd, G)
        assert got[i][1][2] == np.asarray(tail[1])[0] and got[i][2][2] == np.asarray(tail[2])[0], f"member {i}: its ragged group is not rotated"
    head = R.quantize_grouped_rotated(hosts[1][:G], dt, qd, G, SEED)
    assert got[1][1][0] == np.asarray(head[1])[0], "member 1's first group is rotated"
    both = R.quantize_grouped_rotated(np.concatenate(hosts), dt, qd, G, SEED)
    assert np.asarray(both[1])[2] != got[0][1][2], "the concatenation's third group is another group"
    # a member shorter than G between two long ones
    sizes = [4 * G + 3, G - 1, 3 * G]
    hosts = [member_data(i, m, dt, G) for i, m in enumerate(sizes)]
    got = quantize_batch([T.dev(h, dt) for h in hosts], sizes, qd, G, "nearest")
    for i, m in enumerate(sizes):
        T.triple_same(got[i], model_quantize(i, m, dt, qd, G, "nearest"), f"a short member between two long ones: member {i}")
    # empty members first, last and in the middle
    sizes = [0, 2 * G + 1, 0, 1025, 0]
    hosts = [member_data(i, m, dt, G) for i, m in enumerate(sizes)]
    xs = [T.dev(h, dt) for h in hosts]
    got = quantize_batch(xs, sizes, qd, G, "nearest")
    rs = [residual_of(i, m, G) for i, m in enumerate(sizes)]
    quads = ef_batch(xs, rs, sizes, qd, G, "nearest")
    for i, m in enumerate(sizes):
        T.triple_same(got[i], model_quantize(i, m, dt, qd, G, "nearest"), f"empty members around: member {i}")
        quad_same(quads[i], model_ef(i, m, dt, qd, G, "nearest"), f"empty members around, error feedback: member {i}")


def test_a_batch_of_only_empty_members_writes_nothing(ctx):
    """three empty members: nothing is launched, and every canary around the (empty) buffers is intact"""
    import piquant.torch as pt

    G, qd = 128, O.UINT4
    restore(ctx)
    empty = [torch.empty(0, device="cuda") for _ in range(3)]
    triples = quantize_batch(empty, [0, 0, 0], qd, G, "stochastic")
    assert all(t[0].size == 0 and t[1].size == 0 and t[2].size == 0 for t in triples)
    quads = ef_batch(empty, [np.zeros(0, dtype=np.float32)] * 3, [0, 0, 0], qd, G, "stochastic")
    assert all(q[0].size == 0 and q[3].size == 0 for q in quads)
    outs = [T.carve(0, torch.float32) for _ in range(3)]
    pt.dequantize_grouped_rotated_batch([torch.empty(0, dtype=torch.uint8, device="cuda")] * 3, [torch.empty(0, device="cuda")] * 3,
                                        [torch.empty(0, dtype=torch.uint8, device="cuda")] * 3, dtype=torch.float32, group_size=G, seed=SEED,
                                        outs=[o[1] for o in outs], quant_dtype=T.QDT[qd], shapes=[(0,)] * 3)
    torch.cuda.synchronize()
    for buf, _, first in outs:
        T.canaries_intact(buf, first, 0, "an empty out")


# ---- 5. hipGraph capture and replay

def test_graph_capture_and_replay(ctx):
    import piquant.torch as pt

    G, qd, dt = 128, O.UINT4, O.BF16
    sizes = [40037, 3 * G + 5, 1025]
    restore(ctx)
    inputs = [[T.dev(T.data(n, dt, G, seed=90 + 10 * k + i), dt) for i, n in enumerate(sizes)] for k in range(2)]
    xs = [t.clone() for t in inputs[0]]
    rs = [torch.zeros(n, device="cuda") for n in sizes]
    accs = [torch.zeros(n, device="cuda") for n in sizes]

    def calls(src, residuals, accumulate):
        q, s, z = pt.quantize_grouped_rotated_batch(src, dtype=T.QDT[qd], group_size=G, seed=SEED)
        back = pt.dequantize_grouped_rotated_batch(q, s, z, dtype=torch.bfloat16, group_size=G, seed=SEED)
        pt.dequantize_grouped_rotated_batch(q, s, z, dtype=torch.float32, group_size=G, seed=SEED, reduce_op="add", outs=accumulate)
        qe, se, ze = pt.quantize_grouped_rotated_ef_batch(src, residuals, dtype=T.QDT[qd], group_size=G, seed=SEED)
        return q, s, z, back, qe, se, ze

    calls(xs, [torch.zeros_like(r) for r in rs], [torch.zeros_like(a) for a in accs])   # warm-up outside capture (code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = calls(xs, rs, accs)
    want_r = [torch.zeros_like(r) for r in rs]
    want_acc = [torch.zeros_like(a) for a in accs]
    names = ("packed", "scales", "zero points", "round trip", "EF packed", "EF scales", "EF zero points")
    for fresh in inputs:   # the second replay follows the changed inputs
        for x, f in zip(xs, fresh):
            x.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = calls(fresh, want_r, want_acc)
        torch.cuda.synchronize()
        for got_list, want_list, name in zip(captured, eager, names):
            for i, (got, want) in enumerate(zip(got_list, want_list)):
                g = pt.packed_bytes(got) if got.dtype in T.QDT.values() and got.dtype != torch.uint8 else got
                w = pt.packed_bytes(want) if want.dtype in T.QDT.values() and want.dtype != torch.uint8 else want
                T.same(T.host(g), T.host(w), f"captured {name} of member {i}")
        for i in range(len(sizes)):
            T.same(T.host(accs[i]), T.host(want_acc[i]), f"captured ADD of member {i}")
            T.same(T.host(rs[i]), T.host(want_r[i]), f"captured residual of member {i}")
    assert not np.array_equal(T.host(inputs[0][0]), T.host(inputs[1][0]))


# ---- 6. piquant.distributed._DeviceOps on the batched launches

class Spy:
    """a context that records the name of every *_ptr call made through it"""

    def __init__(self, inner):
        self._inner, self.calls = inner, []

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not name.endswith("_ptr"):
            return attr

        def recorded(*args, **kwargs):
            self.calls.append(name)
            return attr(*args, **kwargs)

        return recorded


@pytest.mark.parametrize("numel", (8195, 5))
@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
def test_device_ops_make_one_batched_call(ctx, dt, numel):
    """a three-chunk mesh layout (4096, 4096, 3) and one with empty chunks (5, 0, 0): each of the three _DeviceOps batch methods makes exactly one
    *_batch_ptr call and no single *_rotated_ptr call, and leaves the wire bytes, tensor bytes and residual bytes of the loop of single methods"""
    import piquant.distributed as D

    G, qd, qdtype = 128, O.UINT4, torch.quint4x2
    restore(ctx)
    chunks = D.ring_chunks(numel, 3, 4)
    assert [e - b for b, e in chunks] == ([4096, 4096, 3] if numel == 8195 else [5, 0, 0])
    x = T.dev(T.data(numel, dt, G, seed=95), dt)
    xs = [x[b:e] for b, e in chunks]
    spy = Spy(ctx)
    batched, looped = D._DeviceOps(spy), D._DeviceOps(ctx)

    def wires():
        return [torch.full((D.grouped_wire_layout(e - b, G, 4).nbytes + 32,), T.CANARY, dtype=torch.uint8, device="cuda") for b, e in chunks]

    def wire_same(got, want, what):
        for i, (g, w) in enumerate(zip(got, want)):
            nbytes = D.grouped_wire_layout(chunks[i][1] - chunks[i][0], G, 4).nbytes
            assert bool((g[nbytes:] == T.CANARY).all()), f"{what}: wrote past record {i}"
            lay = D.grouped_wire_layout(chunks[i][1] - chunks[i][0], G, 4)
            pad = slice(lay.zero_points_offset + lay.ngroups, lay.data_offset)   # the padding in front of the packed bytes is nobody's
            gc, wc = g[:nbytes].clone(), w[:nbytes].clone()
            gc[pad], wc[pad] = 0, 0
            assert torch.equal(gc, wc), f"{what}: record {i} differs"

    # encode
    got, want = wires(), wires()
    batched.encode_batch_grouped_rotated(xs, got, qdtype, "nearest", G, SEED)
    for xc, w in zip(xs, want):
        looped.encode_grouped_rotated(xc, w, qdtype, "nearest", G, SEED)
    torch.cuda.synchronize()
    assert spy.calls == ["quantize_grouped_rotated_batch_ptr"], spy.calls
    wire_same(got, want, "encode_batch_grouped_rotated")
    # encode with error feedback
    spy.calls.clear()
    r0 = (np.array(T.data(numel, O.F32, G, seed=96)) * np.float32(0.01)).astype(np.float32)
    rb, r_batched, r_first = put(r0, torch.float32)
    r_looped = torch.from_numpy(r0.copy()).cuda()
    got_ef, want_ef = wires(), wires()
    batched.encode_batch_grouped_rotated_ef(xs, [r_batched[b:e] for b, e in chunks], got_ef, qdtype, "nearest", G, SEED)
    for (b, e), xc, w in zip(chunks, xs, want_ef):
        looped.encode_grouped_rotated_ef(xc, r_looped[b:e], w, qdtype, "nearest", G, SEED)
    torch.cuda.synchronize()
    assert spy.calls == ["quantize_grouped_rotated_ef_batch_ptr"], spy.calls
    wire_same(got_ef, want_ef, "encode_batch_grouped_rotated_ef")
    T.same(T.host(r_batched), T.host(r_looped), "the residual")
    T.canaries_intact(rb, r_first, numel * 4, "the residual")
    # decode
    spy.calls.clear()
    ob, out_batched, o_first = T.carve(numel, T.FDT[dt])
    out_looped = torch.zeros(numel, dtype=T.FDT[dt], device="cuda")
    batched.decode_batch_grouped_rotated(want, [out_batched[b:e] for b, e in chunks], qdtype, "set", G, SEED)
    for (b, e), w in zip(chunks, want):
        looped.decode_grouped_rotated(w, out_looped[b:e], qdtype, "set", G, SEED)
    torch.cuda.synchronize()
    assert spy.calls == ["dequantize_grouped_rotated_batch_ptr"], spy.calls
    T.same(T.host(out_batched), T.host(out_looped), "decode_batch_grouped_rotated")
    T.canaries_intact(ob, o_first, numel * out_batched.element_size(), "the decoded tensor")
    T.same(T.host(x), T.data(numel, dt, G, seed=95), "the tensor is only read")
