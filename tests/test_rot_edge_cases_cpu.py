"""CPU: the edge-value cases of the rotation (tests/rot_edge_cases.py) do what they claim, on the model (tests/rot_model.py) alone.

a  the model's output has the stated classes: a -0.0 from zeros, denormals from the two denormal cases, the finite / infinite / NaN groups of overflow
b  the impulse answer does not depend on the model's butterflies: it is a column of rot_model.hadamard_matrix, by sign alone
c  each wrong rotation below -- a local function here, never project code -- changes the result of at least one named case, in both directions; the
   table of which case notices which is printed.  A kernel with one of these faults therefore fails tests/test_gpu_grouped_rotated_edges.py.
"""
import numpy as np
import pytest

import oracle as O
import per_element_model as PE
import rot_edge_cases as E
import rot_model as R

GROUP_SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
VARIANT_G = (32, 128, 1024)          # k odd, odd and even: c_G is an exact power of two only at 1024
SEED = 0x9E37_79B9_7F4A_7C15
VARIANTS = ("denormal inputs flushed", "every butterfly result flushed", "difference as -(b - a)", "stages in descending order",
            "c_G before the butterflies", "float64 accumulation rounded once", "sign-word bits read from the top",
            "sign words indexed by absolute position", "a zero-padded ragged group rotated")


def differs(a, b):
    """bit for bit, NaN positions but not NaN payloads"""
    an, bn = np.isnan(a), np.isnan(b)
    return not np.array_equal(an, bn) or not np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn])


def flushed(a):
    a = a.copy()
    m = E.is_denormal(a)
    a[m] = np.copysign(np.float32(0.0), a[m])
    return a


def wrong_rotate(x, G, seed, inverse, variant):
    """rot_model.rotate with ONE thing done wrongly"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    full = x.size // G
    c = R.scale_const(G)
    d = R.signs(G, seed)[None, :]
    if variant == "sign-word bits read from the top":
        d = np.array([[-1.0 if (w >> (15 - b)) & 1 else 1.0 for w in R.sign_words(G, seed) for b in range(16)]], dtype=np.float32)
    elif variant == "sign words indexed by absolute position":
        words = [int(O.element_threshold(seed & PE.M64, w) * 16777216.0) & 0xFFFF for w in range(full * G // 16)]
        d = np.array([-1.0 if (w >> b) & 1 else 1.0 for w in words for b in range(16)], dtype=np.float32).reshape(full, G)
    out = x.copy()
    v = x[: full * G].reshape(full, G)
    if variant == "a zero-padded ragged group rotated" and x.size % G:
        v = np.concatenate([v, np.zeros((1, G), dtype=np.float32)])
        v[-1, : x.size % G] = x[full * G:]
    ng = v.shape[0]

    def butterflies(v):
        hs = [1 << s for s in range(R.log2_of(G))]
        if variant == "stages in descending order":
            hs.reverse()
        for h in hs:
            p = v.reshape(ng, G // (2 * h), 2, h)
            a, b = p[:, :, 0, :], p[:, :, 1, :]
            diff = -(b - a) if variant == "difference as -(b - a)" else a - b
            v = np.stack([a + b, diff], axis=2).reshape(ng, G)
            if variant == "every butterfly result flushed":
                v = flushed(v)
        return v

    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if variant == "denormal inputs flushed":
            v = flushed(v)
        if variant == "float64 accumulation rounded once":
            w = v.astype(np.float64) if inverse else v.astype(np.float64) * d
            y = butterflies(w) * np.float64(c)
            y = (y * d if inverse else y).astype(np.float32)
        elif variant == "c_G before the butterflies":
            y = butterflies(v * c) * d if inverse else butterflies((v * d) * c)
        else:
            y = (butterflies(v) * c) * d if inverse else butterflies(v * d) * c
    out[:] = y.reshape(-1)[: x.size] if ng > full else np.concatenate([y.reshape(-1), x[full * G:]])
    return out


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_no_variant_is_the_model(G):
    """wrong_rotate with nothing wrong is rot_model.rotate: the variants differ from the model by their one fault alone"""
    for name, x in E.cases(G, SEED, names=E.SMALL).items():
        for inverse in (False, True):
            assert not differs(wrong_rotate(x, G, SEED, inverse, None), R.rotate(x, G, SEED, inverse)), (name, inverse)


@pytest.mark.parametrize("dt", (O.F32, O.BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("G", GROUP_SIZES)
def test_cases_have_the_stated_classes(G, dt):
    got = E.cases(G, SEED, dt, names=E.SMALL)
    for name, x in got.items():
        assert x.size == E.ngroups(name, G) * G + G - 1 and x.dtype == (np.float32 if dt == O.F32 else np.uint16)
        xf = R.widen(x, dt)
        assert np.array_equal(xf[-(G - 1):].view(np.uint32), xf[: G - 1].view(np.uint32))
        for inverse in (False, True):   # the ragged tail keeps its bits
            y = R.hadamard_grouped(x, dt, G, SEED, inverse)
            assert np.array_equal(y[-(G - 1):], x[-(G - 1):])
    d = R.signs(G, SEED)
    z = R.widen(got["zeros"], dt)[: 4 * G].reshape(4, G)
    assert not z.any() and not E.is_neg_zero(z[0]).any() and E.is_neg_zero(z[1]).all() and E.is_neg_zero(z[2]).sum() == G // 2
    assert not E.is_neg_zero(z[3] * d).any()
    yz = R.rotate(R.widen(got["zeros"], dt), G, SEED)
    assert not yz.any() and E.is_neg_zero(yz).any() and not E.is_neg_zero(yz).all()
    assert E.is_neg_zero(yz[:G]).any(), "an all-(+0) group rotates to a -0.0 somewhere"
    xd = R.widen(got["denormal_in"], dt)
    assert E.is_denormal(xd).all()
    assert E.is_denormal(R.rotate(xd, G, SEED)[: 3 * G]).any()
    xo = R.widen(got["denormal_out"], dt)
    assert not E.is_denormal(xo).any() and np.all(np.abs(xo) >= np.float32(2.0 ** -124))
    yo = R.rotate(xo, G, SEED)[: 3 * G]
    assert E.is_denormal(yo).any() and not E.is_denormal(yo).all()
    xc = R.widen(got["cancel"], dt)[: 12 * G].reshape(12, G)
    assert np.array_equal(np.abs(xc), np.repeat(np.array(E.CANCEL_VALUES, dtype=np.float32), 4)[:, None] * np.ones(G, dtype=np.float32))
    yc = R.rotate(R.widen(got["cancel"], dt), G, SEED)[: 12 * G]
    assert np.count_nonzero(yc == 0) >= 3 * (G - 1) and not E.is_neg_zero(yc).any()   # x - x is +0.0: forward, only a -0.0 input gives a -0.0
    assert E.is_neg_zero(R.rotate(R.widen(got["cancel"], dt), G, SEED, inverse=True)[: 12 * G]).any()   # inverse: d * (+0.0)
    yv = R.rotate(R.widen(got["overflow"], dt), G, SEED)[: 4 * G].reshape(4, G)
    assert np.isposinf(yv[0, 0]) and not yv[0, 1:].any() and np.all(np.isfinite(yv[1])) and yv[1, 0] > 0 and not yv[1, 1:].any()
    assert np.isnan(yv[2]).any() and np.isnan(yv[3]).any()
    if dt == O.BF16:   # the stored result keeps the classes
        yb = R.widen(R.hadamard_grouped(got["overflow"], dt, G, SEED), dt)[: 4 * G].reshape(4, G)
        assert np.isposinf(yb[0, 0]) and not yb[0, 1:].any() and np.isnan(yb[2]).any()


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_impulse_answer_is_a_column_of_the_signed_matrix(G):
    """forward: group p gives c d[p] H[:, p]; inverse: d c H[:, p] -- signs from the matrix, one multiplication by +-1, no butterfly"""
    H = R.hadamard_matrix(G)
    d, c = R.signs(G, SEED), R.scale_const(G)
    assert set(np.unique(H)) == {-1.0, 1.0}
    for dt in (O.F32, O.BF16):
        x = E.case("impulses", G, SEED, dt)
        cs = c if dt == O.F32 else O.bf16_to_f32(O.f32_to_bf16(np.array([c], dtype=np.float32)))[0]   # what the store makes of c
        fwd = (H * d[None, :]).T.astype(np.float32) * cs           # row p: d[p] H[:, p]
        inv = (H * d[:, None]).T.astype(np.float32) * cs           # row p: d H[:, p]
        for inverse, want in ((False, fwd), (True, inv)):
            y = R.widen(R.hadamard_grouped(x, dt, G, SEED, inverse), dt)
            assert np.array_equal(y[: G * G].view(np.uint32), want.reshape(-1).view(np.uint32)), (dt, inverse)
            assert np.array_equal(y[G * G:].view(np.uint32), R.widen(x, dt)[G * G:].view(np.uint32))


@pytest.mark.parametrize("G", GROUP_SIZES)
def test_impulse_blocks_are_the_groups_of_the_case(G):
    """the device test runs `impulses` a block of groups at a time: the blocks are every group once, bit for bit, each with the case's tail"""
    blocks = E.impulse_blocks(G)
    assert [p for first, count in blocks for p in range(first, first + count)] == list(range(G))
    assert all(count * G + G - 1 <= (1 << 19) + G for _, count in blocks) and (G < 2048 or len(blocks) > 1)
    for dt in (O.F32, O.BF16):
        whole = E.case("impulses", G, SEED, dt)
        for first, count in blocks:
            b = E.impulse_block(G, dt, first, count)
            assert b.dtype == whole.dtype and np.array_equal(b[: count * G], whole[first * G: (first + count) * G])
            assert np.array_equal(b[count * G:], whole[G * G:])


@pytest.mark.parametrize("G", VARIANT_G)
def test_every_wrong_rotation_is_noticed(G):
    table, missed = [], []
    xs = E.cases(G, SEED)
    right = {(name, inverse): R.rotate(x, G, SEED, inverse) for name, x in xs.items() for inverse in (False, True)}
    for variant in VARIANTS:
        for inverse in (False, True):
            noticed = [name for name, x in xs.items() if differs(wrong_rotate(x, G, SEED, inverse, variant), right[name, inverse])]
            table.append(f"G={G:5d} {'inverse' if inverse else 'forward'}  {variant:42s} noticed by: {', '.join(noticed) or 'NOTHING'}")
            if not noticed:
                missed.append((variant, inverse))
    print("\n".join(table))
    assert not missed, missed
