"""GPU: the optional buffers of the device-parameter and group-wise piquant.torch wrappers.  Every wrapper is called twice on the same seeded
input -- once with all defaults, once with every optional buffer supplied (out / outs, the parameter arrays or records, a raw uint8 input with
quant_dtype= and shape= / shapes=, return_params=True) -- and the two calls must leave the same bytes in outputs, parameters and residuals,
with the supplied buffers being the objects that come back.  Nearest rounding; group_size 32 on 4 * 32 + 5 elements (a partial last group)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

G = 32
SHAPE = (7, 19)          # 133 = 4 * G + 5 elements
N = SHAPE[0] * SHAPE[1]
CASES = [(torch.float32, torch.quint8), (torch.bfloat16, torch.quint4x2), (torch.bfloat16, torch.quint2x4)]
BATCHES = [(torch.float32, torch.quint8, 3), (torch.bfloat16, torch.quint4x2, 3), (torch.bfloat16, torch.quint2x4, 17)]   # 17: two launches of up to 16
TERMS = [(torch.float32, torch.quint8, 3), (torch.bfloat16, torch.quint4x2, 3), (torch.bfloat16, torch.quint2x4, 0)]
_QUANTIZED = (torch.quint8, torch.quint4x2, torch.quint2x4)


@pytest.fixture(scope="module")
def pt():
    import piquant.torch

    torch.cuda.set_device(0)
    return piquant.torch


def data(seed, fdt, contiguous=False):
    """Seeded values of SHAPE on the device: every other column of a wider tensor (a non-contiguous view) unless ``contiguous``."""
    wide = (torch.randn(SHAPE[0], 2 * SHAPE[1], generator=torch.Generator().manual_seed(seed)) * 3.0).to(fdt).cuda()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    return view.contiguous() if contiguous else view


def raw(pt, t):
    """The bytes a tensor holds, on the host."""
    if t.dtype in _QUANTIZED:
        return pt.packed_bytes(t).cpu()
    return t.contiguous().view(-1).view(torch.uint8).cpu()


def same(pt, a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(pt, x, y) for x, y in zip(a, b))
    return torch.equal(raw(pt, a), raw(pt, b))


def are(returned, supplied):
    if isinstance(supplied, (list, tuple)):
        return len(returned) == len(supplied) and all(r is s for r, s in zip(returned, supplied))
    return returned is supplied


def nbytes(pt, qdt, numel=N):
    return pt.torch_to_piquant_dtype(qdt).packed_nbytes(numel)


def packed_buf(pt, qdt):
    return torch.empty(nbytes(pt, qdt), dtype=torch.uint8, device="cuda")


def group_bufs(numel=N):
    ng = (numel + G - 1) // G
    return torch.empty(ng, dtype=torch.float32, device="cuda"), torch.empty(ng, dtype=torch.uint8, device="cuda")


def record():
    return torch.empty(16, dtype=torch.uint8, device="cuda")


def bytes_of(pt, q):
    """A raw uint8 buffer of its own with the packed bytes of a quantized tensor."""
    return pt.packed_bytes(q).clone()


def residual_dtypes(fdt):
    return [fdt] if fdt == torch.float32 else [fdt, torch.float32]   # a bfloat16 tensor also takes a float32 residual


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_quantize_dequantize(pt, fdt, qdt):
    x = data(1, fdt)
    want = pt.quantize_dequantize(x, scale=0.05, zero_point=1, quant_dtype=qdt)
    out = torch.empty(SHAPE, dtype=fdt, device="cuda")
    got = pt.quantize_dequantize(x, scale=0.05, zero_point=1, quant_dtype=qdt, out=out)
    assert got is out and want.shape == x.shape and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_compute_quant_params_device(pt, fdt, qdt):
    x = data(2, fdt)
    want = pt.compute_quant_params_device(x, dtype=qdt)
    rec = record()
    got = pt.compute_quant_params_device(x, dtype=qdt, out=rec)
    assert got is rec and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_quantize_dynamic(pt, fdt, qdt):
    x = data(3, fdt)
    want = pt.quantize_dynamic(x, dtype=qdt)
    out, rec = packed_buf(pt, qdt), record()
    got = pt.quantize_dynamic(x, dtype=qdt, out=out, params=rec)
    assert are(got, (out, rec)) and want[0].shape == x.shape and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_dequantize_dynamic(pt, fdt, qdt):
    q, rec = pt.quantize_dynamic(data(4, fdt), dtype=qdt)
    want = pt.dequantize_dynamic(q, rec, dtype=fdt)
    out = torch.empty(SHAPE, dtype=fdt, device="cuda")
    got = pt.dequantize_dynamic(bytes_of(pt, q), rec, dtype=fdt, out=out, quant_dtype=qdt, shape=SHAPE)
    assert got is out and want.shape == SHAPE and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_quantize_grouped(pt, fdt, qdt):
    x = data(5, fdt)
    want = pt.quantize_grouped(x, dtype=qdt, group_size=G)
    out, sc, zp = packed_buf(pt, qdt), want[1].clone(), want[2].clone()    # scales= / zero_points= are the given parameters of this call
    got = pt.quantize_grouped(x, dtype=qdt, group_size=G, out=out, scales=sc, zero_points=zp)
    assert are(got, (out, sc, zp)) and want[0].shape == x.shape and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_dequantize_grouped(pt, fdt, qdt):
    q, sc, zp = pt.quantize_grouped(data(6, fdt), dtype=qdt, group_size=G)
    want = pt.dequantize_grouped(q, sc, zp, dtype=fdt, group_size=G)
    out = torch.empty(SHAPE, dtype=fdt, device="cuda")
    got = pt.dequantize_grouped(bytes_of(pt, q), sc, zp, dtype=fdt, group_size=G, out=out, quant_dtype=qdt, shape=SHAPE)
    assert got is out and want.shape == SHAPE and same(pt, got, want)


def grouped_terms(pt, fdt, qdt, count, seed):
    terms = [pt.quantize_grouped(data(seed + i, fdt), dtype=qdt, group_size=G) for i in range(count)]
    return [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms]


@pytest.mark.parametrize("fdt,qdt,count", TERMS)
def test_reduce_quantize_grouped(pt, fdt, qdt, count):
    acc = data(7, fdt, contiguous=True)
    qs, scs, zps = grouped_terms(pt, fdt, qdt, count, 70)
    want = pt.reduce_quantize_grouped(acc.clone(), qs, scs, zps, dtype=qdt, group_size=G)
    out, (sc, zp) = packed_buf(pt, qdt), group_bufs()
    got = pt.reduce_quantize_grouped(acc.clone(), [bytes_of(pt, q) for q in qs], scs, zps, dtype=qdt, group_size=G, out=out, out_scales=sc,
                                     out_zero_points=zp)
    assert are(got, (out, sc, zp)) and want[0].shape == SHAPE and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt,count", BATCHES)
def test_quantize_grouped_batch(pt, fdt, qdt, count):
    xs = [data(80 + i, fdt) for i in range(count)]
    want = pt.quantize_grouped_batch(xs, dtype=qdt, group_size=G)
    outs = [torch.empty(SHAPE, dtype=qdt, device="cuda") for _ in xs]
    scs, zps = [s.clone() for s in want[1]], [z.clone() for z in want[2]]   # the given parameters of this call
    got = pt.quantize_grouped_batch(xs, dtype=qdt, group_size=G, outs=outs, scales=scs, zero_points=zps)
    assert all(are(g, s) for g, s in zip(got, (outs, scs, zps))) and all(same(pt, g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_quantize_dequantize_grouped(pt, fdt, qdt):
    x = data(9, fdt)
    want = pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G)
    _, wsc, wzp = pt.quantize_grouped(x, dtype=qdt, group_size=G)
    out, (sc, zp) = torch.empty(SHAPE, dtype=fdt, device="cuda"), group_bufs()
    got = pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G, return_params=True, out=out)   # computed parameters, handed back
    assert got[0] is out and want.shape == x.shape and same(pt, got, (want, wsc, wzp))
    sc.copy_(wsc)
    zp.copy_(wzp)
    got = pt.quantize_dequantize_grouped(x, quant_dtype=qdt, group_size=G, scales=sc, zero_points=zp, return_params=True, out=out)
    assert are(got, (out, sc, zp)) and same(pt, got, (want, wsc, wzp))


@pytest.mark.parametrize("fdt,qdt,count", BATCHES)
def test_quantize_dequantize_grouped_batch(pt, fdt, qdt, count):
    xs = [data(100 + i, fdt) for i in range(count)]
    want = pt.quantize_dequantize_grouped_batch(xs, quant_dtype=qdt, group_size=G)
    _, wscs, wzps = pt.quantize_grouped_batch(xs, dtype=qdt, group_size=G)
    outs = [torch.empty(SHAPE, dtype=fdt, device="cuda") for _ in xs]
    got = pt.quantize_dequantize_grouped_batch(xs, quant_dtype=qdt, group_size=G, return_params=True, outs=outs)
    assert are(got[0], outs) and all(same(pt, g, w) for g, w in zip(got, (want, wscs, wzps)))
    scs, zps = [s.clone() for s in wscs], [z.clone() for z in wzps]
    got = pt.quantize_dequantize_grouped_batch(xs, quant_dtype=qdt, group_size=G, scales=scs, zero_points=zps, return_params=True, outs=outs)
    assert all(are(g, s) for g, s in zip(got, (outs, scs, zps))) and all(same(pt, g, w) for g, w in zip(got, (want, wscs, wzps)))


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_quantize_grouped_ef(pt, fdt, qdt):
    x = data(11, fdt)
    for rdt in residual_dtypes(fdt):
        r0 = (data(12, torch.float32, contiguous=True) * 0.01).to(rdt)
        r_want, r_got = r0.clone(), r0.clone()
        want = pt.quantize_grouped_ef(x, r_want, dtype=qdt, group_size=G)
        out, (sc, zp) = packed_buf(pt, qdt), group_bufs()
        got = pt.quantize_grouped_ef(x, r_got, dtype=qdt, group_size=G, out=out, out_scales=sc, out_zero_points=zp)
        assert are(got, (out, sc, zp)) and want[0].shape == x.shape and same(pt, got, want)
        assert same(pt, r_got, r_want) and not same(pt, r_got, r0)


@pytest.mark.parametrize("fdt,qdt,count", TERMS)
def test_reduce_quantize_grouped_ef(pt, fdt, qdt, count):
    acc = data(13, fdt, contiguous=True)
    qs, scs, zps = grouped_terms(pt, fdt, qdt, count, 130)
    for rdt in residual_dtypes(fdt):
        r0 = (data(14, torch.float32, contiguous=True) * 0.01).to(rdt)
        r_want, r_got = r0.clone(), r0.clone()
        want = pt.reduce_quantize_grouped_ef(acc.clone(), r_want, qs, scs, zps, dtype=qdt, group_size=G)
        out, (sc, zp) = packed_buf(pt, qdt), group_bufs()
        got = pt.reduce_quantize_grouped_ef(acc.clone(), r_got, [bytes_of(pt, q) for q in qs], scs, zps, dtype=qdt, group_size=G, out=out,
                                            out_scales=sc, out_zero_points=zp)
        assert are(got, (out, sc, zp)) and want[0].shape == SHAPE and same(pt, got, want)
        assert same(pt, r_got, r_want) and not same(pt, r_got, r0)


@pytest.mark.parametrize("fdt,qdt,count", BATCHES)
def test_quantize_grouped_ef_batch(pt, fdt, qdt, count):
    xs = [data(150 + i, fdt) for i in range(count)]
    for rdt in residual_dtypes(fdt):
        r0 = [(data(200 + i, torch.float32, contiguous=True) * 0.01).to(rdt) for i in range(count)]
        r_want, r_got = [r.clone() for r in r0], [r.clone() for r in r0]
        want = pt.quantize_grouped_ef_batch(xs, r_want, dtype=qdt, group_size=G)
        outs = [torch.empty(SHAPE, dtype=qdt, device="cuda") for _ in xs]
        scs, zps = zip(*[group_bufs() for _ in xs])
        got = pt.quantize_grouped_ef_batch(xs, r_got, dtype=qdt, group_size=G, outs=outs, out_scales=scs, out_zero_points=zps)
        assert all(are(g, s) for g, s in zip(got, (outs, scs, zps))) and all(same(pt, g, w) for g, w in zip(got, want))
        assert same(pt, r_got, r_want) and not same(pt, r_got, r0)


@pytest.mark.parametrize("fdt,qdt,count", BATCHES)
def test_dequantize_grouped_batch(pt, fdt, qdt, count):
    qs, scs, zps = grouped_terms(pt, fdt, qdt, count, 160)
    want = pt.dequantize_grouped_batch(qs, scs, zps, dtype=fdt, group_size=G)
    outs = [torch.empty(SHAPE, dtype=fdt, device="cuda") for _ in qs]
    got = pt.dequantize_grouped_batch([bytes_of(pt, q) for q in qs], scs, zps, dtype=fdt, group_size=G, outs=outs, quant_dtype=qdt,
                                      shapes=[SHAPE] * count)
    assert are(got, outs) and all(w.shape == SHAPE for w in want) and same(pt, got, want)


def dynamic_terms(pt, fdt, qdt, count, seed):
    terms = [pt.quantize_dynamic(data(seed + i, fdt), dtype=qdt) for i in range(count)]
    return [t[0] for t in terms], [t[1] for t in terms]


@pytest.mark.parametrize("fdt,qdt", CASES)
def test_dequantize_sum(pt, fdt, qdt):
    qs, recs = dynamic_terms(pt, fdt, qdt, 3, 170)
    want = pt.dequantize_sum(qs, recs, dtype=fdt)
    out = torch.empty(SHAPE, dtype=fdt, device="cuda")
    got = pt.dequantize_sum([bytes_of(pt, q) for q in qs], recs, dtype=fdt, out=out, quant_dtype=qdt, shape=SHAPE)
    assert got is out and want.shape == SHAPE and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt,count", BATCHES)
def test_quantize_dynamic_batch(pt, fdt, qdt, count):
    xs = [data(180 + i, fdt) for i in range(count)]
    want = pt.quantize_dynamic_batch(xs, dtype=qdt)
    outs, recs = [torch.empty(SHAPE, dtype=qdt, device="cuda") for _ in xs], [record() for _ in xs]
    got = pt.quantize_dynamic_batch(xs, dtype=qdt, outs=outs, params=recs)
    assert all(are(g, s) for g, s in zip(got, (outs, recs))) and all(same(pt, g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("fdt,qdt,count", BATCHES)
def test_dequantize_dynamic_batch(pt, fdt, qdt, count):
    qs, recs = dynamic_terms(pt, fdt, qdt, count, 190)
    want = pt.dequantize_dynamic_batch(qs, recs, dtype=fdt)
    outs = [torch.empty(SHAPE, dtype=fdt, device="cuda") for _ in qs]
    got = pt.dequantize_dynamic_batch([bytes_of(pt, q) for q in qs], recs, dtype=fdt, outs=outs, quant_dtype=qdt, shapes=[SHAPE] * count)
    assert are(got, outs) and all(w.shape == SHAPE for w in want) and same(pt, got, want)


@pytest.mark.parametrize("fdt,qdt,count", TERMS)
def test_reduce_quantize_dynamic(pt, fdt, qdt, count):
    acc = data(21, fdt, contiguous=True)
    qs, recs = dynamic_terms(pt, fdt, qdt, count, 210)
    want = pt.reduce_quantize_dynamic(acc.clone(), qs, recs, dtype=qdt)
    out, rec = packed_buf(pt, qdt), record()
    got = pt.reduce_quantize_dynamic(acc.clone(), [bytes_of(pt, q) for q in qs], recs, dtype=qdt, out=out, out_params=rec)
    assert are(got, (out, rec)) and want[0].shape == SHAPE and same(pt, got, want)
