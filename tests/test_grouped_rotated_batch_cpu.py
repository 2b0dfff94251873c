"""The batched rotated grouped calls without a GPU: what piquant.torch.quantize_grouped_rotated_batch / dequantize_grouped_rotated_batch /
quantize_grouped_rotated_ef_batch refuse (ValueError, before anything is launched: host tensors throughout, nothing here touches a device), the
length asserts of the three Context.*_batch_ptr methods, and the three symbols of the C ABI."""
import re
import subprocess
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
SEED = 0x9E37_79B9_7F4A_7C15
SYMBOLS = {"piquant_hip_quantize_grouped_rotated_batch": 12, "piquant_hip_dequantize_grouped_rotated_batch": 12,
           "piquant_hip_quantize_grouped_rotated_ef_batch": 13}


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    import piquant
    import piquant.torch as pt
    from piquant._bootstrap import C_LIB, library_path

    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for symbol, nargs in SYMBOLS.items():
        assert re.search(r"PIQUANT_EXPORT\s+void\s+" + symbol + r"\s*\(", header), f"{symbol} is not declared in piquant_hip.h"
        assert len(getattr(C_LIB, symbol).argtypes) == nargs
        assert symbol in exported, f"libpiquant.so does not export {symbol}"
    for name in ("quantize_grouped_rotated_batch", "dequantize_grouped_rotated_batch", "quantize_grouped_rotated_ef_batch"):
        assert callable(getattr(pt, name)) and callable(getattr(piquant.Context, name + "_ptr"))


def quantize_calls():
    """(name, call) of the two quantizing batches on the same tensors; the error-feedback one gets matching float32 residuals unless told otherwise"""
    import piquant.torch as pt

    def plain(tensors, residuals=None, **kw):
        return pt.quantize_grouped_rotated_batch(tensors, dtype=kw.pop("dtype", torch.quint4x2), **kw)

    def ef(tensors, residuals=None, **kw):
        residuals = [torch.zeros(t.numel()) for t in tensors] if residuals is None else residuals
        return pt.quantize_grouped_rotated_ef_batch(tensors, residuals, dtype=kw.pop("dtype", torch.quint4x2), **kw)

    return [("quantize_grouped_rotated_batch", plain), ("quantize_grouped_rotated_ef_batch", ef)]


def test_the_quantizing_batches_refuse_bad_arguments():
    xs = [torch.zeros(1000), torch.zeros(300)]
    s, z = [torch.zeros(8), torch.zeros(3)], [torch.zeros(8, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8)]
    outs = [torch.zeros(500, dtype=torch.uint8), torch.zeros(150, dtype=torch.uint8)]
    for name, call in quantize_calls():
        with pytest.raises(ValueError, match="batch is empty"):
            call([], seed=SEED)
        with pytest.raises(ValueError, match="same length"):
            call(xs, seed=SEED, outs=outs[:1])
        with pytest.raises(ValueError, match="same length"):
            call(xs, seed=SEED, out_scales=s[:1], out_zero_points=z)
        with pytest.raises(ValueError, match="seed"):
            call(xs)
        for bad in (1.5, "7", None, True):
            with pytest.raises(ValueError, match="seed"):
                call(xs, seed=bad)
        for bad in (100, 16, 8192, None, 128.0, True):
            with pytest.raises(ValueError, match="group_size"):
                call(xs, seed=SEED, group_size=bad)
        with pytest.raises(ValueError, match="quantized dtype"):
            call(xs, seed=SEED, dtype=torch.float32)
        with pytest.raises(ValueError, match="round_mode"):
            call(xs, seed=SEED, round_mode="up")
        with pytest.raises(ValueError, match="both out_scales and out_zero_points"):
            call(xs, seed=SEED, out_scales=s)
        with pytest.raises(ValueError, match="both out_scales and out_zero_points"):
            call(xs, seed=SEED, out_zero_points=z)
        with pytest.raises(ValueError):   # mixed dtypes
            call([xs[0], xs[1].bfloat16()], seed=SEED)
        with pytest.raises(ValueError):   # mixed devices
            call([xs[0], torch.zeros(300, device="meta")], seed=SEED)
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            call([xs[0], torch.zeros(300, dtype=torch.float16)], seed=SEED)
        with pytest.raises(ValueError, match="ROCm"):   # everything matches, but host tensors
            call(xs, seed=SEED)


def test_the_error_feedback_batch_refuses_bad_residuals():
    import piquant.torch as pt

    xs = [torch.zeros(1000), torch.zeros(300)]
    good = [torch.zeros(1000), torch.zeros(300)]
    kw = dict(dtype=torch.quint4x2, seed=SEED)
    with pytest.raises(ValueError, match="same length"):
        pt.quantize_grouped_rotated_ef_batch(xs, good[:1], **kw)
    with pytest.raises(ValueError, match=r"residuals\[1\] must be torch.float32"):
        pt.quantize_grouped_rotated_ef_batch(xs, [good[0], torch.zeros(300, dtype=torch.bfloat16)], **kw)
    with pytest.raises(ValueError, match=r"residuals\[0\] must be torch.float32"):   # float32 also for bfloat16 tensors
        pt.quantize_grouped_rotated_ef_batch([x.bfloat16() for x in xs], [torch.zeros(1000, dtype=torch.bfloat16), good[1]], **kw)
    with pytest.raises(ValueError, match=r"residuals\[1\] must be contiguous"):
        pt.quantize_grouped_rotated_ef_batch(xs, [good[0], torch.zeros(600)[::2]], **kw)
    with pytest.raises(ValueError, match=r"residuals\[1\] must have the numel"):
        pt.quantize_grouped_rotated_ef_batch(xs, [good[0], torch.zeros(299)], **kw)
    with pytest.raises(ValueError, match=r"residuals\[0\] must be a torch.Tensor"):
        pt.quantize_grouped_rotated_ef_batch(xs, [None, good[1]], **kw)
    with pytest.raises(ValueError, match=r"residuals\[1\] must live on"):
        pt.quantize_grouped_rotated_ef_batch(xs, [good[0], torch.zeros(300, device="meta")], **kw)


def test_the_dequantizing_batch_refuses_bad_arguments():
    import piquant.torch as pt

    qs = [torch.zeros(1000, dtype=torch.uint8), torch.zeros(300, dtype=torch.uint8)]
    s, z = [torch.zeros(8), torch.zeros(3)], [torch.zeros(8, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8)]
    kw = dict(dtype=torch.float32, group_size=128, seed=SEED)
    with pytest.raises(ValueError, match="batch is empty"):
        pt.dequantize_grouped_rotated_batch([], [], [], **kw)
    with pytest.raises(ValueError, match="same length"):
        pt.dequantize_grouped_rotated_batch(qs, s[:1], z, **kw)
    with pytest.raises(ValueError, match="same length"):
        pt.dequantize_grouped_rotated_batch(qs, s, z, outs=[torch.zeros(1000)], **kw)
    with pytest.raises(ValueError, match="same length"):
        pt.dequantize_grouped_rotated_batch(qs, s, z, quant_dtype=torch.uint8, shapes=[(1000,)], **kw)
    with pytest.raises(ValueError, match="seed"):
        pt.dequantize_grouped_rotated_batch(qs, s, z, dtype=torch.float32, group_size=128)
    for bad in (1.5, "7", None, True):
        with pytest.raises(ValueError, match="seed"):
            pt.dequantize_grouped_rotated_batch(qs, s, z, dtype=torch.float32, group_size=128, seed=bad)
    for bad in (100, 16, 8192, None, 128.0, True):
        with pytest.raises(ValueError, match="group_size"):
            pt.dequantize_grouped_rotated_batch(qs, s, z, dtype=torch.float32, group_size=bad, seed=SEED)
    with pytest.raises(ValueError, match="float dtype"):
        pt.dequantize_grouped_rotated_batch(qs, s, z, dtype=torch.uint8, group_size=128, seed=SEED)
    with pytest.raises(ValueError, match="reduce_op"):
        pt.dequantize_grouped_rotated_batch(qs, s, z, reduce_op="mul", **kw)
    with pytest.raises(ValueError, match="accumulates into outs"):
        pt.dequantize_grouped_rotated_batch(qs, s, z, reduce_op="add", **kw)
    with pytest.raises(ValueError, match="quantized tensor"):
        pt.dequantize_grouped_rotated_batch([torch.zeros(1000), qs[1]], s, z, **kw)
    with pytest.raises(ValueError):   # mixed devices
        pt.dequantize_grouped_rotated_batch([qs[0], torch.zeros(300, dtype=torch.uint8, device="meta")], s, z, **kw)
    with pytest.raises(ValueError, match="ROCm"):   # everything matches, but host tensors
        pt.dequantize_grouped_rotated_batch(qs, s, z, **kw)


def test_the_batch_ptr_methods_check_their_lists_before_the_call():
    """lists of different lengths are an AssertionError of the method's own, an empty batch returns -- both before the context is touched"""
    import piquant

    class Unreachable:
        def assume_device_pointers(self, flag):
            raise RuntimeError("the call was about to be made")

    C, f32, u8 = piquant.Context, piquant.DataType.F32, piquant.DataType.UINT8
    nearest, op = piquant.RoundMode.NEAREST, piquant.ReduceOp.SET
    two, one = [16, 32], [16]
    for short in range(5):   # each of the five lists in turn is one entry short
        lists = [one if i == short else two for i in range(5)]
        with pytest.raises(AssertionError):
            C.quantize_grouped_rotated_batch_ptr(Unreachable(), lists[0], f32, lists[1], u8, lists[2], 128, lists[3], lists[4], SEED, nearest)
        with pytest.raises(AssertionError):
            C.dequantize_grouped_rotated_batch_ptr(Unreachable(), lists[0], u8, lists[1], f32, lists[2], 128, lists[3], lists[4], SEED, op)
    for short in range(6):
        lists = [one if i == short else two for i in range(6)]
        with pytest.raises(AssertionError):
            C.quantize_grouped_rotated_ef_batch_ptr(Unreachable(), lists[0], f32, lists[1], lists[2], u8, lists[3], 128, lists[4], lists[5], SEED, nearest)
    with pytest.raises(AssertionError):   # the dtypes the wrong way round
        C.quantize_grouped_rotated_batch_ptr(Unreachable(), two, u8, two, f32, two, 128, two, two, SEED, nearest)
    with pytest.raises(AssertionError):
        C.dequantize_grouped_rotated_batch_ptr(Unreachable(), two, f32, two, u8, two, 128, two, two, SEED, op)
    with pytest.raises(AssertionError):
        C.quantize_grouped_rotated_ef_batch_ptr(Unreachable(), two, u8, two, two, f32, two, 128, two, two, SEED, nearest)
    assert C.quantize_grouped_rotated_batch_ptr(Unreachable(), [], f32, [], u8, [], 128, [], [], SEED, nearest) is None
    assert C.dequantize_grouped_rotated_batch_ptr(Unreachable(), [], u8, [], f32, [], 128, [], [], SEED, op) is None
    assert C.quantize_grouped_rotated_ef_batch_ptr(Unreachable(), [], f32, [], [], u8, [], 128, [], [], SEED, nearest) is None
    with pytest.raises(RuntimeError, match="about to be made"):   # a well-formed batch does reach the call
        C.quantize_grouped_rotated_batch_ptr(Unreachable(), two, f32, two, u8, two, 128, two, two, SEED, nearest)


def test_device_ops_reach_the_batch_methods_with_one_call_each():
    """_DeviceOps hands each rotated batch to ONE *_batch_ptr call (recorded, not made: no device here) and an empty list to none"""
    import piquant
    import piquant.distributed as D

    calls = []

    class Recorder:
        device = 0

        def __getattr__(self, name):
            if not name.endswith("_ptr"):
                raise AttributeError(name)
            return lambda *args, **kwargs: calls.append((name, len(args[0])))

    class Ops(D._DeviceOps):
        def _cx(self, t):
            return self.ctx

    ops = Ops(Recorder())
    xs = [torch.zeros(4096), torch.zeros(4096), torch.zeros(3)]
    bufs = [torch.zeros(D.grouped_wire_layout(x.numel(), 128, 4).nbytes, dtype=torch.uint8) for x in xs]
    ops.encode_batch_grouped_rotated(xs, bufs, torch.quint4x2, "nearest", 128, SEED)
    ops.encode_batch_grouped_rotated_ef(xs, [torch.zeros_like(x) for x in xs], bufs, torch.quint4x2, "nearest", 128, SEED)
    ops.decode_batch_grouped_rotated(bufs, xs, torch.quint4x2, "set", 128, SEED)
    assert calls == [("quantize_grouped_rotated_batch_ptr", 3), ("quantize_grouped_rotated_ef_batch_ptr", 3), ("dequantize_grouped_rotated_batch_ptr", 3)]
    calls.clear()
    ops.encode_batch_grouped_rotated([], [], torch.quint4x2, "nearest", 128, SEED)
    ops.encode_batch_grouped_rotated_ef([], [], [], torch.quint4x2, "nearest", 128, SEED)
    ops.decode_batch_grouped_rotated([], [], torch.quint4x2, "set", 128, SEED)
    assert calls == []
    assert piquant.Context.quantize_grouped_rotated_batch_ptr.__doc__ and "piquant_hip_quantize_grouped_rotated_batch" in piquant.Context.quantize_grouped_rotated_batch_ptr.__doc__
