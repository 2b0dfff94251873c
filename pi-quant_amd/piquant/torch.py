"""``piquant.torch`` -- the reference's tensor-level API on PyTorch-ROCm tensors.

Same functions and keyword arguments as the reference module (``python/src/piquant/torch.py:40-129``):
``torch_to_piquant_dtype``, ``piquant_to_torch_dtype``, ``compute_quant_params``, ``quantize``,
``dequantize``.  Differences, all additive:

* tensors may live on a ROCm device; the output is allocated on ``tensor.device`` and the kernels are
  enqueued on the current PyTorch stream (ordinary PyTorch stream semantics, no host sync);
* CPU tensors still work: their host buffers are served where they live by the companion library ``libpiquant_cpu.so`` (the default since
  round 4, synchronous on host threads) or, without it / with ``PIQUANT_HIP_HOST_PATH=stage``, staged through the GPU over PCIe;
* ``out=`` lets ``reduce_op='add'`` accumulate into an existing tensor -- the reference allocates a fresh
  uninitialised output (``torch.py:117``), which makes ADD unusable through its tensor API;
* ``ctx=None`` resolves to the default context of the tensor's device at call time (the reference evaluates
  ``Context.get()`` once, at import).

Quantized results are real ``torch.quint8`` / ``torch.quint4x2`` / ``torch.quint2x4`` tensors of the input's shape,
exactly as in the reference; PyTorch-ROCm can allocate them on the device (``torch.empty(shape, dtype=torch.quint4x2,
device='cuda')``) even though it implements hardly any operator on them -- ``packed_bytes`` gives the raw bytes.
"""
from __future__ import annotations

from itertools import repeat
from typing import Optional, Tuple

import torch

from . import Context, DataType, ReduceOp, RoundMode

_TORCH_DTYPE_MAP: dict[torch.dtype, DataType] = {
    torch.float32: DataType.F32,
    torch.bfloat16: DataType.BF16,
    torch.quint2x4: DataType.UINT2,
    torch.quint4x2: DataType.UINT4,
    torch.quint8: DataType.UINT8,
    torch.uint8: DataType.UINT8,
}

# Native front end (csrc/torch_binding.cpp): checks, output allocation, current stream and the C ABI call in one C++ function.
# Optional -- it only removes Python/ctypes overhead (8.8 -> ~4.5 us per call on a 10^6-element tensor); without it the same C
# ABI entry points are reached through ctypes below.
try:
    from . import _piquant_torch as _native
except ImportError:
    _native = None

_QUANT_TYPES: set[torch.dtype] = {torch.quint2x4, torch.quint4x2, torch.quint8, torch.uint8}
_DEQUANT_TYPES: set[torch.dtype] = {torch.float32, torch.bfloat16}
_ROUND_MODES: dict[str, RoundMode] = {'nearest': RoundMode.NEAREST, 'stochastic': RoundMode.STOCHASTIC}
_REDUCE_OPS: dict[str, ReduceOp] = {'set': ReduceOp.SET, 'add': ReduceOp.ADD}
_ROUND_MODE_CODES: dict[str, int] = {k: v.value for k, v in _ROUND_MODES.items()}   # plain ints for the native front end
_REDUCE_OP_CODES: dict[str, int] = {k: v.value for k, v in _REDUCE_OPS.items()}


def torch_to_piquant_dtype(dtype: torch.dtype) -> DataType:
    if dtype not in _TORCH_DTYPE_MAP:
        raise ValueError(f'Unsupported quant_dtype: {dtype} (float32, bfloat16, uint8 / quint8, quint4x2 and quint2x4 have a piquant counterpart)')
    return _TORCH_DTYPE_MAP[dtype]


def piquant_to_torch_dtype(dtype: DataType) -> torch.dtype:
    """First torch dtype mapped to ``dtype`` (the intent of reference ``torch.py:46-50``)."""
    for torch_dtype, piquant_dtype in _TORCH_DTYPE_MAP.items():
        if piquant_dtype == dtype:
            return torch_dtype
    raise ValueError(f'Unsupported quantized dtype: {dtype} (no torch dtype is mapped to it)')


def packed_bytes(tensor: torch.Tensor) -> torch.Tensor:
    """1-D uint8 view of the bytes that hold a quantized tensor: ``ceil(numel * bits / 8)`` of them, lower element
    index in the lower bits (PyTorch's own packing for quint4x2 / quint2x4 and the reference's)."""
    dt = torch_to_piquant_dtype(tensor.dtype)
    raw = torch.empty(0, dtype=torch.uint8, device=tensor.device).set_(tensor.untyped_storage())
    first = tensor.storage_offset() * max(dt.bit_size, 8) // 8
    return raw[first: first + dt.packed_nbytes(tensor.numel())]


# torch.cuda.current_stream(i).cuda_stream builds a Stream object per call (~1.2 us); the raw getter is ~5x cheaper
_current_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None) or (lambda index: torch.cuda.current_stream(index).cuda_stream)


def _ctx_for(tensor: torch.Tensor, ctx: Optional[Context]) -> Context:
    """Default context of the tensor's device, with the current PyTorch stream attached for device tensors."""
    if tensor.is_cuda:
        index = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
        if ctx is None:
            ctx = Context.get(index)
        elif ctx.device != index:
            raise ValueError(f'context is bound to device {ctx.device} but the tensor lives on device {index}')
        ctx.set_stream(_current_raw_stream(index))
        ctx.set_blocking(False)   # stream-ordered, like every other PyTorch device op
    else:
        if ctx is None:
            ctx = Context.get()
        ctx.reset_stream()        # host buffers: staged on the context's own streams, complete on return
        ctx.set_blocking(True)
    return ctx


def _resolve_default_handle(index: int) -> int:
    """Called by the native front end once per (thread, device): the native handle of the thread's default context of that device.  The front end
    pushes stream / non-blocking / device-pointer mode to the native context itself on every call, so the Python-side cache of pushed settings is
    switched off for this context (``Context._native_managed``): a later ctypes call pushes what it needs whatever the cache says."""
    ctx = Context._thread_defaults().get(index) or Context.get(index)
    ctx._native_managed = True
    return ctx._native_call()


if _native is not None:
    _native.set_default_resolver(_resolve_default_handle)


def _native_handle(tensor: torch.Tensor, ctx: Optional[Context]) -> int:
    """Native context handle for a call through the C++ front end (default context of the tensor's device unless one is given)."""
    if ctx is None:
        index = tensor.device.index
        ctx = Context._thread_defaults().get(index) or Context.get(index)
    return ctx._native_call()


def _quant_meta(tensor: torch.Tensor, quant_dtype: Optional[torch.dtype], shape) -> Tuple[DataType, torch.Size]:
    """Quantized dtype and logical shape of a dequantize input: from the tensor itself, or -- for a raw uint8 buffer of
    packed bytes -- from the ``quant_dtype=`` / ``shape=`` keywords."""
    if quant_dtype is not None and quant_dtype != tensor.dtype:
        _require(tensor.dtype == torch.uint8, 'quant_dtype= reinterprets a raw uint8 byte buffer')
        _require(shape is not None, 'shape= is required together with quant_dtype= for raw packed buffers')
        return torch_to_piquant_dtype(quant_dtype), torch.Size(shape)
    return torch_to_piquant_dtype(tensor.dtype), tensor.shape


# Argument checks of the additive entry points.  They raise (ValueError) rather than assert: a short, misplaced or non-contiguous
# buffer handed to a kernel by raw pointer is an out-of-bounds device write, and `python -O` strips asserts.
def _require(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _check_float_input(t: torch.Tensor, what: str = 'tensor') -> None:
    _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in _DEQUANT_TYPES, f'{what} must be a float32 or bfloat16 ROCm device tensor')


def _check_packed_out(out: torch.Tensor, dt: DataType, numel: int, device: torch.device, what: str = 'out') -> None:
    """`out` receives `numel` quantized elements: a raw uint8 buffer of at least packed_nbytes bytes, or a quantized torch tensor of numel elements."""
    _require(isinstance(out, torch.Tensor) and out.device == device and out.is_contiguous(), f'{what} must be a contiguous tensor on {device}')
    if out.dtype == torch.uint8:
        _require(out.numel() >= dt.packed_nbytes(numel), f'{what} holds {out.numel()} bytes, {dt.packed_nbytes(numel)} are needed for {numel} {dt.name} elements')
    else:
        _require(out.dtype in _QUANT_TYPES and torch_to_piquant_dtype(out.dtype) == dt and out.numel() == numel,
                 f'{what} must be a {dt.name} tensor of {numel} elements (or a uint8 buffer of the packed bytes)')


def _check_packed_in(t: torch.Tensor, dt: DataType, numel: int, device: torch.device, what: str) -> None:
    """`t` supplies `numel` quantized elements: a raw uint8 buffer of at least packed_nbytes bytes, or a quantized torch tensor of that dtype."""
    _require(isinstance(t, torch.Tensor) and t.device == device and t.is_contiguous(), f'{what} must be a contiguous tensor on {device}')
    if t.dtype == torch.uint8:
        _require(t.numel() >= dt.packed_nbytes(numel), f'{what} holds {t.numel()} bytes, {dt.packed_nbytes(numel)} are needed for {numel} {dt.name} elements')
    else:
        _require(t.dtype in _QUANT_TYPES and torch_to_piquant_dtype(t.dtype) == dt and t.numel() >= numel, f'{what} does not hold {numel} {dt.name} elements')


def _check_float_out(out: torch.Tensor, dtype: torch.dtype, numel: int, device: torch.device, what: str = 'out') -> None:
    _require(isinstance(out, torch.Tensor) and out.dtype == dtype and out.is_contiguous() and out.device == device and out.numel() == numel,
             f'{what} must be a contiguous {dtype} tensor of {numel} elements on {device}')


def _check_params(params: torch.Tensor, device: torch.device, what: str = 'params') -> None:
    _require(isinstance(params, torch.Tensor) and params.dtype == torch.uint8 and params.device == device and params.is_contiguous() and
             params.numel() >= PARAMS_NBYTES and params.data_ptr() % 8 == 0,
             f'{what} must be a contiguous uint8 tensor of at least {PARAMS_NBYTES} bytes on {device}, 8-byte aligned (the device parameter record)')


def _numel_of(shape) -> int:
    n = 1
    for s_ in shape:
        n *= int(s_)
    return n


# The blocks every additive entry point is made of.  The ORDER in which a function calls them is behaviour: it decides which fault is reported when
# an argument list has several, and everything that can be checked on host tensors is checked before the "ROCm device tensor" rule.
_NA = object()   # "this call has no such argument" (None is a value callers pass, and it is reported)


def _check_modes(*, quant_dtype=_NA, float_dtype=_NA, round_mode=_NA, reduce_op=_NA, group_size=_NA) -> None:
    """The mode arguments a call has, in the order every entry point reports them."""
    if quant_dtype is not _NA and quant_dtype not in _QUANT_TYPES:
        raise ValueError(f'{quant_dtype} is not a quantized dtype')
    if float_dtype is not _NA and float_dtype not in _DEQUANT_TYPES:
        raise ValueError(f'{float_dtype} is not a float dtype to dequantize into')
    if round_mode is not _NA and round_mode not in _ROUND_MODES:
        raise ValueError(f'round_mode must be one of {sorted(_ROUND_MODES)}, got {round_mode!r}')
    if reduce_op is not _NA and reduce_op not in _REDUCE_OPS:
        raise ValueError(f'reduce_op must be one of {sorted(_REDUCE_OPS)}, got {reduce_op!r}')
    if group_size is not _NA:
        _check_group_size(group_size)


def _packed_outs(outs, dtype: torch.dtype, like, device: torch.device, what: str = 'outs'):
    """Quantized outputs of `dtype`, one per tensor of `like` and of its shape: given, so check; otherwise allocate."""
    if outs is None:
        return [torch.empty(t.shape, dtype=dtype, device=device) for t in like]
    qdt = torch_to_piquant_dtype(dtype)
    for i, (o, t) in enumerate(zip(outs, like)):
        _check_packed_out(o, qdt, t.numel(), device, what if what == 'out' else f'{what}[{i}]')
    return outs


def _float_outs(outs, reduce_op: str, dtype: torch.dtype, shapes, numels, device: torch.device, what: str = 'outs'):
    """Float outputs of `dtype`, one per shape: given, so check; otherwise allocate -- which ``reduce_op='add'`` cannot use, it accumulates."""
    if outs is None:
        if reduce_op == 'add':
            raise ValueError(f"reduce_op='add' accumulates into {what}=; pass the accumulator tensor{'' if what == 'out' else 's'}")
        return [torch.empty(shape, dtype=dtype, device=device) for shape in shapes]
    for i, (o, n) in enumerate(zip(outs, numels)):
        _check_float_out(o, dtype, n, device, what if what == 'out' else f'{what}[{i}]')
    return outs


def _group_params(scales, zero_points, numels, group_size: int, device: torch.device, what: str = 'scales and zero_points', shapes_checked: bool = False):
    """Per-group parameters, one float32[ngroups] / uint8[ngroups] pair per tensor of `numels` elements: given, so check -- their placement alone if
    shape and dtype were checked ahead of the device rule; otherwise allocate."""
    if scales is None:
        ngroups = [num_groups(n, group_size) for n in numels]
        return [torch.empty(g, dtype=torch.float32, device=device) for g in ngroups], [torch.empty(g, dtype=torch.uint8, device=device) for g in ngroups]
    for sc, zp, n in zip(scales, zero_points, numels):
        if not shapes_checked:
            _check_group_params(sc, zp, num_groups(n, group_size))
        _require(sc.device == device and zp.device == device, f'{what} must live on {device}')
    return scales, zero_points


# The same for one tensor: lists of one, unwrapped.  (The list forms are the base: a None inside a given list is a fault of that list, not "allocate".)
def _packed_out(out, dtype: torch.dtype, like: torch.Tensor, device: torch.device) -> torch.Tensor:
    return _packed_outs(None if out is None else (out,), dtype, (like,), device, 'out')[0]


def _float_out(out, reduce_op: str, dtype: torch.dtype, shape, numel: int, device: torch.device) -> torch.Tensor:
    return _float_outs(None if out is None else (out,), reduce_op, dtype, (shape,), (numel,), device, 'out')[0]


def _group_params_of(scales, zero_points, numel: int, group_size: int, device: torch.device, what: str = 'scales and zero_points', shapes_checked: bool = False):
    sc, zp = _group_params(None if scales is None else (scales,), None if zero_points is None else (zero_points,), (numel,), group_size, device, what,
                           shapes_checked)
    return sc[0], zp[0]


def _check_grouped_terms(tensors, scales, zero_points, dtype_in: DataType, numels, group_size: int, device: torch.device) -> None:
    """Term i of a grouped reduce or batched dequantize: `numels[i]` packed elements with their own per-group parameters, all on `device`."""
    for i, (t, sc, zp, n) in enumerate(zip(tensors, scales, zero_points, numels)):
        _check_packed_in(t, dtype_in, n, device, f'tensors[{i}]')
        _check_group_params(sc, zp, num_groups(n, group_size))
        _require(sc.device == device and zp.device == device, f'scales[{i}] and zero_points[{i}] must live on {device}')


def _check_dynamic_terms(tensors, params, dtype_in: DataType, numels, device: torch.device) -> None:
    """Term i of a per-tensor reduce or batched dequantize: `numels[i]` packed elements with their device parameter record, all on `device`."""
    for i, (t, p, n) in enumerate(zip(tensors, params, numels)):
        _check_packed_in(t, dtype_in, n, device, f'tensors[{i}]')
        _check_params(p, device, f'params[{i}]')


def _contiguous(tensors):
    return [t if t.is_contiguous() else t.contiguous() for t in tensors]


def _ptrs(tensors):
    return [t.data_ptr() for t in tensors]


def compute_quant_params(tensor: torch.Tensor, *, dtype: torch.dtype, ctx: Optional[Context] = None) -> Tuple[float, int]:
    """(scale, zero_point) from the tensor's min/max (reference ``torch.py:53-67``)."""
    assert dtype in _QUANT_TYPES, f'Unsupported quantized dtype: {dtype}; choose from {[str(t) for t in _QUANT_TYPES]}'
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    ctx = _ctx_for(tensor, ctx)
    if tensor.dtype == torch.bfloat16:
        return ctx.compute_quant_params_ptr_bfloat16(tensor.data_ptr(), torch_to_piquant_dtype(dtype), tensor.numel(), _device_ptrs=tensor.is_cuda)
    assert tensor.dtype == torch.float32, f'compute_quant_params needs float32 or bfloat16, got {tensor.dtype}'
    return ctx.compute_quant_params_ptr_float32(tensor.data_ptr(), torch_to_piquant_dtype(dtype), tensor.numel(), _device_ptrs=tensor.is_cuda)


def quantize(
    tensor: torch.Tensor,
    *,
    scale: float,
    zero_point: int,
    dtype: torch.dtype,
    round_mode: str = 'nearest',
    ctx: Optional[Context] = None,
    out: Optional[torch.Tensor] = None,
    uniform: bool = False,
) -> torch.Tensor:
    """Reference ``torch.py:70-99``; the result lives on ``tensor.device``.  The bytes are those of a reference context with the
    context's ``num_threads`` (``Context.set_reference_layout``); ``uniform=True`` (additive) asks for the position-independent form
    instead -- what shards of one logical tensor must be computed with (``piquant.distributed``)."""
    if _native is not None and ctx is None and tensor.is_cuda:      # the whole call in C++: checks, default context, output, stream, the C ABI call
        return _native.quantize_default(tensor, scale, zero_point, dtype, round_mode, out, uniform)
    assert dtype in _QUANT_TYPES, f'Unsupported quantized dtype: {dtype}; choose from {[str(t) for t in _QUANT_TYPES]}'
    if _native is not None and tensor.is_cuda and tensor.dtype in _DEQUANT_TYPES:
        return _native.quantize(_native_handle(tensor, ctx), tensor, scale, zero_point, dtype, _ROUND_MODE_CODES[round_mode], out, uniform)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    dtype_in = torch_to_piquant_dtype(tensor.dtype)
    dtype_out = torch_to_piquant_dtype(dtype)
    if out is None:
        out = torch.empty(tensor.shape, dtype=dtype, device=tensor.device)   # reference torch.py:87, plus the device
    else:
        _check_packed_out(out, dtype_out, tensor.numel(), tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_ptr(
        tensor.data_ptr(),
        dtype_in,
        out.data_ptr(),
        dtype_out,
        numel=tensor.numel(),
        scale=scale,
        zero_point=zero_point,
        round_mode=_ROUND_MODES[round_mode],
        _device_ptrs=tensor.is_cuda,
        uniform=uniform,
    )
    return out


def dequantize(
    tensor: torch.Tensor,
    *,
    scale: float,
    zero_point: int,
    dtype: torch.dtype,
    reduce_op: str = 'set',
    ctx: Optional[Context] = None,
    out: Optional[torch.Tensor] = None,
    quant_dtype: Optional[torch.dtype] = None,
    shape=None,
    uniform: bool = False,
) -> torch.Tensor:
    """Reference ``torch.py:102-129``.  ``out=`` (same shape, ``dtype``) is the accumulator for ``reduce_op='add'``; ``uniform``: see ``quantize``."""
    if dtype not in _DEQUANT_TYPES:
        raise ValueError(f'Unsupported dequantized dtype: {dtype}; choose from {[str(t) for t in _DEQUANT_TYPES]}')
    if _native is not None and ctx is None and quant_dtype is None and shape is None and tensor.is_cuda and tensor.dtype in _QUANT_TYPES:
        return _native.dequantize_default(tensor, scale, zero_point, dtype, reduce_op, out, uniform)
    if _native is not None and tensor.is_cuda and quant_dtype is None and shape is None and tensor.dtype in _QUANT_TYPES:
        if out is None and reduce_op == 'add':
            raise ValueError("reduce_op='add' accumulates into out=; pass the accumulator tensor")
        return _native.dequantize(_native_handle(tensor, ctx), tensor, scale, zero_point, dtype, _REDUCE_OP_CODES[reduce_op], out, uniform)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    dtype_in, logical_shape = _quant_meta(tensor, quant_dtype, shape)
    numel = 1
    for s in logical_shape:
        numel *= int(s)
    if out is None:
        if reduce_op == 'add':
            raise ValueError("reduce_op='add' accumulates into out=; pass the accumulator tensor")
        out = torch.empty(logical_shape, dtype=dtype, device=tensor.device)
    else:
        _check_float_out(out, dtype, numel, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.dequantize_ptr(
        tensor.data_ptr(),
        dtype_in,
        out.data_ptr(),
        torch_to_piquant_dtype(out.dtype),
        numel=numel,
        scale=scale,
        zero_point=zero_point,
        reduce_op=_REDUCE_OPS[reduce_op],
        _device_ptrs=tensor.is_cuda,
        uniform=uniform,
    )
    return out


# With the native front end built, the two functions above ARE its entry points: keyword arguments are parsed in C++, a device tensor with the default
# context never enters a Python frame, and everything else comes back to the implementations above (kept under their own names for that).
_quantize_py, _dequantize_py = quantize, dequantize
if _native is not None:
    _native.set_python_implementations(_quantize_py, _dequantize_py)
    quantize, dequantize = _native.quantize_entry, _native.dequantize_entry


def quantize_dequantize(
    tensor: torch.Tensor,
    *,
    scale: float,
    zero_point: int,
    quant_dtype: torch.dtype,
    round_mode: str = 'nearest',
    reduce_op: str = 'set',
    ctx: Optional[Context] = None,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out (op)= dequantize(quantize(tensor)) in one pass over HBM -- the reference's C++-only
    ``context::quantize_dequantize_fused`` (``include/piquant.hpp:276-285``); ``out`` may be ``tensor`` (in place)."""
    _check_modes(quant_dtype=quant_dtype)
    _check_float_input(tensor)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _float_out(out, reduce_op, tensor.dtype, tensor.shape, tensor.numel(), tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_dequantize_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), torch_to_piquant_dtype(quant_dtype),
                                tensor.numel(), scale, zero_point, _ROUND_MODES[round_mode], _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return out


# -----------------------------------------------------------------------------------------------------------------
# Device-resident parameters (additive): no host round trip between the min/max scan and its consumers.
# -----------------------------------------------------------------------------------------------------------------
PARAMS_NBYTES = 16   # piquant_hip_params_t: float scale, float 1/scale, int64 zero_point


def params_to_host(params: torch.Tensor) -> Tuple[float, int]:
    """(scale, zero_point) of a device parameter record (synchronises)."""
    import struct

    scale, _inv, zp = struct.unpack('<ffq', bytes(params[:PARAMS_NBYTES].cpu().numpy().tobytes()))
    return scale, zp


def compute_quant_params_device(tensor: torch.Tensor, *, dtype: torch.dtype, ctx: Optional[Context] = None,
                                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Like ``compute_quant_params`` but asynchronous: the result is a 16-byte uint8 device tensor (the parameter record)."""
    _check_modes(quant_dtype=dtype)
    _check_float_input(tensor)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    if out is None:
        out = torch.empty(PARAMS_NBYTES, dtype=torch.uint8, device=tensor.device)
    _check_params(out, tensor.device, 'out')
    ctx = _ctx_for(tensor, ctx)
    ctx.compute_quant_params_device_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), tensor.numel(), torch_to_piquant_dtype(dtype),
                                        out.data_ptr(), _device_ptrs=True)
    return out


# ---- histogram clip search for per-tensor parameters (include/piquant_hip.h, "HISTOGRAM CLIP SEARCH") ----------------------------------------
CLIP_BINS = 8192            # PIQUANT_HIP_CLIP_BINS
CLIP_PARAMS_STEPS_MAX = 63  # candidate ranges of the per-tensor search: r_k = 1 - k / 64, k < steps


def _check_clip_params_steps(steps) -> None:
    _require(isinstance(steps, int) and not isinstance(steps, bool) and 1 <= steps <= CLIP_PARAMS_STEPS_MAX,
             f'steps must be an int in [1, {CLIP_PARAMS_STEPS_MAX}], got {steps!r}')


def _check_clip_keys(keys, device=None) -> None:
    _require(isinstance(keys, torch.Tensor) and keys.is_cuda and keys.dtype == torch.int32 and keys.dim() == 1 and keys.numel() == 2 and keys.is_contiguous(),
             'keys must be a contiguous int32[2] ROCm device tensor ({key(min), key(-max)}, local_minmax_keys)')
    _require(device is None or keys.device == device, f'keys must live on {device}')


def _check_clip_hist(hist, device: torch.device, what: str) -> None:
    _require(isinstance(hist, torch.Tensor) and hist.dtype == torch.int64 and hist.dim() == 1 and hist.numel() == CLIP_BINS and hist.is_contiguous(),
             f'{what} must be a contiguous 1-D int64 tensor of {CLIP_BINS} elements')
    _require(hist.device == device, f'{what} must live on {device}')


def clip_histogram(tensor: torch.Tensor, keys: torch.Tensor, *, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                   ctx: Optional[Context] = None) -> torch.Tensor:
    """int64[8192] counts of ``tensor`` against the range in ``keys`` (int32[2], ``piquant.distributed.local_minmax_keys`` -- of this tensor, or
    MIN-reduced over the shards of a larger one).  ``accumulate=True`` adds to ``out`` instead of overwriting it.  One streaming launch plus a
    fold, asynchronous on the current stream."""
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    _check_float_input(tensor)
    _check_clip_keys(keys, tensor.device)
    _require(out is not None or not accumulate, 'accumulate=True needs out= (the counts to add to)')
    if out is None:
        out = torch.empty(CLIP_BINS, dtype=torch.int64, device=tensor.device)
    _check_clip_hist(out, tensor.device, 'out')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    ctx = _ctx_for(tensor, ctx)
    ctx.clip_histogram_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), tensor.numel(), keys.data_ptr(), out.data_ptr(), init=not accumulate,
                           _device_ptrs=True)
    return out


def quant_params_from_histogram(keys: torch.Tensor, hist: torch.Tensor, *, dtype: torch.dtype, steps: int = 63, ctx: Optional[Context] = None,
                                return_choice: bool = False, return_errors: bool = False):
    """The search on given keys and counts: the 16-byte parameter record, then -- where asked for -- the int32[1] choice and the float64[63] errors
    (NaN: candidate not evaluated), all on the device of ``keys``."""
    _check_modes(quant_dtype=dtype)
    _check_clip_params_steps(steps)
    _check_clip_keys(keys)
    _check_clip_hist(hist, keys.device, 'hist')
    params = torch.empty(PARAMS_NBYTES, dtype=torch.uint8, device=keys.device)
    choice = torch.empty(1, dtype=torch.int32, device=keys.device) if return_choice else None
    errors = torch.empty(CLIP_PARAMS_STEPS_MAX, dtype=torch.float64, device=keys.device) if return_errors else None
    ctx = _ctx_for(keys, ctx)
    ctx.quant_params_from_histogram_ptr(keys.data_ptr(), hist.data_ptr(), torch_to_piquant_dtype(dtype), steps, params.data_ptr(),
                                        0 if choice is None else choice.data_ptr(), 0 if errors is None else errors.data_ptr())
    extra = tuple(t for t in (choice, errors) if t is not None)
    return (params,) + extra if extra else params


def compute_quant_params_clipped_device(tensor: torch.Tensor, *, dtype: torch.dtype, steps: int = 63, ctx: Optional[Context] = None,
                                        out: Optional[torch.Tensor] = None, return_choice: bool = False):
    """``compute_quant_params_device`` with a search for the clipping range: ``steps`` ranges -- min and max both shrunk towards zero by
    ``1 - k / 64``, ``k < steps`` -- are judged on an 8192-bin histogram of the tensor, and the record of the one with the smallest estimated squared
    error is returned (the 16-byte uint8 device tensor ``quantize_dp`` / ``dequantize_dynamic`` take); with ``return_choice=True`` also the int32[1]
    device tensor of the chosen ``k``.  ``steps=1``, a constant, an empty and an all-NaN tensor give ``compute_quant_params_device``'s record.
    Asynchronous on the current stream: scan, histogram pass, search."""
    _check_modes(quant_dtype=dtype)
    _check_clip_params_steps(steps)
    _check_float_input(tensor)
    if out is None:
        out = torch.empty(PARAMS_NBYTES, dtype=torch.uint8, device=tensor.device)
    _check_params(out, tensor.device, 'out')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    choice = torch.empty(1, dtype=torch.int32, device=tensor.device) if return_choice else None
    ctx = _ctx_for(tensor, ctx)
    ctx.compute_quant_params_clipped_device_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), tensor.numel(), torch_to_piquant_dtype(dtype), steps,
                                                out.data_ptr(), 0 if choice is None else choice.data_ptr(), _device_ptrs=True)
    return (out, choice) if return_choice else out


def compute_quant_params_clipped(tensor: torch.Tensor, *, dtype: torch.dtype, steps: int = 63, ctx: Optional[Context] = None) -> Tuple[float, int]:
    """(scale, zero_point) of ``compute_quant_params_clipped_device`` on the host (synchronises)."""
    return params_to_host(compute_quant_params_clipped_device(tensor, dtype=dtype, steps=steps, ctx=ctx))


def quantize_dynamic(tensor: torch.Tensor, *, dtype: torch.dtype, round_mode: str = 'nearest', ctx: Optional[Context] = None,
                     out: Optional[torch.Tensor] = None, params: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``compute_quant_params`` + ``quantize`` in one asynchronous call, parameters computed and kept on the device.  Returns
    (quantized, parameter record).  A tensor that fits on the chip (up to ~113 MB on an MI355X) is read from HBM once, by a single
    kernel that keeps it in registers / LDS between the min/max pass and the quantization; larger ones take two launches (scan with the parameter epilogue, then quantize)."""
    _check_modes(quant_dtype=dtype)
    _check_float_input(tensor)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    if params is None:
        params = torch.empty(PARAMS_NBYTES, dtype=torch.uint8, device=tensor.device)
    _check_params(params, tensor.device)
    out = _packed_out(out, dtype, tensor, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_dynamic_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), torch_to_piquant_dtype(dtype), tensor.numel(),
                             params.data_ptr(), _ROUND_MODES[round_mode], _device_ptrs=True)
    return out, params


def dequantize_dynamic(tensor: torch.Tensor, params: torch.Tensor, *, dtype: torch.dtype, reduce_op: str = 'set',
                       ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None, quant_dtype: Optional[torch.dtype] = None,
                       shape=None) -> torch.Tensor:
    """``dequantize`` with (scale, zero_point) read from a device parameter record."""
    _check_modes(float_dtype=dtype)
    _require(isinstance(tensor, torch.Tensor) and tensor.is_cuda, 'dequantize_dynamic needs a ROCm device tensor')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    dtype_in, logical_shape = _quant_meta(tensor, quant_dtype, shape)
    numel = _numel_of(logical_shape)
    _check_packed_in(tensor, dtype_in, numel, tensor.device, 'tensor')
    _check_params(params, tensor.device)
    out = _float_out(out, reduce_op, dtype, logical_shape, numel, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.dequantize_dp_ptr(tensor.data_ptr(), dtype_in, out.data_ptr(), torch_to_piquant_dtype(out.dtype), numel, params.data_ptr(),
                          _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return out


# ---- group-wise quantization: one (scale, zero point) per run of group_size contiguous elements --------------------------------------------
GROUP_SIZES = tuple(1 << k for k in range(5, 13))   # powers of two in [32, 4096]


def num_groups(numel: int, group_size: int) -> int:
    """Groups of a tensor of ``numel`` elements (the last one may be partial)."""
    return (int(numel) + int(group_size) - 1) // int(group_size)


def _check_group_size(group_size) -> None:
    _require(isinstance(group_size, int) and not isinstance(group_size, bool) and group_size in GROUP_SIZES,
             f'group_size must be a power of two in [32, 4096], got {group_size!r}')


_GIVEN_PAIR = 'pass both scales and zero_points (given parameters) or neither (computed parameters)'
_OUT_PAIR = 'pass both out_scales and out_zero_points or neither'


def _check_group_params(scales, zero_points, ngroups: int) -> None:
    """Shape and dtype of the per-group parameters (device placement is checked against the tensor separately)."""
    _require(isinstance(scales, torch.Tensor) and scales.dtype == torch.float32 and scales.dim() == 1 and scales.numel() == ngroups and scales.is_contiguous(),
             f'scales must be a contiguous 1-D float32 tensor of {ngroups} elements')
    _require(isinstance(zero_points, torch.Tensor) and zero_points.dtype == torch.uint8 and zero_points.dim() == 1 and zero_points.numel() == ngroups and
             zero_points.is_contiguous(), f'zero_points must be a contiguous 1-D uint8 tensor of {ngroups} elements')


def quantize_grouped(tensor: torch.Tensor, *, dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest', ctx: Optional[Context] = None,
                     out: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
                     zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Group-wise quantization: the flattened tensor is cut into ``ceil(numel / group_size)`` groups of ``group_size`` contiguous elements
    (the last may be partial), each with its own (scale, zero point).  Returns (quantized, scales, zero_points): the quantized tensor has the
    input's shape and ``dtype``; ``scales`` is float32[ngroups], ``zero_points`` uint8[ngroups], both on the tensor's device.  Group g's
    parameters equal ``compute_quant_params`` of that slice and its bytes equal the position-independent quantize of the slice with them.
    Passing both ``scales`` and ``zero_points`` quantizes with those parameters instead of computing them.  One asynchronous launch on the
    current stream (``include/piquant_hip.h``, piquant_hip_quantize_grouped)."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    _require((scales is None) == (zero_points is None), _GIVEN_PAIR)
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    given = scales is not None
    if given:
        _check_group_params(scales, zero_points, num_groups(tensor.numel(), group_size))
    _check_float_input(tensor)
    scales, zero_points = _group_params_of(scales, zero_points, tensor.numel(), group_size, tensor.device, shapes_checked=True)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _packed_out(out, dtype, tensor, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_grouped_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), torch_to_piquant_dtype(dtype), tensor.numel(),
                             group_size, scales.data_ptr(), zero_points.data_ptr(), given, _ROUND_MODES[round_mode], _device_ptrs=True)
    return out, scales, zero_points


CLIP_STEPS_MAX = 12   # candidate ranges of the clip search: r_k = 1 - k / 16, k < steps


def _check_clip_steps(steps) -> None:
    _require(isinstance(steps, int) and not isinstance(steps, bool) and 1 <= steps <= CLIP_STEPS_MAX,
             f'steps must be an int in [1, {CLIP_STEPS_MAX}], got {steps!r}')


def _check_choices(choices, ngroups: int, device: torch.device, what: str) -> None:
    _require(isinstance(choices, torch.Tensor) and choices.dtype == torch.uint8 and choices.dim() == 1 and choices.numel() == ngroups and
             choices.is_contiguous(), f'{what} must be a contiguous 1-D uint8 tensor of {ngroups} elements')
    _require(choices.device == device, f'{what} must live on {device}')


def quantize_grouped_clipped(tensor: torch.Tensor, *, dtype: torch.dtype, group_size: int = 128, steps: int = 9, round_mode: str = 'nearest',
                             ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None, out_scales: Optional[torch.Tensor] = None,
                             out_zero_points: Optional[torch.Tensor] = None, out_choices: Optional[torch.Tensor] = None,
                             return_choices: bool = False):
    """``quantize_grouped`` (computed parameters) with a per-group search for the clipping range, in one launch: every full group tries ``steps``
    ranges -- its min and max both shrunk towards zero by ``1 - k / 16``, ``k < steps`` -- and is quantized with the one whose nearest round trip
    has the smallest squared error (ties keep the smaller ``k``; ``k = 0`` is ``quantize_grouped``'s range).  On a narrow wire this is worth a
    large part of the error (uint2, Gaussian, group_size 128: about half); a searched group is an ordinary group, so ``dequantize_grouped`` and
    every other consumer take the result as it is.  Constant and all-NaN groups and a ragged last group are not searched; ``steps=1`` is
    ``quantize_grouped`` bit for bit.  Returns (quantized, scales, zero_points), and with ``return_choices=True`` also the uint8[ngroups] tensor
    of the chosen ``k`` (``include/piquant_hip.h``, piquant_hip_quantize_grouped_clipped, has the definition)."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    _check_clip_steps(steps)
    _require((out_scales is None) == (out_zero_points is None), _OUT_PAIR)
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    ngroups = num_groups(tensor.numel(), group_size)
    if out_scales is not None:
        _check_group_params(out_scales, out_zero_points, ngroups)
    _check_float_input(tensor)
    scales, zero_points = _group_params_of(out_scales, out_zero_points, tensor.numel(), group_size, tensor.device, 'out_scales and out_zero_points',
                                           shapes_checked=True)
    if out_choices is not None:
        _check_choices(out_choices, ngroups, tensor.device, 'out_choices')
    elif return_choices:
        out_choices = torch.empty(ngroups, dtype=torch.uint8, device=tensor.device)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _packed_out(out, dtype, tensor, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_grouped_clipped_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), torch_to_piquant_dtype(dtype),
                                     tensor.numel(), group_size, scales.data_ptr(), zero_points.data_ptr(),
                                     0 if out_choices is None else out_choices.data_ptr(), steps, _ROUND_MODES[round_mode], _device_ptrs=True)
    return (out, scales, zero_points, out_choices) if return_choices else (out, scales, zero_points)


def quantize_grouped_clipped_batch(tensors, *, dtype: torch.dtype, group_size: int = 128, steps: int = 9, round_mode: str = 'nearest',
                                   ctx: Optional[Context] = None, outs=None, scales=None, zero_points=None, choices=None,
                                   return_choices: bool = False):
    """``quantize_grouped_clipped`` of several independent tensors (one dtype pair, group size, ``steps`` and round mode) with one kernel launch per
    16 tensors.  Returns (outs, scales, zero_points) as lists -- ``scales`` / ``zero_points`` are outputs, given or allocated -- and with
    ``return_choices=True`` also the list of choices; tensor i's entries equal ``quantize_grouped_clipped(tensors[i])`` (a stochastic batch draws
    one threshold) (``include/piquant_hip.h``, piquant_hip_quantize_grouped_clipped_batch)."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    _check_clip_steps(steps)
    _require((scales is None) == (zero_points is None), 'pass both scales and zero_points or neither')
    tensors = list(tensors)
    lists = [tensors]
    for given in (outs, scales, zero_points, choices):
        if given is not None:
            lists.append(list(given))
    _check_batch_lists(*lists)
    for i, t in enumerate(tensors):
        _check_float_input(t, f'tensors[{i}]')
        _require(t.device == tensors[0].device and t.dtype == tensors[0].dtype, 'the tensors of a batch must share one device and one dtype')
    device = tensors[0].device
    tensors = _contiguous(tensors)
    numels = [t.numel() for t in tensors]
    scales, zero_points = _group_params(None if scales is None else list(scales), None if zero_points is None else list(zero_points), numels, group_size,
                                        device, 'scales and zero_points')
    if choices is not None:
        choices = list(choices)
        for i, (c, n) in enumerate(zip(choices, numels)):
            _check_choices(c, num_groups(n, group_size), device, f'choices[{i}]')
    elif return_choices:
        choices = [torch.empty(num_groups(n, group_size), dtype=torch.uint8, device=device) for n in numels]
    outs = _packed_outs(None if outs is None else list(outs), dtype, tensors, device)
    ctx = _ctx_for(tensors[0], ctx)
    ctx.quantize_grouped_clipped_batch_ptr(_ptrs(tensors), torch_to_piquant_dtype(tensors[0].dtype), _ptrs(outs), torch_to_piquant_dtype(dtype), numels,
                                           group_size, _ptrs(scales), _ptrs(zero_points), None if choices is None else _ptrs(choices), steps,
                                           _ROUND_MODES[round_mode], _device_ptrs=True)
    return (outs, scales, zero_points, choices) if return_choices else (outs, scales, zero_points)


def dequantize_grouped(tensor: torch.Tensor, scales: torch.Tensor, zero_points: torch.Tensor, *, dtype: torch.dtype, group_size: int,
                       reduce_op: str = 'set', ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None,
                       quant_dtype: Optional[torch.dtype] = None, shape=None) -> torch.Tensor:
    """Inverse of ``quantize_grouped``: group g of the result (``reduce_op='set'``) or of ``out`` (``'add'``) is the dequantized group g with
    ``scales[g]`` / ``zero_points[g]``.  A raw uint8 buffer of packed bytes needs ``quant_dtype=`` and ``shape=``."""
    _check_modes(float_dtype=dtype, reduce_op=reduce_op, group_size=group_size)
    _require(isinstance(tensor, torch.Tensor) and (tensor.dtype in _QUANT_TYPES or quant_dtype is not None), 'tensor must be a quantized tensor')
    dtype_in, logical_shape = _quant_meta(tensor, quant_dtype, shape)
    numel = _numel_of(logical_shape)
    _check_group_params(scales, zero_points, num_groups(numel, group_size))
    _require(tensor.is_cuda, 'dequantize_grouped needs a ROCm device tensor')
    _require(scales.device == tensor.device and zero_points.device == tensor.device, f'scales and zero_points must live on {tensor.device}')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    _check_packed_in(tensor, dtype_in, numel, tensor.device, 'tensor')
    out = _float_out(out, reduce_op, dtype, logical_shape, numel, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.dequantize_grouped_ptr(tensor.data_ptr(), dtype_in, out.data_ptr(), torch_to_piquant_dtype(out.dtype), numel, group_size, scales.data_ptr(),
                               zero_points.data_ptr(), _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return out


def _check_seed(seed) -> int:
    """The rotation's seed: any Python int, taken modulo 2^64 (``_NA``: the call was made without one)."""
    _require(seed is not _NA, 'seed= is required: the rotation is defined by it, and the inverse needs the same one')
    _require(isinstance(seed, int) and not isinstance(seed, bool), f'seed must be an int, got {seed!r}')
    return seed & 0xFFFFFFFFFFFFFFFF


def hadamard_grouped(tensor: torch.Tensor, *, group_size: int = 128, seed=_NA, inverse: bool = False, out: Optional[torch.Tensor] = None,
                     ctx: Optional[Context] = None) -> torch.Tensor:
    """The randomized Hadamard rotation of every full group of ``group_size`` contiguous elements of the flattened tensor: random signs drawn from
    ``seed`` (the same for every group), the Walsh-Hadamard butterflies in float32, the factor ``group_size ** -0.5``; ``inverse=True`` undoes it
    (``include/piquant_hip.h``, piquant_hip_hadamard_grouped, has the definition).  Orthogonal: group norms and L2 errors are those of the original
    domain.  bfloat16 is transformed in float32 and rounded on store.  A ragged last group is not rotated.  ``out`` may be ``tensor`` (in place).
    One asynchronous launch on the current stream."""
    _check_modes(group_size=group_size)
    seed = _check_seed(seed)
    _check_float_input(tensor)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _float_out(out, 'set', tensor.dtype, tensor.shape, tensor.numel(), tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.hadamard_grouped_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), tensor.numel(), group_size, seed, bool(inverse),
                             _device_ptrs=True)
    return out


def quantize_grouped_rotated(tensor: torch.Tensor, *, dtype: torch.dtype, group_size: int = 128, seed=_NA, round_mode: str = 'nearest',
                             ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None, out_scales: Optional[torch.Tensor] = None,
                             out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``quantize_grouped`` (computed parameters) of the rotated tensor, in one launch that never writes the rotated tensor: bit for bit
    ``quantize_grouped(hadamard_grouped(tensor.float(), group_size=group_size, seed=seed), dtype=dtype, ...)``.  An outlier no longer stretches the
    step of its group: heavy-tailed data loses 3 to 30 times less, Gaussian data the same, flat data more.  Returns (quantized, scales,
    zero_points) as ``quantize_grouped`` does; ``dequantize_grouped_rotated`` with the same ``seed`` is the way back
    (``include/piquant_hip.h``, piquant_hip_quantize_grouped_rotated)."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    seed = _check_seed(seed)
    _require((out_scales is None) == (out_zero_points is None), _OUT_PAIR)
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    if out_scales is not None:
        _check_group_params(out_scales, out_zero_points, num_groups(tensor.numel(), group_size))
    _check_float_input(tensor)
    scales, zero_points = _group_params_of(out_scales, out_zero_points, tensor.numel(), group_size, tensor.device, 'out_scales and out_zero_points',
                                           shapes_checked=True)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _packed_out(out, dtype, tensor, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_grouped_rotated_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), torch_to_piquant_dtype(dtype),
                                     tensor.numel(), group_size, scales.data_ptr(), zero_points.data_ptr(), seed, _ROUND_MODES[round_mode],
                                     _device_ptrs=True)
    return out, scales, zero_points


def dequantize_grouped_rotated(tensor: torch.Tensor, scales: torch.Tensor, zero_points: torch.Tensor, *, dtype: torch.dtype, group_size: int,
                               seed=_NA, reduce_op: str = 'set', ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None,
                               quant_dtype: Optional[torch.dtype] = None, shape=None) -> torch.Tensor:
    """Inverse of ``quantize_grouped_rotated``: the float32 ``dequantize_grouped`` of the tensor, rotated back with ``seed``, stored
    (``reduce_op='set'``) or added into ``out`` (``'add'``: one float32 add, one rounding), in one launch that never writes the un-rotated
    intermediate (``include/piquant_hip.h``, piquant_hip_dequantize_grouped_rotated).  A raw uint8 buffer of packed bytes needs ``quant_dtype=``
    and ``shape=``."""
    _check_modes(float_dtype=dtype, reduce_op=reduce_op, group_size=group_size)
    seed = _check_seed(seed)
    _require(isinstance(tensor, torch.Tensor) and (tensor.dtype in _QUANT_TYPES or quant_dtype is not None), 'tensor must be a quantized tensor')
    dtype_in, logical_shape = _quant_meta(tensor, quant_dtype, shape)
    numel = _numel_of(logical_shape)
    _check_group_params(scales, zero_points, num_groups(numel, group_size))
    _require(tensor.is_cuda, 'dequantize_grouped_rotated needs a ROCm device tensor')
    _require(scales.device == tensor.device and zero_points.device == tensor.device, f'scales and zero_points must live on {tensor.device}')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    _check_packed_in(tensor, dtype_in, numel, tensor.device, 'tensor')
    out = _float_out(out, reduce_op, dtype, logical_shape, numel, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.dequantize_grouped_rotated_ptr(tensor.data_ptr(), dtype_in, out.data_ptr(), torch_to_piquant_dtype(out.dtype), numel, group_size,
                                       scales.data_ptr(), zero_points.data_ptr(), seed, _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return out


def reduce_quantize_grouped(acc: torch.Tensor, tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest',
                            ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None, out_scales: Optional[torch.Tensor] = None,
                            out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``quantize_grouped(acc + dequantize_grouped(tensors[0]) + ... + dequantize_grouped(tensors[k - 1]))`` in one launch (up to 16 terms) that
    never stores the sum.  Term i is a packed tensor of ``dtype`` (or the raw uint8 buffer of its bytes) with ``acc.numel()`` elements and its
    own per-group ``scales[i]`` / ``zero_points[i]`` (same ``group_size``).  The bytes, scales and zero points are exactly those of
    ``dequantize_grouped(tensors[i], ..., reduce_op='add', out=acc)`` for every i in order followed by ``quantize_grouped(acc)``.  Returns
    (out, out_scales, out_zero_points) as ``quantize_grouped`` does; ``acc`` is unspecified afterwards (``include/piquant_hip.h``,
    piquant_hip_reduce_quantize_grouped)."""
    return _reduce_quantize_grouped(acc, _NA, tensors, scales, zero_points, dtype, group_size, round_mode, ctx, out, out_scales, out_zero_points)


def reduce_quantize_grouped_rotated(acc: torch.Tensor, tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int = 128, seed=_NA,
                                    round_mode: str = 'nearest', ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None,
                                    out_scales: Optional[torch.Tensor] = None,
                                    out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``reduce_quantize_grouped`` in the rotated domain, in one launch (at most 16 terms; more raise): the terms are records made by
    ``quantize_grouped_rotated`` with the same ``seed``, so only ``acc`` is rotated.  Bit for bit ``y = hadamard_grouped(acc.float(), seed=seed)``,
    ``dequantize_grouped(tensors[i], ..., dtype=torch.float32, reduce_op='add', out=y)`` for every i in order, ``quantize_grouped(y)``: the sum
    stays float32 until it is quantized, also for a bfloat16 ``acc``, which -- unlike ``reduce_quantize_grouped``'s -- is only read.  No terms is
    ``quantize_grouped_rotated(acc)``.  Returns (out, out_scales, out_zero_points) (``include/piquant_hip.h``,
    piquant_hip_reduce_quantize_grouped_rotated)."""
    seed = _check_seed(seed)
    return _reduce_quantize_grouped(acc, _NA, tensors, scales, zero_points, dtype, group_size, round_mode, ctx, out, out_scales, out_zero_points, seed)


def _reduce_quantize_grouped(acc, residual, tensors, scales, zero_points, dtype, group_size, round_mode, ctx, out, out_scales, out_zero_points, seed=None):
    """``reduce_quantize_grouped`` (``residual`` is ``_NA``) and ``reduce_quantize_grouped_ef``: the second checks the residual and makes the ``_ef`` call.
    With a ``seed`` (and no residual): ``reduce_quantize_grouped_rotated``, which takes at most 16 terms."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    tensors, scales, zero_points = list(tensors), list(scales), list(zero_points)
    _require(seed is None or len(tensors) <= 16, f'reduce_quantize_grouped_rotated takes at most 16 terms, got {len(tensors)}')
    _require(len(tensors) == len(scales) == len(zero_points), f'tensors, scales and zero_points must have the same length, got '
             f'{len(tensors)}, {len(scales)} and {len(zero_points)}')
    if residual is not _NA:
        _require(isinstance(acc, torch.Tensor) and acc.dtype in _DEQUANT_TYPES, 'acc must be a float32 or bfloat16 tensor')
        _check_residual(residual, acc)
    _check_float_input(acc, 'acc')
    _require(acc.is_contiguous(), 'acc must be contiguous (it is the accumulator)')
    _require((out_scales is None) == (out_zero_points is None), _OUT_PAIR)
    numel = acc.numel()
    qdt = torch_to_piquant_dtype(dtype)
    _check_grouped_terms(tensors, scales, zero_points, qdt, repeat(numel), group_size, acc.device)
    out = _packed_out(out, dtype, acc, acc.device)
    out_scales, out_zero_points = _group_params_of(out_scales, out_zero_points, numel, group_size, acc.device, 'out_scales and out_zero_points')
    ctx = _ctx_for(acc, ctx)
    if seed is not None:
        ctx.reduce_quantize_grouped_rotated_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), _ptrs(tensors), _ptrs(scales), _ptrs(zero_points),
                                                out.data_ptr(), qdt, numel, group_size, out_scales.data_ptr(), out_zero_points.data_ptr(), seed,
                                                _ROUND_MODES[round_mode], _device_ptrs=True)
    elif residual is _NA:
        ctx.reduce_quantize_grouped_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), _ptrs(tensors), _ptrs(scales), _ptrs(zero_points), out.data_ptr(), qdt,
                                        numel, group_size, out_scales.data_ptr(), out_zero_points.data_ptr(), _ROUND_MODES[round_mode], _device_ptrs=True)
    else:
        ctx.reduce_quantize_grouped_ef_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), residual.data_ptr(), _ptrs(tensors), _ptrs(scales),
                                           _ptrs(zero_points), out.data_ptr(), qdt, numel, group_size, out_scales.data_ptr(), out_zero_points.data_ptr(),
                                           _ROUND_MODES[round_mode], _device_ptrs=True, residual_dtype=_residual_dtype(residual, acc))
    return out, out_scales, out_zero_points


def _check_batch_lists(*lists) -> None:
    _require(len(lists[0]) > 0, 'the batch is empty')
    _require(all(len(x) == len(lists[0]) for x in lists), f'the lists of a batch must have the same length, got {[len(x) for x in lists]}')


def quantize_grouped_batch(tensors, *, dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest', ctx: Optional[Context] = None,
                           outs=None, scales=None, zero_points=None):
    """``quantize_grouped`` of several independent tensors (one dtype pair, group size and round mode) with one kernel launch per 16 tensors.
    Returns (outs, scales, zero_points) as lists; tensor i's entries equal ``quantize_grouped(tensors[i])`` (a stochastic batch draws one
    threshold).  Passing ``scales`` and ``zero_points`` (lists) quantizes with those parameters instead of computing them."""
    return _quantize_grouped_batch(tensors, _NA, dtype, group_size, round_mode, ctx, outs, scales, zero_points, _GIVEN_PAIR, 'scales and zero_points')


def _quantize_grouped_batch(tensors, residuals, dtype, group_size, round_mode, ctx, outs, scales, zero_points, pair_rule: str, what: str, seed=None):
    """``quantize_grouped_batch`` (``residuals`` is ``_NA``; ``scales`` / ``zero_points`` are given parameters) and ``quantize_grouped_ef_batch`` (they are
    its ``out_scales`` / ``out_zero_points``): the second checks the residuals and makes the ``_ef`` call.  With a ``seed``: their rotated forms,
    whose parameters are always computed (``scales`` / ``zero_points`` are outputs) and whose residuals are float32."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    _require((scales is None) == (zero_points is None), pair_rule)
    tensors = list(tensors)
    lists = [tensors]
    if residuals is not _NA:
        residuals = list(residuals)
        lists.append(residuals)
    if outs is not None:
        outs = list(outs)
        lists.append(outs)
    given = scales is not None
    if given:
        scales, zero_points = list(scales), list(zero_points)
        lists += [scales, zero_points]
    _check_batch_lists(*lists)
    if residuals is not _NA:
        for i, (t, r) in enumerate(zip(tensors, residuals)):
            _require(isinstance(t, torch.Tensor) and t.dtype in _DEQUANT_TYPES, f'tensors[{i}] must be a float32 or bfloat16 tensor')
            if seed is not None:
                _check_rotated_residual(r, t, f'residuals[{i}]')
                continue
            _check_residual(r, t, f'residuals[{i}]')
            _require(r.dtype == residuals[0].dtype, f'the residuals of a batch must share one dtype, got {residuals[0].dtype} and {r.dtype}')
    for i, t in enumerate(tensors):
        _check_float_input(t, f'tensors[{i}]')
        _require(t.device == tensors[0].device and t.dtype == tensors[0].dtype, 'the tensors of a batch must share one device and one dtype')
    device = tensors[0].device
    tensors = _contiguous(tensors)
    numels = [t.numel() for t in tensors]
    scales, zero_points = _group_params(scales, zero_points, numels, group_size, device, what)
    outs = _packed_outs(outs, dtype, tensors, device)
    ctx = _ctx_for(tensors[0], ctx)
    fdt, qdt, mode = torch_to_piquant_dtype(tensors[0].dtype), torch_to_piquant_dtype(dtype), _ROUND_MODES[round_mode]
    if seed is not None and residuals is _NA:
        ctx.quantize_grouped_rotated_batch_ptr(_ptrs(tensors), fdt, _ptrs(outs), qdt, numels, group_size, _ptrs(scales), _ptrs(zero_points), seed, mode,
                                               _device_ptrs=True)
    elif seed is not None:
        ctx.quantize_grouped_rotated_ef_batch_ptr(_ptrs(tensors), fdt, _ptrs(residuals), _ptrs(outs), qdt, numels, group_size, _ptrs(scales),
                                                  _ptrs(zero_points), seed, mode, _device_ptrs=True)
    elif residuals is _NA:
        ctx.quantize_grouped_batch_ptr(_ptrs(tensors), fdt, _ptrs(outs), qdt, numels, group_size, _ptrs(scales), _ptrs(zero_points), given, mode, _device_ptrs=True)
    else:
        ctx.quantize_grouped_ef_batch_ptr(_ptrs(tensors), fdt, _ptrs(residuals), _ptrs(outs), qdt, numels, group_size, _ptrs(scales), _ptrs(zero_points), mode,
                                          _device_ptrs=True, residual_dtype=_residual_dtype(residuals[0], tensors[0]))
    return outs, scales, zero_points


def quantize_dequantize_grouped(tensor: torch.Tensor, *, quant_dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest',
                                reduce_op: str = 'set', scales: Optional[torch.Tensor] = None, zero_points: Optional[torch.Tensor] = None,
                                return_params: bool = False, ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None):
    """Group-wise fake quantization: ``out (op)= dequantize_grouped(quantize_grouped(tensor))`` -- what the tensor looks like after a group-wise
    round trip through ``quant_dtype`` -- bit for bit those two calls, in one launch that reads the tensor once and never writes the packed
    bytes.  Returns ``out`` (the input's shape and dtype), or ``(out, scales, zero_points)`` with ``return_params=True``.  ``scales`` and
    ``zero_points`` given together mean "quantize with these per-group parameters"; otherwise they are computed (and only materialised when
    ``return_params``).  ``reduce_op='add'`` accumulates into ``out=``; ``out=tensor`` is in place, for both ops (``include/piquant_hip.h``,
    piquant_hip_quantize_dequantize_grouped)."""
    _check_modes(quant_dtype=quant_dtype, round_mode=round_mode, reduce_op=reduce_op, group_size=group_size)
    _require((scales is None) == (zero_points is None), _GIVEN_PAIR)
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    given = scales is not None
    if given:
        _check_group_params(scales, zero_points, num_groups(tensor.numel(), group_size))
    out = _float_out(out, reduce_op, tensor.dtype, tensor.shape, tensor.numel(), tensor.device)
    _check_float_input(tensor)
    if given or return_params:
        scales, zero_points = _group_params_of(scales, zero_points, tensor.numel(), group_size, tensor.device, shapes_checked=True)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_dequantize_grouped_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), out.data_ptr(), torch_to_piquant_dtype(quant_dtype),
                                        tensor.numel(), group_size, 0 if scales is None else scales.data_ptr(),
                                        0 if zero_points is None else zero_points.data_ptr(), given, _ROUND_MODES[round_mode], _REDUCE_OPS[reduce_op],
                                        _device_ptrs=True)
    return (out, scales, zero_points) if return_params else out


def quantize_dequantize_grouped_batch(tensors, *, quant_dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest', reduce_op: str = 'set',
                                      scales=None, zero_points=None, return_params: bool = False, ctx: Optional[Context] = None, outs=None):
    """``quantize_dequantize_grouped`` of several independent tensors (one dtype, quantized dtype, group size, round mode and op) with one kernel
    launch per 16 tensors.  Returns ``outs``, or ``(outs, scales, zero_points)`` (lists) with ``return_params=True``; tensor i's entries equal the
    single call on it (a stochastic batch draws one threshold).  ``scales`` and ``zero_points`` (lists) given together quantize with those
    parameters; ``reduce_op='add'`` needs ``outs=``; ``outs[i]`` may be ``tensors[i]``."""
    tensors = list(tensors)
    _check_modes(quant_dtype=quant_dtype, round_mode=round_mode, reduce_op=reduce_op, group_size=group_size)
    _require((scales is None) == (zero_points is None), _GIVEN_PAIR)
    _require(all(isinstance(t, torch.Tensor) and t.dtype in _DEQUANT_TYPES for t in tensors), 'tensor must be a float32 or bfloat16 tensor')
    given = scales is not None
    _require(outs is not None or reduce_op != 'add', "reduce_op='add' accumulates into outs=; pass the accumulator tensors")
    lists = [tensors]
    if outs is not None:
        outs = list(outs)
        lists.append(outs)
    if given:
        scales, zero_points = list(scales), list(zero_points)
        lists += [scales, zero_points]
    _check_batch_lists(*lists)
    _require(all(t.device == tensors[0].device and t.dtype == tensors[0].dtype for t in tensors), 'the tensors of a batch must share one device and one dtype')
    device = tensors[0].device
    numels = [t.numel() for t in tensors]
    if given:
        for sc, zp, n in zip(scales, zero_points, numels):
            _check_group_params(sc, zp, num_groups(n, group_size))
    outs = _float_outs(outs, reduce_op, tensors[0].dtype, [t.shape for t in tensors], numels, device)
    for i, t in enumerate(tensors):
        _check_float_input(t, f'tensors[{i}]')
    if given or return_params:
        scales, zero_points = _group_params(scales, zero_points, numels, group_size, device, shapes_checked=True)
    tensors = _contiguous(tensors)
    ctx = _ctx_for(tensors[0], ctx)
    ctx.quantize_dequantize_grouped_batch_ptr(_ptrs(tensors), torch_to_piquant_dtype(tensors[0].dtype), _ptrs(outs), torch_to_piquant_dtype(quant_dtype), numels,
                                              group_size, None if scales is None else _ptrs(scales), None if zero_points is None else _ptrs(zero_points), given,
                                              _ROUND_MODES[round_mode], _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return (outs, scales, zero_points) if return_params else outs


def _check_residual(residual, tensor: torch.Tensor, what: str = 'residual') -> None:
    """The residual of an error-feedback call is written by raw pointer: a contiguous device tensor of the input's device and numel, and of the
    input's dtype -- or float32 for a bfloat16 input (the float32 residual, ``piquant_hip_quantize_grouped_ef_mixed``); no other pair."""
    _require(isinstance(residual, torch.Tensor), f'{what} must be a torch.Tensor')
    _require(residual.dtype == tensor.dtype or (tensor.dtype == torch.bfloat16 and residual.dtype == torch.float32),
             f'{what} must have the dtype of the tensor ({tensor.dtype}), or torch.float32 for a torch.bfloat16 tensor, got {residual.dtype}')
    _require(residual.numel() == tensor.numel(), f'{what} must have the numel of the tensor ({tensor.numel()}), got {residual.numel()}')
    _require(residual.device == tensor.device, f'{what} must live on the device of the tensor ({tensor.device}), got {residual.device}')
    _require(residual.is_contiguous(), f'{what} must be contiguous (it is updated in place)')


def _residual_dtype(residual: torch.Tensor, tensor: torch.Tensor):
    """``residual_dtype=`` of the ``*_ef*_ptr`` methods: None (the old symbol) unless the residual's dtype differs from the tensor's."""
    return None if residual.dtype == tensor.dtype else torch_to_piquant_dtype(residual.dtype)


def quantize_grouped_ef(tensor: torch.Tensor, residual: torch.Tensor, *, dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest',
                        ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None, out_scales: Optional[torch.Tensor] = None,
                        out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``quantize_grouped`` with error feedback, in one launch: quantizes ``y = tensor + residual`` (rounded to the tensor's dtype) with computed
    per-group parameters and replaces ``residual`` by ``y - dequantize_grouped(quantized)`` (rounded to the tensor's dtype), so that the rounding
    error of this step is part of the next step's input.  Bit for bit ``torch.add`` -> ``quantize_grouped`` -> ``dequantize_grouped`` ->
    ``torch.sub``.  ``residual`` is a contiguous tensor of the tensor's dtype, device and numel that the caller keeps between steps (zeros before
    the first); ``tensor`` is not written.  Returns (quantized, scales, zero_points) as ``quantize_grouped`` does.  A constant group gets the
    degenerate (1.0, qmax >> 1) and a group whose range lies far from zero has its zero point clamped: most of such a group goes to the residual,
    which conserves it but does not make it representable (``include/piquant_hip.h``, piquant_hip_quantize_grouped_ef).
    A bfloat16 ``tensor`` also takes a float32 ``residual``: then ``y`` and the new residual are float32 and the call writes exactly what
    ``quantize_grouped_ef(tensor.float(), residual)`` writes, still in one launch -- the residual no longer loses up to 2^-9 |y| per rounding,
    as much as the half step of a uint8 wire (piquant_hip_quantize_grouped_ef_mixed).  No other pair of dtypes is accepted."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    _require((out_scales is None) == (out_zero_points is None), _OUT_PAIR)
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    _check_residual(residual, tensor)
    _check_float_input(tensor)
    out_scales, out_zero_points = _group_params_of(out_scales, out_zero_points, tensor.numel(), group_size, tensor.device, 'out_scales and out_zero_points')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _packed_out(out, dtype, tensor, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_grouped_ef_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), residual.data_ptr(), out.data_ptr(), torch_to_piquant_dtype(dtype),
                                tensor.numel(), group_size, out_scales.data_ptr(), out_zero_points.data_ptr(), _ROUND_MODES[round_mode], _device_ptrs=True,
                                residual_dtype=_residual_dtype(residual, tensor))
    return out, out_scales, out_zero_points


def reduce_quantize_grouped_ef(acc: torch.Tensor, residual: torch.Tensor, tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int = 128,
                               round_mode: str = 'nearest', ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None,
                               out_scales: Optional[torch.Tensor] = None,
                               out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``reduce_quantize_grouped`` with error feedback on the re-quantization, in one launch (up to 16 terms): quantizes
    ``y = acc + dequantize_grouped(tensors[0]) + ... + dequantize_grouped(tensors[k - 1]) + residual`` with computed per-group parameters and
    replaces ``residual`` by ``y - dequantize_grouped(quantized)``.  The two-call identity: the bytes, scales, zero points and residual are exactly
    those of ``dequantize_grouped(tensors[i], ..., reduce_op='add', out=acc)`` for every i in order (the running sum rounded to ``acc``'s dtype after
    each term) followed by ``quantize_grouped_ef(acc, residual)`` -- the residual is added AFTER the terms.  ``residual`` is a contiguous tensor of
    ``acc``'s dtype, device and numel that the caller keeps between steps (zeros before the first); the terms are as for
    ``reduce_quantize_grouped``.  Returns (out, out_scales, out_zero_points); ``acc`` is unspecified afterwards (``include/piquant_hip.h``,
    piquant_hip_reduce_quantize_grouped_ef).  A bfloat16 ``acc`` also takes a float32 ``residual``: the same two-call identity with the mixed
    ``quantize_grouped_ef(acc, residual)`` as its second call, in one launch like the others (``acc`` 8-byte aligned is enough for this pair)."""
    return _reduce_quantize_grouped(acc, residual, tensors, scales, zero_points, dtype, group_size, round_mode, ctx, out, out_scales, out_zero_points)


def _check_rotated_residual(residual, tensor: torch.Tensor, what: str = 'residual') -> None:
    """The residual of an error-feedback call in the rotated domain: float32 whatever the tensor's dtype, contiguous, of the tensor's device and
    numel (it is updated in place by raw pointer)."""
    _require(isinstance(residual, torch.Tensor), f'{what} must be a torch.Tensor')
    _require(residual.dtype == torch.float32, f'{what} must be torch.float32 (a record of rotated float32 values, also for a bfloat16 tensor), got '
             f'{residual.dtype}')
    _require(residual.numel() == tensor.numel(), f'{what} must have the numel of the tensor ({tensor.numel()}), got {residual.numel()}')
    _require(residual.device == tensor.device, f'{what} must live on the device of the tensor ({tensor.device}), got {residual.device}')
    _require(residual.is_contiguous(), f'{what} must be contiguous (it is updated in place)')


def quantize_grouped_rotated_ef(tensor: torch.Tensor, residual: torch.Tensor, *, dtype: torch.dtype, group_size: int = 128, seed=_NA,
                                round_mode: str = 'nearest', ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None,
                                out_scales: Optional[torch.Tensor] = None,
                                out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``quantize_grouped_rotated`` with error feedback, the residual kept in the ROTATED domain, in one launch that never writes the rotated
    tensor: bit for bit ``quantize_grouped_ef(hadamard_grouped(tensor.float(), group_size=group_size, seed=seed), residual, ...)``.  ``residual``
    is a contiguous float32 tensor (float32 also for a bfloat16 ``tensor``) of the tensor's device and numel that the caller keeps between steps
    (zeros before the first); it belongs to one (``seed``, ``group_size``) and is not the residual ``quantize_grouped_ef`` keeps.
    ``hadamard_grouped(residual, seed=seed, inverse=True)`` is the original-domain residual up to float32 rounding: the way to change the seed or
    to stop rotating.  One NaN makes its whole rotated group NaN, and that group's residual stays NaN until the caller zeroes it.  ``tensor`` is
    not written.  Returns (quantized, scales, zero_points) (``include/piquant_hip.h``, piquant_hip_quantize_grouped_rotated_ef)."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    seed = _check_seed(seed)
    _require((out_scales is None) == (out_zero_points is None), _OUT_PAIR)
    _require(isinstance(tensor, torch.Tensor) and tensor.dtype in _DEQUANT_TYPES, 'tensor must be a float32 or bfloat16 tensor')
    _check_rotated_residual(residual, tensor)
    if out_scales is not None:
        _check_group_params(out_scales, out_zero_points, num_groups(tensor.numel(), group_size))
    _check_float_input(tensor)
    out_scales, out_zero_points = _group_params_of(out_scales, out_zero_points, tensor.numel(), group_size, tensor.device, 'out_scales and out_zero_points',
                                                   shapes_checked=True)
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    out = _packed_out(out, dtype, tensor, tensor.device)
    ctx = _ctx_for(tensor, ctx)
    ctx.quantize_grouped_rotated_ef_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), residual.data_ptr(), out.data_ptr(),
                                        torch_to_piquant_dtype(dtype), tensor.numel(), group_size, out_scales.data_ptr(), out_zero_points.data_ptr(), seed,
                                        _ROUND_MODES[round_mode], _device_ptrs=True)
    return out, out_scales, out_zero_points


def reduce_quantize_grouped_rotated_ef(acc: torch.Tensor, residual: torch.Tensor, tensors, scales, zero_points, *, dtype: torch.dtype,
                                       group_size: int = 128, seed=_NA, round_mode: str = 'nearest', ctx: Optional[Context] = None,
                                       out: Optional[torch.Tensor] = None, out_scales: Optional[torch.Tensor] = None,
                                       out_zero_points: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``reduce_quantize_grouped_rotated`` with error feedback on the re-quantization, the residual kept in the rotated domain, in one launch (at
    most 16 terms; more raise).  Bit for bit ``y = hadamard_grouped(acc.float(), seed=seed)``, ``dequantize_grouped(tensors[i], ...,
    dtype=torch.float32, reduce_op='add', out=y)`` for every i in order, ``quantize_grouped_ef(y, residual)``: the residual is added AFTER the
    terms.  ``residual`` is as for ``quantize_grouped_rotated_ef``; ``acc`` is only read.  No terms is ``quantize_grouped_rotated_ef(acc,
    residual)``.  Returns (out, out_scales, out_zero_points) (``include/piquant_hip.h``, piquant_hip_reduce_quantize_grouped_rotated_ef)."""
    _check_modes(quant_dtype=dtype, round_mode=round_mode, group_size=group_size)
    seed = _check_seed(seed)
    tensors, scales, zero_points = list(tensors), list(scales), list(zero_points)
    _require(len(tensors) <= 16, f'reduce_quantize_grouped_rotated_ef takes at most 16 terms, got {len(tensors)}')
    _require(len(tensors) == len(scales) == len(zero_points), f'tensors, scales and zero_points must have the same length, got '
             f'{len(tensors)}, {len(scales)} and {len(zero_points)}')
    _require(isinstance(acc, torch.Tensor) and acc.dtype in _DEQUANT_TYPES, 'acc must be a float32 or bfloat16 tensor')
    _check_rotated_residual(residual, acc)
    _check_float_input(acc, 'acc')
    _require(acc.is_contiguous(), 'acc must be contiguous (it is the accumulator)')
    _require((out_scales is None) == (out_zero_points is None), _OUT_PAIR)
    numel = acc.numel()
    qdt = torch_to_piquant_dtype(dtype)
    _check_grouped_terms(tensors, scales, zero_points, qdt, repeat(numel), group_size, acc.device)
    out = _packed_out(out, dtype, acc, acc.device)
    out_scales, out_zero_points = _group_params_of(out_scales, out_zero_points, numel, group_size, acc.device, 'out_scales and out_zero_points')
    ctx = _ctx_for(acc, ctx)
    ctx.reduce_quantize_grouped_rotated_ef_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), residual.data_ptr(), _ptrs(tensors), _ptrs(scales),
                                               _ptrs(zero_points), out.data_ptr(), qdt, numel, group_size, out_scales.data_ptr(),
                                               out_zero_points.data_ptr(), seed, _ROUND_MODES[round_mode], _device_ptrs=True)
    return out, out_scales, out_zero_points


def quantize_grouped_ef_batch(tensors, residuals, *, dtype: torch.dtype, group_size: int = 128, round_mode: str = 'nearest', ctx: Optional[Context] = None,
                              outs=None, out_scales=None, out_zero_points=None):
    """``quantize_grouped_ef`` of several independent (tensor, residual) pairs (one dtype pair, group size and round mode) with one kernel launch
    per 16 pairs.  Returns (outs, scales, zero_points) as lists; pair i's entries and its updated residual equal
    ``quantize_grouped_ef(tensors[i], residuals[i])`` (a stochastic batch draws one threshold).  The residuals of a batch share one dtype: the
    tensors', or float32 for bfloat16 tensors."""
    return _quantize_grouped_batch(tensors, residuals, dtype, group_size, round_mode, ctx, outs, out_scales, out_zero_points, _OUT_PAIR,
                                   'out_scales and out_zero_points')


def quantize_grouped_rotated_batch(tensors, *, dtype: torch.dtype, group_size: int = 128, seed=_NA, round_mode: str = 'nearest',
                                   ctx: Optional[Context] = None, outs=None, out_scales=None, out_zero_points=None):
    """``quantize_grouped_rotated`` of several independent tensors (one dtype pair, group size, ``seed`` and round mode) with one kernel launch per
    16 tensors.  Returns (outs, scales, zero_points) as lists; tensor i's entries equal ``quantize_grouped_rotated(tensors[i], seed=seed)`` (a
    stochastic batch draws one threshold).  A batch is its members, not their concatenation: the ragged last group of each tensor is not rotated
    (``include/piquant_hip.h``, piquant_hip_quantize_grouped_rotated_batch)."""
    seed = _check_seed(seed)
    return _quantize_grouped_batch(tensors, _NA, dtype, group_size, round_mode, ctx, outs, out_scales, out_zero_points, _OUT_PAIR,
                                   'out_scales and out_zero_points', seed)


def quantize_grouped_rotated_ef_batch(tensors, residuals, *, dtype: torch.dtype, group_size: int = 128, seed=_NA, round_mode: str = 'nearest',
                                      ctx: Optional[Context] = None, outs=None, out_scales=None, out_zero_points=None):
    """``quantize_grouped_rotated_ef`` of several independent (tensor, residual) pairs (one dtype pair, group size, ``seed`` and round mode) with
    one kernel launch per 16 pairs.  Returns (outs, scales, zero_points) as lists; pair i's entries and its updated residual equal
    ``quantize_grouped_rotated_ef(tensors[i], residuals[i], seed=seed)`` (a stochastic batch draws one threshold).  Every residual is float32, also
    for bfloat16 tensors (``include/piquant_hip.h``, piquant_hip_quantize_grouped_rotated_ef_batch)."""
    seed = _check_seed(seed)
    return _quantize_grouped_batch(tensors, residuals, dtype, group_size, round_mode, ctx, outs, out_scales, out_zero_points, _OUT_PAIR,
                                   'out_scales and out_zero_points', seed)


def dequantize_grouped_batch(tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int, reduce_op: str = 'set', ctx: Optional[Context] = None,
                             outs=None, quant_dtype: Optional[torch.dtype] = None, shapes=None):
    """``dequantize_grouped`` of several independent tensors with one kernel launch per 16 tensors; returns the list of outputs.  Raw uint8
    buffers of packed bytes need ``quant_dtype=`` and ``shapes=`` (one shape per tensor); ``reduce_op='add'`` accumulates into ``outs``."""
    return _dequantize_grouped_batch(tensors, scales, zero_points, dtype, group_size, reduce_op, ctx, outs, quant_dtype, shapes)


def dequantize_grouped_rotated_batch(tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int, seed=_NA, reduce_op: str = 'set',
                                     ctx: Optional[Context] = None, outs=None, quant_dtype: Optional[torch.dtype] = None, shapes=None):
    """``dequantize_grouped_rotated`` of several independent tensors (records made with the same ``seed``) with one kernel launch per 16 tensors;
    returns the list of outputs, output i equal to ``dequantize_grouped_rotated(tensors[i], scales[i], zero_points[i], seed=seed)``.  Raw uint8
    buffers of packed bytes need ``quant_dtype=`` and ``shapes=`` (one shape per tensor); ``reduce_op='add'`` accumulates into ``outs``
    (``include/piquant_hip.h``, piquant_hip_dequantize_grouped_rotated_batch)."""
    seed = _check_seed(seed)
    return _dequantize_grouped_batch(tensors, scales, zero_points, dtype, group_size, reduce_op, ctx, outs, quant_dtype, shapes, seed)


def _dequantize_grouped_batch(tensors, scales, zero_points, dtype, group_size, reduce_op, ctx, outs, quant_dtype, shapes, seed=None):
    """``dequantize_grouped_batch`` and, with a ``seed``, ``dequantize_grouped_rotated_batch``."""
    _check_modes(float_dtype=dtype, reduce_op=reduce_op, group_size=group_size)
    tensors, scales, zero_points = list(tensors), list(scales), list(zero_points)
    outs = None if outs is None else list(outs)
    lists = [tensors, scales, zero_points] + ([outs] if outs is not None else []) + ([list(shapes)] if shapes is not None else [])
    _check_batch_lists(*lists)
    _require(outs is not None or reduce_op != 'add', "reduce_op='add' accumulates into outs=; pass the accumulator tensors")
    metas = []
    for i, t in enumerate(tensors):
        _require(isinstance(t, torch.Tensor) and (t.dtype in _QUANT_TYPES or quant_dtype is not None), f'tensors[{i}] must be a quantized tensor')
        _require(t.is_cuda, 'dequantize_grouped_batch needs ROCm device tensors')
        metas.append(_quant_meta(t, quant_dtype, shapes[i] if shapes is not None else None))
    device = tensors[0].device
    _require(all(t.device == device for t in tensors) and all(m[0] == metas[0][0] for m in metas), 'the tensors of a batch must share one device and one dtype')
    tensors = _contiguous(tensors)
    numels = [_numel_of(shape) for _, shape in metas]
    _check_grouped_terms(tensors, scales, zero_points, metas[0][0], numels, group_size, device)
    outs = _float_outs(outs, reduce_op, dtype, [shape for _, shape in metas], numels, device)
    ctx = _ctx_for(tensors[0], ctx)
    if seed is not None:
        ctx.dequantize_grouped_rotated_batch_ptr(_ptrs(tensors), metas[0][0], _ptrs(outs), torch_to_piquant_dtype(dtype), numels, group_size, _ptrs(scales),
                                                 _ptrs(zero_points), seed, _REDUCE_OPS[reduce_op], _device_ptrs=True)
        return outs
    ctx.dequantize_grouped_batch_ptr(_ptrs(tensors), metas[0][0], _ptrs(outs), torch_to_piquant_dtype(dtype), numels, group_size, _ptrs(scales),
                                     _ptrs(zero_points), _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return outs


def dequantize_sum_grouped(tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int, reduce_op: str = 'set', ctx: Optional[Context] = None,
                           out: Optional[torch.Tensor] = None, quant_dtype: Optional[torch.dtype] = None, shape=None) -> torch.Tensor:
    """out (op)= ``dequantize_grouped(tensors[0]) + ... + dequantize_grouped(tensors[k - 1])`` in one launch (up to 16 terms) and one pass over
    ``out``.  Term i is a packed tensor (or, with ``quant_dtype=`` and ``shape=``, the raw uint8 buffer of its bytes) with its own per-group
    ``scales[i]`` / ``zero_points[i]`` (same ``group_size`` and numel).  The bytes are exactly those of ``dequantize_grouped(tensors[i], ...,
    out=out)`` for every i in order, the first with ``reduce_op`` and the others with 'add': the running sum is rounded to ``dtype`` after every
    term.  ``'add'`` accumulates into ``out=``; ``'set'`` never reads it.  Returns ``out`` (``include/piquant_hip.h``,
    piquant_hip_dequantize_sum_grouped)."""
    return _dequantize_sum_grouped(tensors, scales, zero_points, dtype, group_size, reduce_op, ctx, out, quant_dtype, shape)


def dequantize_sum_grouped_rotated(tensors, scales, zero_points, *, dtype: torch.dtype, group_size: int, seed=_NA, reduce_op: str = 'set',
                                   ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None, quant_dtype: Optional[torch.dtype] = None,
                                   shape=None) -> torch.Tensor:
    """``dequantize_sum_grouped`` in the rotated domain, in one launch (1 to 16 terms; more raise): the terms are records made by
    ``quantize_grouped_rotated`` or ``reduce_quantize_grouped_rotated`` with the same ``seed``; they are summed in float32 (the first stored, the
    others added in order) and only the sum is rotated back.  ``'set'`` stores it converted to ``dtype`` and never reads ``out``; ``'add'`` adds it
    into ``out=`` with one float32 add and one rounding.  One term is ``dequantize_grouped_rotated``.  Returns ``out``
    (``include/piquant_hip.h``, piquant_hip_dequantize_sum_grouped_rotated)."""
    seed = _check_seed(seed)
    return _dequantize_sum_grouped(tensors, scales, zero_points, dtype, group_size, reduce_op, ctx, out, quant_dtype, shape, seed)


def _dequantize_sum_grouped(tensors, scales, zero_points, dtype, group_size, reduce_op, ctx, out, quant_dtype, shape, seed=None):
    """``dequantize_sum_grouped`` and, with a ``seed``, ``dequantize_sum_grouped_rotated``, which takes at most 16 terms."""
    _check_modes(float_dtype=dtype, reduce_op=reduce_op, group_size=group_size)
    tensors, scales, zero_points = list(tensors), list(scales), list(zero_points)
    _require(len(tensors) > 0, 'dequantize_sum_grouped needs at least one term')
    _require(seed is None or len(tensors) <= 16, f'dequantize_sum_grouped_rotated takes at most 16 terms, got {len(tensors)}')
    _require(len(tensors) == len(scales) == len(zero_points), f'tensors, scales and zero_points must have the same length, got '
             f'{len(tensors)}, {len(scales)} and {len(zero_points)}')
    _require(out is not None or reduce_op != 'add', "reduce_op='add' accumulates into out=; pass the accumulator tensor")
    first = tensors[0]
    _require(isinstance(first, torch.Tensor) and (first.dtype in _QUANT_TYPES or quant_dtype is not None), 'tensors[0] must be a quantized tensor')
    dtype_in, logical_shape = _quant_meta(first, quant_dtype, shape)
    numel = _numel_of(logical_shape)
    _require(first.is_cuda, 'dequantize_sum_grouped needs ROCm device tensors')
    _check_grouped_terms(tensors, scales, zero_points, dtype_in, repeat(numel), group_size, first.device)
    out = _float_out(out, reduce_op, dtype, logical_shape, numel, first.device)
    ctx = _ctx_for(first, ctx)
    if seed is not None:
        ctx.dequantize_sum_grouped_rotated_ptr(_ptrs(tensors), dtype_in, _ptrs(scales), _ptrs(zero_points), out.data_ptr(),
                                               torch_to_piquant_dtype(out.dtype), numel, group_size, seed, _REDUCE_OPS[reduce_op], _device_ptrs=True)
        return out
    ctx.dequantize_sum_grouped_ptr(_ptrs(tensors), dtype_in, _ptrs(scales), _ptrs(zero_points), out.data_ptr(), torch_to_piquant_dtype(out.dtype), numel,
                                   group_size, _REDUCE_OPS[reduce_op], _device_ptrs=True)
    return out


def dequantize_sum(tensors, params, *, dtype: torch.dtype, reduce_op: str = 'set', ctx: Optional[Context] = None,
                   out: Optional[torch.Tensor] = None, quant_dtype: Optional[torch.dtype] = None, shape=None) -> torch.Tensor:
    """out (op)= sum_i dequantize(tensors[i]) with (scale, zero_point) of input i read from the device record ``params[i]``: one pass
    over the accumulator instead of ``len(tensors)``; the result equals ``dequantize_dynamic`` applied in order (first with
    ``reduce_op``, the rest with 'add') bit for bit.  The reduction step of ``piquant.distributed.quantized_all_reduce``."""
    _check_modes(float_dtype=dtype)
    _require(len(tensors) == len(params) and len(tensors) > 0, 'dequantize_sum needs as many parameter records as tensors, and at least one')
    first = tensors[0]
    _require(isinstance(first, torch.Tensor) and first.is_cuda, 'dequantize_sum needs ROCm device tensors')
    dtype_in, logical_shape = _quant_meta(first, quant_dtype, shape)
    numel = _numel_of(logical_shape)
    _check_dynamic_terms(tensors, params, dtype_in, repeat(numel), first.device)
    out = _float_out(out, reduce_op, dtype, logical_shape, numel, first.device)
    ctx = _ctx_for(first, ctx)
    ctx.dequantize_sum_ptr(_ptrs(tensors), _ptrs(params), dtype_in, out.data_ptr(), torch_to_piquant_dtype(out.dtype), numel, _REDUCE_OPS[reduce_op],
                           _device_ptrs=True)
    return out


def quantize_dynamic_batch(tensors, *, dtype: torch.dtype, round_mode: str = 'nearest', ctx: Optional[Context] = None, outs=None, params=None):
    """``quantize_dynamic`` for a list of independent tensors of one float dtype: each gets its own (scale, zero_point) and record,
    up to 16 of them are processed by ONE kernel launch.  Returns (list of quantized tensors, list of parameter records)."""
    _check_modes(quant_dtype=dtype)
    _require(len(tensors) > 0, 'quantize_dynamic_batch needs at least one tensor')
    fdt = tensors[0].dtype
    for i, t in enumerate(tensors):
        _check_float_input(t, f'tensors[{i}]')
        _require(t.dtype == fdt and t.device == tensors[0].device, 'all tensors of a batch share one float dtype and one device')
    tensors = _contiguous(tensors)
    if outs is None:
        outs = [torch.empty(t.shape, dtype=dtype, device=t.device) for t in tensors]
    if params is None:
        block = torch.empty(len(tensors) * PARAMS_NBYTES, dtype=torch.uint8, device=tensors[0].device)
        params = [block[i * PARAMS_NBYTES: (i + 1) * PARAMS_NBYTES] for i in range(len(tensors))]
    _require(len(outs) == len(params) == len(tensors), 'outs= and params= must have one entry per tensor')
    qdt = torch_to_piquant_dtype(dtype)
    for i, (t, o, p) in enumerate(zip(tensors, outs, params)):
        _check_packed_out(o, qdt, t.numel(), t.device, f'outs[{i}]')
        _check_params(p, t.device, f'params[{i}]')
    ctx = _ctx_for(tensors[0], ctx)
    ctx.quantize_dynamic_batch_ptr(_ptrs(tensors), torch_to_piquant_dtype(fdt), _ptrs(outs), qdt, [t.numel() for t in tensors], _ptrs(params), _ROUND_MODES[round_mode],
                                   _device_ptrs=True)
    return outs, params


def dequantize_dynamic_batch(tensors, params, *, dtype: torch.dtype, reduce_op: str = 'set', ctx: Optional[Context] = None, outs=None,
                             quant_dtype: Optional[torch.dtype] = None, shapes=None):
    """``dequantize_dynamic`` for a list of independent quantized tensors (raw uint8 buffers with ``quant_dtype=`` and ``shapes=``, or
    quantized torch tensors) in one launch per 16; ``outs`` are required for ``reduce_op='add'``."""
    _check_modes(float_dtype=dtype)
    _require(len(tensors) == len(params) and len(tensors) > 0, 'dequantize_dynamic_batch needs as many parameter records as tensors, and at least one')
    _require(all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors), 'dequantize_dynamic_batch needs ROCm device tensors')
    metas = [_quant_meta(t, quant_dtype, None if shapes is None else shapes[i]) for i, t in enumerate(tensors)]
    dtype_in = metas[0][0]
    _require(all(m[0] == dtype_in for m in metas), 'all tensors of a batch share one quantized dtype')
    numels = [_numel_of(shp) for _dt, shp in metas]
    device = tensors[0].device
    _check_dynamic_terms(tensors, params, dtype_in, numels, device)
    _require(outs is None or len(outs) == len(tensors), 'outs= must have one entry per tensor')
    outs = _float_outs(outs, reduce_op, dtype, [shape for _, shape in metas], numels, device)
    ctx = _ctx_for(tensors[0], ctx)
    ctx.dequantize_dp_batch_ptr(_ptrs(tensors), dtype_in, _ptrs(outs), torch_to_piquant_dtype(dtype), numels, _ptrs(params), _REDUCE_OPS[reduce_op],
                                _device_ptrs=True)
    return outs


def reduce_quantize_dynamic(acc: torch.Tensor, tensors, params, *, dtype: torch.dtype, round_mode: str = 'nearest', ctx: Optional[Context] = None,
                            out: Optional[torch.Tensor] = None, out_params: Optional[torch.Tensor] = None):
    """(quantize(acc + sum_i dequantize(tensors[i])), record): the owner's step of a mesh all-reduce as one call -- one kernel launch
    that never writes the sum to memory when it stays on chip.  ``tensors`` are raw uint8 buffers of packed ``dtype`` values with
    ``acc.numel()`` elements each, ``params`` their device records.  The contents of ``acc`` afterwards are unspecified."""
    _check_modes(quant_dtype=dtype)
    _check_float_input(acc, 'acc')
    _require(acc.is_contiguous(), 'acc must be contiguous')
    _require(len(tensors) == len(params), 'reduce_quantize_dynamic needs as many parameter records as tensors')
    qdt = torch_to_piquant_dtype(dtype)
    _check_dynamic_terms(tensors, params, qdt, repeat(acc.numel()), acc.device)
    out = _packed_out(out, dtype, acc, acc.device)
    if out_params is None:
        out_params = torch.empty(PARAMS_NBYTES, dtype=torch.uint8, device=acc.device)
    _check_params(out_params, acc.device, 'out_params')
    ctx = _ctx_for(acc, ctx)
    ctx.reduce_quantize_dynamic_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), _ptrs(tensors), _ptrs(params), out.data_ptr(), qdt, acc.numel(),
                                    out_params.data_ptr(), _ROUND_MODES[round_mode], _device_ptrs=True)
    return out, out_params
