"""Multi-GPU use of the path: one process per GPU, ``torch.distributed`` (backend ``nccl`` == RCCL over xGMI).

The reference is a single-process CPU library; its only "parallelism" is a static split of one flat array
over pool threads (``src/piquant.cpp:132-176``).  Here the same split rule shards a tensor over ranks:

* ``quantize`` / ``dequantize`` are element-local -> every rank processes its own shard, **no collective**;
* ``compute_quant_params`` needs the global min/max -> each rank scans its shard on its GPU into two int32
  keys {key(min), key(-max)}; **one** 8-byte ``all_reduce(MIN)`` combines them; every rank then runs the same
  double-precision epilogue and obtains identical ``(scale, zero_point)``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
import torch.distributed as dist

from . import Context, DataType, decode_minmax_keys, quant_params_from_minmax
from .torch import _QUANT_TYPES, _REDUCE_OPS, _ROUND_MODES, _ctx_for, _residual_dtype, torch_to_piquant_dtype


_P2P_MAX_TIMEOUT_S = 4294.0   # the C ABI carries microseconds in 32 bits


def _p2p_timeout_us(timeout: Optional[float]) -> int:
    """``timeout`` (seconds) of the peer-to-peer transports as the C ABI's microseconds.  None: ``PIQUANT_P2P_TIMEOUT_S`` from the environment,
    else the library's default (0 -> 10 minutes, what torch.distributed gives a collective before it calls a rank missing).  A rank may be
    minutes late for honest reasons -- a checkpoint write, an evaluation pass on rank 0, a first-call compile."""
    import os

    if timeout is None:
        env = os.environ.get('PIQUANT_P2P_TIMEOUT_S')
        if not env:
            return 0
        timeout = float(env)
    if not 0.0 < timeout <= _P2P_MAX_TIMEOUT_S:
        raise ValueError(f'timeout={timeout} s is outside (0, {_P2P_MAX_TIMEOUT_S:.0f}] s')
    return max(1, int(timeout * 1e6))


def _raise_peer_timeout(ctx: Context, what: str) -> None:
    """RuntimeError if a peer-to-peer wait of ``ctx`` ran out since the last look (the GPU queue is NOT faulted by such a wait: the kernel reports
    and the stream goes on, ``piquant_hip_peer_timeout``)."""
    t = ctx.peer_timeout()
    if t is None:
        return
    kind, rank, expected, seen = t
    # The buffers of the exchange that gave up are void from here on: the rank that was waited for may still store into them (its chunk into a receive
    # buffer of a LATER exchange's parity, its key pair into a mailbox slot nobody empties), and this rank signalled nothing behind the wait that ran out
    # (signal_flags_kernel), so its peers are about to give up on it in turn.  Every mesh of that kind on the device is poisoned until the group
    # rebuilds them (release_peer_meshes, a collective).
    for m in list((_PeerMesh if kind == 'flags' else _KeyMesh)._cache.values()):
        if m.device.index == ctx.device:
            m.poisoned = True
    if kind == 'flags':
        raise RuntimeError(f"{what}: rank {rank} did not arrive within the timeout (its flag read {seen}, exchange {expected} was waited for); the tensors of that "
                           f"all-reduce hold stale bytes.  Raise timeout= / PIQUANT_P2P_TIMEOUT_S if ranks may be that far apart.")
    raise RuntimeError(f"{what}: rank {rank} did not deliver its min/max keys within the timeout; the parameters of that call are void.  "
                       f"Raise timeout= / PIQUANT_P2P_TIMEOUT_S if ranks may be that far apart.")


class _StreamOrder:
    """The buffers and sequence numbers of a cached mesh are ONE resource: its two-parity argument ("a rank enters exchange s + 1 only behind its own
    decode of s") holds for exchanges issued in stream order.  Exchanges from different streams (a comm side stream, a DDP hook, two threads) are put
    in that order here: an event behind every exchange, waited for by the next one when it comes from another stream."""

    def __init__(self):
        import threading

        self._last_stream = None
        self._event = None
        self.lock = threading.Lock()      # the host side of an exchange (sequence number, parity, the launches) is one critical section per mesh

    def enter(self, device: torch.device) -> None:
        cur = torch.cuda.current_stream(device)
        if self._last_stream is not None and self._last_stream != cur.cuda_stream:
            cur.wait_event(self._event)

    def leave(self, device: torch.device) -> None:
        cur = torch.cuda.current_stream(device)
        if self._event is None:
            self._event = torch.cuda.Event()
        self._event.record(cur)
        self._last_stream = cur.cuda_stream


def shard_range(numel: int, rank: int, world_size: int, packed_bits: int = 8, align: int = 1) -> Tuple[int, int]:
    """[begin, end) of ``rank``'s shard: the reference's range split (``src/piquant.cpp:145-157``) -- boundaries are
    aligned down to a whole packed byte (2 elements for uint4, 4 for uint2); the last rank keeps the ragged end.
    ``align`` (1 = the reference rule only; otherwise a multiple of the pack factor, e.g. 4096) aligns interior boundaries down further, so that every shard of ONE
    shared allocation also starts on a 16-byte vector of both the float and the packed side."""
    world_size = max(1, world_size)
    pack = 8 // packed_bits if packed_bits < 8 else 1
    if align < 1 or (align != 1 and align % pack != 0):
        raise ValueError(f'align={align} must be 1 (whole packed bytes only) or a multiple of the pack factor {pack}')
    unit = max(pack, align)
    begin = numel * rank // world_size
    end = numel * (rank + 1) // world_size
    if unit > 1:
        begin -= begin % unit
        if rank + 1 != world_size:
            end -= end % unit
    return begin, max(begin, end)


def _rank_world(rank: Optional[int], world_size: Optional[int], group) -> Tuple[int, int]:
    if rank is None or world_size is None:
        if not (dist.is_available() and dist.is_initialized()):
            raise ValueError('rank= and world_size= are required when torch.distributed is not initialised')
        rank = dist.get_rank(group) if rank is None else rank
        world_size = dist.get_world_size(group) if world_size is None else world_size
    if not 0 <= rank < world_size:
        raise ValueError(f'rank {rank} is outside [0, {world_size})')
    return rank, world_size


def quantize_shard(
    tensor: torch.Tensor,
    *,
    scale: float,
    zero_point: int,
    dtype: torch.dtype,
    round_mode: str = 'nearest',
    out: Optional[torch.Tensor] = None,
    rank: Optional[int] = None,
    world_size: Optional[int] = None,
    group: Optional[dist.ProcessGroup] = None,
    align: int = 1,
    ctx: Optional[Context] = None,
    _quantize=None,
) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """This rank's share of ``quantize(tensor)`` for ONE logical tensor that every rank holds (or addresses): elements
    ``shard_range(numel, rank, world)`` -- the reference's pool split (``src/piquant.cpp:145-157``) with ranks in place of
    threads -- are quantized with the caller's (global) ``scale`` / ``zero_point``; no collective.

    Returns ``(packed bytes of the shard, (begin, end))``.  With ``out=`` (a contiguous quantized tensor or raw uint8 buffer
    for the WHOLE tensor) the bytes are written in place at ``begin * bits / 8`` and the returned tensor is that slice, so
    the concatenation over ranks is byte for byte what a single ``quantize`` call produces (the kernels are
    position-independent; tested)."""
    from .torch import packed_bytes, quantize

    if dtype not in _QUANT_TYPES:
        raise ValueError(f'{dtype} is not a quantized dtype')
    if not tensor.is_contiguous():
        raise ValueError('quantize_shard needs a contiguous tensor: a shard is a range of the flat element order')
    qdt = torch_to_piquant_dtype(dtype)
    rank, world_size = _rank_world(rank, world_size, group)
    flat = tensor.view(-1)
    begin, end = shard_range(flat.numel(), rank, world_size, qdt.bit_size, align)
    n_bytes = qdt.packed_nbytes(end - begin)
    first = begin * qdt.bit_size // 8
    if out is None:
        dst = torch.empty(n_bytes, dtype=torch.uint8, device=tensor.device)
    else:
        whole = out if out.dtype == torch.uint8 else packed_bytes(out)
        if whole.device != tensor.device or not whole.is_contiguous() or whole.numel() < qdt.packed_nbytes(flat.numel()):
            raise ValueError(f'out= must be a contiguous buffer on {tensor.device} holding the whole quantized tensor '
                             f'({qdt.packed_nbytes(flat.numel())} bytes)')
        dst = whole.view(-1)[first: first + n_bytes]
    if end > begin:
        (_quantize or quantize)(flat[begin:end], scale=scale, zero_point=zero_point, dtype=dtype,
                                round_mode=round_mode, ctx=ctx, out=dst, uniform=True)
    return dst, (begin, end)


def dequantize_shard(
    packed: torch.Tensor,
    *,
    numel: int,
    scale: float,
    zero_point: int,
    quant_dtype: torch.dtype,
    out: torch.Tensor,
    reduce_op: str = 'set',
    rank: Optional[int] = None,
    world_size: Optional[int] = None,
    group: Optional[dist.ProcessGroup] = None,
    align: int = 1,
    ctx: Optional[Context] = None,
    _dequantize=None,
) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """This rank's share of ``dequantize``: ``packed`` holds the WHOLE quantized tensor of ``numel`` elements (a quantized
    torch tensor or its raw uint8 bytes), ``out`` the whole float tensor; elements ``shard_range(numel, rank, world)`` of
    ``out`` are set (or accumulated into, ``reduce_op='add'``).  Returns ``(out[begin:end] view, (begin, end))``."""
    from .torch import dequantize, packed_bytes

    if quant_dtype not in _QUANT_TYPES:
        raise ValueError(f'{quant_dtype} is not a quantized dtype')
    qdt = torch_to_piquant_dtype(quant_dtype)
    raw = packed if packed.dtype == torch.uint8 else packed_bytes(packed)
    if not raw.is_contiguous() or raw.numel() < qdt.packed_nbytes(numel):
        raise ValueError(f'packed must be contiguous and hold {qdt.packed_nbytes(numel)} bytes for {numel} elements')
    if not out.is_contiguous() or out.numel() != numel or out.device != raw.device:
        raise ValueError('out= must be the contiguous float tensor of the whole logical tensor, on the same device')
    rank, world_size = _rank_world(rank, world_size, group)
    begin, end = shard_range(numel, rank, world_size, qdt.bit_size, align)
    dst = out.view(-1)[begin:end]
    if end > begin:
        first = begin * qdt.bit_size // 8
        src = raw.view(-1)[first: first + qdt.packed_nbytes(end - begin)]
        (_dequantize or dequantize)(src, scale=scale, zero_point=zero_point, dtype=out.dtype, reduce_op=reduce_op, ctx=ctx, out=dst,
                                    quant_dtype=quant_dtype, shape=(end - begin,), uniform=True)
    return dst, (begin, end)


def local_minmax_keys(tensor: torch.Tensor, ctx: Optional[Context] = None) -> torch.Tensor:
    """int32[2] tensor on ``tensor.device`` holding {key(min), key(-max)} of the local shard (HIP scan, async)."""
    if not tensor.is_cuda:
        raise RuntimeError('local_minmax_keys needs a ROCm device tensor: the min/max scan is a HIP kernel, there is no CPU path')
    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    ctx = _ctx_for(tensor, ctx)
    keys = torch.empty(2, dtype=torch.int32, device=tensor.device)
    ctx.minmax_keys_ptr(tensor.data_ptr(), torch_to_piquant_dtype(tensor.dtype), tensor.numel(), keys.data_ptr(), init=True, _device_ptrs=True)
    return keys


def compute_quant_params(
    local_shard: torch.Tensor,
    *,
    dtype: torch.dtype,
    group: Optional[dist.ProcessGroup] = None,
    ctx: Optional[Context] = None,
    transport: str = 'collective',
    timeout: Optional[float] = None,
    _scan=local_minmax_keys,
) -> Tuple[float, int]:
    """Quantization parameters of the tensor whose shards are spread over ``group`` (identical on every rank).

    ``transport='collective'``: the local keys, ONE 8-byte ``all_reduce(MIN)`` (RCCL over xGMI), the epilogue.  ``transport='p2p'`` (GPUs of
    one node): the same MIN over peer-mapped mailboxes by one one-wave kernel behind the scan -- a store to and a poll for every peer instead
    of a collective's launch and protocol (``piquant_hip_exchange_minmax_keys``); same keys, hence the same parameters.  At most 64 ranks.
    ``timeout`` (seconds, p2p only; default ``PIQUANT_P2P_TIMEOUT_S`` or 10 minutes): how long a rank waits for its peers before the call raises
    RuntimeError naming the missing rank."""
    if dtype not in _QUANT_TYPES:
        raise ValueError(f'{dtype} is not a quantized dtype')
    if transport not in ('collective', 'p2p'):
        raise ValueError(f"transport must be 'collective' or 'p2p', got {transport!r}")
    keys = _scan(local_shard, ctx)
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world > 1 and transport == 'p2p':
        if world > _KEY_MESH_MAX_RANKS:
            raise ValueError(f"transport='p2p' exchanges the keys in one wave: at most {_KEY_MESH_MAX_RANKS} ranks, the group has {world}")
        if not keys.is_cuda:
            raise RuntimeError("transport='p2p' exchanges device memory between GPUs: the shard must live on one")
        cx = _ctx_for(local_shard, ctx)
        mesh = _KeyMesh.get(group, keys.device, world, dist.get_rank(group))
        keys = mesh.exchange(keys, cx, _p2p_timeout_us(timeout))
        k = keys.cpu()                    # synchronises: the exchange is over, one way or the other
        try:
            _raise_peer_timeout(cx, "compute_quant_params(transport='p2p')")
        except RuntimeError:
            mesh.poisoned = True          # the late rank's word will land in a slot nobody empties any more
            raise
    elif world > 1:
        dist.all_reduce(keys, op=dist.ReduceOp.MIN, group=group)   # the path's only collective: 8 bytes
    k = keys.cpu()
    r_min, r_max = decode_minmax_keys(int(k[0]), int(k[1]))
    return quant_params_from_minmax(r_min, r_max, torch_to_piquant_dtype(dtype))


def compute_quant_params_clipped(
    local_shard: torch.Tensor,
    *,
    dtype: torch.dtype,
    steps: int = 63,
    group: Optional[dist.ProcessGroup] = None,
    ctx: Optional[Context] = None,
) -> Tuple[float, int]:
    """``piquant.torch.compute_quant_params_clipped`` of the tensor whose shards are spread over ``group``: the local keys, the 8-byte
    ``all_reduce(MIN)``, the local histogram against the GLOBAL keys, one ``all_reduce(SUM)`` of the int64[8192] counts, the search.  Counts are
    integers, so the result is identical on every rank and identical to the single-GPU call on the whole tensor.  Collective transport only."""
    from .torch import _check_clip_params_steps, _check_float_input, clip_histogram, params_to_host, quant_params_from_histogram

    if dtype not in _QUANT_TYPES:
        raise ValueError(f'{dtype} is not a quantized dtype')
    _check_clip_params_steps(steps)
    _check_float_input(local_shard, 'local_shard (the tensor)')   # before the first launch and the first collective: a bad rank enters neither
    keys = local_minmax_keys(local_shard, ctx)
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world > 1:
        dist.all_reduce(keys, op=dist.ReduceOp.MIN, group=group)
    hist = clip_histogram(local_shard, keys, ctx=ctx)
    if world > 1:
        dist.all_reduce(hist, op=dist.ReduceOp.SUM, group=group)
    return params_to_host(quant_params_from_histogram(keys, hist, dtype=dtype, steps=steps, ctx=ctx))


def _device_identity(index: int) -> str:
    props = torch.cuda.get_device_properties(index)
    uuid = getattr(props, 'uuid', None)
    return str(uuid) if uuid is not None else f'{props.name}#{index}'


def _check_peers_reachable(group, device: torch.device, world: int, rank: int) -> None:
    """Collective.  Before anything is mapped: every rank must sit on the same host, and every GPU of the group must be able to address every other
    one (``hipDeviceCanAccessPeer``).  If a pair cannot, EVERY rank raises the same RuntimeError naming the pairs -- a refusal before the first
    IPC handle is opened instead of a fault inside a kernel.  (``PIQUANT_P2P_PRETEND_UNREACHABLE="i-j"`` declares a pair of ranks unreachable:
    the refusal can be tested on a box where everything is reachable.)  A peer's GPU that this process cannot see at all (per-rank
    HIP_VISIBLE_DEVICES) cannot be asked about; the mapping itself then decides."""
    import os
    import socket

    me = (socket.gethostname(), _device_identity(device.index))
    everyone = [None] * world
    dist.all_gather_object(everyone, me, group=group)
    hosts = {h for h, _ in everyone}
    if len(hosts) > 1:
        raise RuntimeError(f"transport='p2p' maps device memory between the GPUs of ONE node; the group spans {sorted(hosts)}")
    visible = {_device_identity(i): i for i in range(torch.cuda.device_count())}
    pretend = set()
    for pair in filter(None, os.environ.get('PIQUANT_P2P_PRETEND_UNREACHABLE', '').split(',')):
        a, b = (int(v) for v in pair.split('-'))
        pretend.add((min(a, b), max(a, b)))
    mine = []
    for j, (_, ident) in enumerate(everyone):
        if j == rank:
            continue
        if (min(rank, j), max(rank, j)) in pretend:
            mine.append((rank, j))
        elif ident != me[1] and ident in visible and not torch.cuda.can_device_access_peer(device.index, visible[ident]):
            mine.append((rank, j))
    unreachable = [None] * world
    dist.all_gather_object(unreachable, mine, group=group)
    pairs = sorted({(min(a, b), max(a, b)) for per_rank in unreachable for a, b in per_rank})
    if pairs:
        raise RuntimeError(f"transport='p2p' refused: the GPUs of ranks {pairs} cannot address each other's memory (hipDeviceCanAccessPeer); "
                           f"use transport='collective'")


class _PeerMapped:
    """One allocation per rank that every other rank of the group maps into its own address space (HIP IPC through the library's
    ``piquant_hip_peer_*`` calls; the 64-byte handles travel over the process group).  ``ptrs[j]`` is the local address of rank j's
    allocation (``ptrs[rank]`` the own one).  On one node every GPU reaches every other over its own xGMI link; several processes on one GPU
    -- the tests -- share memory the same way."""

    def __init__(self, ctx: Context, group, nbytes: int, world: int, rank: int, fine_grained: bool, fill_word: int = 0):
        self.ctx, self.rank = ctx, rank
        self.own, handle = ctx.peer_alloc(nbytes, fine_grained, fill_word)
        handles = [None] * world
        dist.all_gather_object(handles, handle, group=group)
        self.ptrs = [self.own if j == rank else ctx.peer_open(h) for j, h in enumerate(handles)]

    def release(self, group) -> None:
        """Collective: everybody unmaps before anybody frees."""
        dist.barrier(group=group)
        for j, p in enumerate(self.ptrs):
            if j != self.rank:
                self.ctx.peer_close(p)
        self.ptrs = []
        dist.barrier(group=group)
        self.ctx.peer_free(self.own)
        self.own = 0

    def discard(self) -> None:
        """NOT collective: the peers are gone (their process group was destroyed); unmap what was mapped, free what was allocated."""
        torch.cuda.synchronize()
        for j, p in enumerate(self.ptrs):
            if j != self.rank:
                self.ctx.peer_close(p)
        self.ptrs = []
        if self.own:
            self.ctx.peer_free(self.own)
            self.own = 0


_KEY_MESH_MAX_RANKS = 64   # include/piquant_hip.h, piquant_hip_exchange_minmax_keys: one lane per rank


class _KeyMesh:
    """Mailboxes of ``compute_quant_params(transport='p2p')``: per rank two arrays (parities) of ``world`` 8-byte words in FINE-GRAINED device
    memory (another GPU writes them while a kernel of this one polls).  Word j of rank r's mailbox is where rank j stores its key pair for r;
    a word is emptied by its reader; exchanges alternate between the parities (``include/piquant_hip.h``)."""

    _cache = {}

    def __init__(self, group, device: torch.device, world: int, rank: int):
        self.world, self.rank, self.device = world, rank, device
        self.ctx = Context.get(device.index)
        _check_peers_reachable(group, device, world, rank)
        self.mem = _PeerMapped(self.ctx, group, 16 * world, world, rank, fine_grained=True, fill_word=0x7fffffff)   # every word = two keys of NaN patterns: empty
        self.out = torch.empty(2, dtype=torch.int32, device=device)
        torch.cuda.synchronize(device)
        dist.barrier(group=group)
        self.seq = 0
        self.order = _StreamOrder()
        self.poisoned = False            # an exchange of this mesh gave up: a late word may sit in a mailbox slot for ever

    @classmethod
    def get(cls, group, device, world, rank):
        owner = group if group is not None else dist.group.WORLD
        key = (id(owner), device.index, world)
        m = cls._cache.get(key)
        if m is not None and m.owner is not owner:      # an id recycled by a later process group: those peers are gone
            cls._cache.pop(key).mem.discard()
            m = None
        if m is None:
            m = cls._cache[key] = cls(group, device, world, rank)
            m.owner = owner
        return m

    def exchange(self, keys: torch.Tensor, ctx: Context, timeout_us: int = 0) -> torch.Tensor:
        if self.poisoned:
            raise RuntimeError("compute_quant_params(transport='p2p'): an earlier exchange of this group gave up on a late rank, whose keys may still sit in a "
                               "mailbox; every rank must call piquant.distributed.release_peer_meshes(group) before the group uses transport='p2p' again")
        _raise_peer_timeout(ctx, "an earlier compute_quant_params(transport='p2p')")
        with self.order.lock:
            self.order.enter(self.device)
            self.seq += 1
            par = self.seq & 1
            slots = [self.mem.ptrs[j] + 8 * (par * self.world + self.rank) for j in range(self.world)]
            ctx.exchange_minmax_keys_ptr(keys.data_ptr(), slots, self.mem.own + 8 * par * self.world, self.out.data_ptr(), timeout_us)
            self.order.leave(self.device)
        return self.out

    def release(self, group) -> None:
        torch.cuda.synchronize(self.device)
        self.mem.release(group)


# -----------------------------------------------------------------------------------------------------------------
# Quantized ring all-reduce: the caller pattern the reference's SET/ADD store operators were
# designed for ("useful for ring-reduction operations", reference README.md:29), built from the path's primitives.
# -----------------------------------------------------------------------------------------------------------------
_HEADER_BYTES = 16   # wire header per hop == the device parameter record {float scale, float 1/scale, int64 zero_point}


class GroupedWireLayout(NamedTuple):
    """One chunk's record on the grouped wire: ``float32 scales[ngroups] | uint8 zero_points[ngroups] | pad to 16 | packed bytes``."""
    ngroups: int
    zero_points_offset: int
    data_offset: int         # 16-byte aligned: the packed bytes start on a vector boundary of the kernels
    nbytes: int              # the whole record (scales, zero points, padding, packed bytes)


def grouped_wire_layout(numel: int, group_size: int, packed_bits: int) -> GroupedWireLayout:
    """Layout of the grouped wire record of a chunk of ``numel`` elements (``quantized_all_reduce(group_size=...)``): ngroups = ceil(numel /
    group_size) float32 scales, then as many uint8 zero points, zero padding up to a multiple of 16 bytes, then the packed bytes (``packed_bits``
    per element, whole bytes).  The record of an empty chunk is empty."""
    ngroups = -(-int(numel) // int(group_size))
    zp = 4 * ngroups
    data = -(-(zp + ngroups) // 16) * 16
    return GroupedWireLayout(ngroups, zp, data, data + -(-int(numel) * int(packed_bits) // 8))


class _DeviceOps:
    """Wire encode / decode on ROCm device tensors (HIP kernels through libpiquant.so).  The parameters are derived on
    the device straight into the buffer's header and read back from it by the receiver's dequantize kernel: a hop
    needs no host synchronisation at all.

    The calls go through the context's raw-pointer entry points (round 5): every buffer here is one this module laid out itself (16-byte header +
    packed bytes, slots on 16-byte boundaries), and the tensor-level wrappers of ``piquant.torch`` -- two slices and a dozen attribute checks per
    buffer -- cost 17 us of host time for a one-term ``reduce_encode`` and 42 us for a seven-term one, more than the kernels they launch
    (profiles/EXPERIMENTS.md): an all-reduce of 109 MB was bound by its host."""

    def __init__(self, ctx: Optional[Context]):
        self.ctx = ctx

    def _cx(self, t: torch.Tensor) -> Context:
        if not t.is_cuda:
            raise RuntimeError('the wire kernels are HIP kernels: quantized_all_reduce needs ROCm device tensors (there is no CPU path)')
        return _ctx_for(t, self.ctx)    # the tensor's device, PyTorch's current stream, stream-ordered

    @staticmethod
    def _mode(round_mode: str):
        """``quantized_all_reduce`` hands its ``round_mode=`` down unchecked: as ever, whatever is not 'nearest' rounds stochastically."""
        return _ROUND_MODES['nearest' if round_mode == 'nearest' else 'stochastic']

    def encode(self, x: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str) -> None:
        p = buf.data_ptr()
        self._cx(x).quantize_dynamic_ptr(x.data_ptr(), torch_to_piquant_dtype(x.dtype), p + _HEADER_BYTES, torch_to_piquant_dtype(qdtype), x.numel(), p,
                                         self._mode(round_mode), _device_ptrs=True)

    def decode(self, buf: torch.Tensor, out: torch.Tensor, qdtype: torch.dtype, reduce_op: str) -> None:
        p = buf.data_ptr()
        self._cx(out).dequantize_dp_ptr(p + _HEADER_BYTES, torch_to_piquant_dtype(qdtype), out.data_ptr(), torch_to_piquant_dtype(out.dtype), out.numel(), p,
                                        _REDUCE_OPS[reduce_op], _device_ptrs=True)

    def encode_batch(self, xs, bufs, qdtype: torch.dtype, round_mode: str) -> None:
        """encode(xs[i], bufs[i]) for all i with one kernel launch per 16 chunks (each chunk its own parameters)."""
        if xs:
            ps = [b.data_ptr() for b in bufs]
            self._cx(xs[0]).quantize_dynamic_batch_ptr([x.data_ptr() for x in xs], torch_to_piquant_dtype(xs[0].dtype), [p + _HEADER_BYTES for p in ps],
                                                       torch_to_piquant_dtype(qdtype), [x.numel() for x in xs], ps, self._mode(round_mode), _device_ptrs=True)

    def decode_batch(self, bufs, outs, qdtype: torch.dtype, reduce_op: str) -> None:
        """decode(bufs[i], outs[i]) for all i with one kernel launch per 16 chunks."""
        if bufs:
            ps = [b.data_ptr() for b in bufs]
            self._cx(outs[0]).dequantize_dp_batch_ptr([p + _HEADER_BYTES for p in ps], torch_to_piquant_dtype(qdtype), [o.data_ptr() for o in outs],
                                                      torch_to_piquant_dtype(outs[0].dtype), [o.numel() for o in outs], ps,
                                                      _REDUCE_OPS[reduce_op], _device_ptrs=True)

    def reduce_encode(self, bufs, acc: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str) -> None:
        """encode(acc + sum of the wire buffers) into ``buf`` as one call (``acc`` is scratch afterwards)."""
        ps = [b.data_ptr() for b in bufs]
        p = buf.data_ptr()
        self._cx(acc).reduce_quantize_dynamic_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), [q + _HEADER_BYTES for q in ps], ps, p + _HEADER_BYTES,
                                                  torch_to_piquant_dtype(qdtype), acc.numel(), p, self._mode(round_mode), _device_ptrs=True)

    def decode_sum(self, bufs, out: torch.Tensor, qdtype: torch.dtype) -> None:
        """out += sum of the wire buffers, one pass over ``out`` (same result as decode(..., 'add') buffer by buffer)."""
        ps = [b.data_ptr() for b in bufs]
        self._cx(out).dequantize_sum_ptr([p + _HEADER_BYTES for p in ps], ps, torch_to_piquant_dtype(qdtype), out.data_ptr(), torch_to_piquant_dtype(out.dtype),
                                         out.numel(), _REDUCE_OPS['add'], _device_ptrs=True)

    # ---- the grouped wire (grouped_wire_layout): per-group parameters in front of the packed bytes ----
    @staticmethod
    def _record(buf: torch.Tensor, numel: int, qdtype: torch.dtype, group_size: int):
        """(scales, zero points, packed bytes) addresses of the grouped record in ``buf``"""
        lay = grouped_wire_layout(numel, group_size, torch_to_piquant_dtype(qdtype).bit_size)
        p = buf.data_ptr()
        return p, p + lay.zero_points_offset, p + lay.data_offset

    def encode_grouped(self, x: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int) -> None:
        sc, zp, data = self._record(buf, x.numel(), qdtype, group_size)
        self._cx(x).quantize_grouped_ptr(x.data_ptr(), torch_to_piquant_dtype(x.dtype), data, torch_to_piquant_dtype(qdtype), x.numel(), group_size, sc, zp,
                                         False, self._mode(round_mode), _device_ptrs=True)

    def decode_grouped(self, buf: torch.Tensor, out: torch.Tensor, qdtype: torch.dtype, reduce_op: str, group_size: int) -> None:
        sc, zp, data = self._record(buf, out.numel(), qdtype, group_size)
        self._cx(out).dequantize_grouped_ptr(data, torch_to_piquant_dtype(qdtype), out.data_ptr(), torch_to_piquant_dtype(out.dtype), out.numel(), group_size,
                                             sc, zp, _REDUCE_OPS[reduce_op], _device_ptrs=True)

    def encode_batch_grouped(self, xs, bufs, qdtype: torch.dtype, round_mode: str, group_size: int) -> None:
        """encode_grouped(xs[i], bufs[i]) for all i with one kernel launch per 16 chunks."""
        if xs:
            recs = [self._record(b, x.numel(), qdtype, group_size) for x, b in zip(xs, bufs)]
            self._cx(xs[0]).quantize_grouped_batch_ptr([x.data_ptr() for x in xs], torch_to_piquant_dtype(xs[0].dtype), [r[2] for r in recs],
                                                       torch_to_piquant_dtype(qdtype), [x.numel() for x in xs], group_size, [r[0] for r in recs],
                                                       [r[1] for r in recs], False, self._mode(round_mode), _device_ptrs=True)

    def encode_grouped_clipped(self, x: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int, steps: int) -> None:
        """encode_grouped with the per-group clip search (``clip_steps``): the same record, other parameters."""
        sc, zp, data = self._record(buf, x.numel(), qdtype, group_size)
        self._cx(x).quantize_grouped_clipped_ptr(x.data_ptr(), torch_to_piquant_dtype(x.dtype), data, torch_to_piquant_dtype(qdtype), x.numel(), group_size,
                                                 sc, zp, 0, steps, self._mode(round_mode), _device_ptrs=True)

    def encode_batch_grouped_clipped(self, xs, bufs, qdtype: torch.dtype, round_mode: str, group_size: int, steps: int) -> None:
        """encode_grouped_clipped(xs[i], bufs[i]) for all i with one kernel launch per 16 chunks."""
        if xs:
            recs = [self._record(b, x.numel(), qdtype, group_size) for x, b in zip(xs, bufs)]
            self._cx(xs[0]).quantize_grouped_clipped_batch_ptr([x.data_ptr() for x in xs], torch_to_piquant_dtype(xs[0].dtype), [r[2] for r in recs],
                                                               torch_to_piquant_dtype(qdtype), [x.numel() for x in xs], group_size, [r[0] for r in recs],
                                                               [r[1] for r in recs], None, steps, self._mode(round_mode), _device_ptrs=True)

    def encode_grouped_ef(self, x: torch.Tensor, residual: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int) -> None:
        """encode_grouped(x + residual) with residual <- (x + residual) - what the record decodes to, one launch.  The residual's dtype goes down
        with it: float32 for a bfloat16 ``x`` is the float32 pipeline on the widened ``x``."""
        sc, zp, data = self._record(buf, x.numel(), qdtype, group_size)
        self._cx(x).quantize_grouped_ef_ptr(x.data_ptr(), torch_to_piquant_dtype(x.dtype), residual.data_ptr(), data, torch_to_piquant_dtype(qdtype),
                                            x.numel(), group_size, sc, zp, self._mode(round_mode), _device_ptrs=True,
                                            residual_dtype=_residual_dtype(residual, x))

    def encode_batch_grouped_ef(self, xs, residuals, bufs, qdtype: torch.dtype, round_mode: str, group_size: int) -> None:
        """encode_grouped_ef(xs[i], residuals[i], bufs[i]) for all i with one kernel launch per 16 chunks."""
        if xs:
            recs = [self._record(b, x.numel(), qdtype, group_size) for x, b in zip(xs, bufs)]
            self._cx(xs[0]).quantize_grouped_ef_batch_ptr([x.data_ptr() for x in xs], torch_to_piquant_dtype(xs[0].dtype), [r.data_ptr() for r in residuals],
                                                          [r[2] for r in recs], torch_to_piquant_dtype(qdtype), [x.numel() for x in xs], group_size,
                                                          [r[0] for r in recs], [r[1] for r in recs], self._mode(round_mode), _device_ptrs=True,
                                                          residual_dtype=_residual_dtype(residuals[0], xs[0]))

    def decode_batch_grouped(self, bufs, outs, qdtype: torch.dtype, reduce_op: str, group_size: int) -> None:
        """decode_grouped(bufs[i], outs[i]) for all i with one kernel launch per 16 chunks."""
        if bufs:
            recs = [self._record(b, o.numel(), qdtype, group_size) for b, o in zip(bufs, outs)]
            self._cx(outs[0]).dequantize_grouped_batch_ptr([r[2] for r in recs], torch_to_piquant_dtype(qdtype), [o.data_ptr() for o in outs],
                                                           torch_to_piquant_dtype(outs[0].dtype), [o.numel() for o in outs], group_size, [r[0] for r in recs],
                                                           [r[1] for r in recs], _REDUCE_OPS[reduce_op], _device_ptrs=True)

    def decode_sum_grouped(self, bufs, out: torch.Tensor, qdtype: torch.dtype, reduce_op: str, group_size: int) -> None:
        """out (op)= the wire buffers, added in order, one launch and one pass over ``out`` (the bytes of decode_grouped buffer by buffer, the first
        with ``reduce_op`` and the others with 'add')."""
        if bufs:
            n = out.numel()
            recs = [self._record(b, n, qdtype, group_size) for b in bufs]
            self._cx(out).dequantize_sum_grouped_ptr([r[2] for r in recs], torch_to_piquant_dtype(qdtype), [r[0] for r in recs], [r[1] for r in recs],
                                                     out.data_ptr(), torch_to_piquant_dtype(out.dtype), n, group_size, _REDUCE_OPS[reduce_op], _device_ptrs=True)

    def reduce_encode_grouped(self, bufs, acc: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int) -> None:
        """encode_grouped(acc + the wire buffers, added in order) into ``buf`` as one launch (``acc`` is scratch afterwards)."""
        n = acc.numel()
        recs = [self._record(b, n, qdtype, group_size) for b in bufs]
        sc, zp, data = self._record(buf, n, qdtype, group_size)
        self._cx(acc).reduce_quantize_grouped_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), [r[2] for r in recs], [r[0] for r in recs],
                                                  [r[1] for r in recs], data, torch_to_piquant_dtype(qdtype), n, group_size, sc, zp, self._mode(round_mode),
                                                  _device_ptrs=True)

    def reduce_encode_grouped_ef(self, bufs, acc: torch.Tensor, residual: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str,
                                 group_size: int) -> None:
        """reduce_encode_grouped(acc + residual) with residual <- what that quantization lost, one launch: the terms are added first, then the
        residual (``acc`` is scratch afterwards).  A float32 residual for a bfloat16 ``acc``: the decode ADD launches, then the mixed encode."""
        n = acc.numel()
        recs = [self._record(b, n, qdtype, group_size) for b in bufs]
        sc, zp, data = self._record(buf, n, qdtype, group_size)
        self._cx(acc).reduce_quantize_grouped_ef_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), residual.data_ptr(), [r[2] for r in recs],
                                                     [r[0] for r in recs], [r[1] for r in recs], data, torch_to_piquant_dtype(qdtype), n, group_size, sc, zp,
                                                     self._mode(round_mode), _device_ptrs=True, residual_dtype=_residual_dtype(residual, acc))

    # ---- the grouped wire in the rotated domain (``rotation_seed``): the same records, holding the rotated values ----
    def encode_grouped_rotated(self, x: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int, seed: int) -> None:
        sc, zp, data = self._record(buf, x.numel(), qdtype, group_size)
        self._cx(x).quantize_grouped_rotated_ptr(x.data_ptr(), torch_to_piquant_dtype(x.dtype), data, torch_to_piquant_dtype(qdtype), x.numel(), group_size,
                                                 sc, zp, seed, self._mode(round_mode), _device_ptrs=True)

    def decode_grouped_rotated(self, buf: torch.Tensor, out: torch.Tensor, qdtype: torch.dtype, reduce_op: str, group_size: int, seed: int) -> None:
        sc, zp, data = self._record(buf, out.numel(), qdtype, group_size)
        self._cx(out).dequantize_grouped_rotated_ptr(data, torch_to_piquant_dtype(qdtype), out.data_ptr(), torch_to_piquant_dtype(out.dtype), out.numel(),
                                                     group_size, sc, zp, seed, _REDUCE_OPS[reduce_op], _device_ptrs=True)

    def encode_batch_grouped_rotated(self, xs, bufs, qdtype: torch.dtype, round_mode: str, group_size: int, seed: int) -> None:
        """encode_grouped_rotated(xs[i], bufs[i]) for all i with one kernel launch per 16 chunks."""
        if xs:
            recs = [self._record(b, x.numel(), qdtype, group_size) for x, b in zip(xs, bufs)]
            self._cx(xs[0]).quantize_grouped_rotated_batch_ptr([x.data_ptr() for x in xs], torch_to_piquant_dtype(xs[0].dtype), [r[2] for r in recs],
                                                               torch_to_piquant_dtype(qdtype), [x.numel() for x in xs], group_size, [r[0] for r in recs],
                                                               [r[1] for r in recs], seed, self._mode(round_mode), _device_ptrs=True)

    def decode_batch_grouped_rotated(self, bufs, outs, qdtype: torch.dtype, reduce_op: str, group_size: int, seed: int) -> None:
        """decode_grouped_rotated(bufs[i], outs[i]) for all i with one kernel launch per 16 chunks."""
        if bufs:
            recs = [self._record(b, o.numel(), qdtype, group_size) for b, o in zip(bufs, outs)]
            self._cx(outs[0]).dequantize_grouped_rotated_batch_ptr([r[2] for r in recs], torch_to_piquant_dtype(qdtype), [o.data_ptr() for o in outs],
                                                                   torch_to_piquant_dtype(outs[0].dtype), [o.numel() for o in outs], group_size,
                                                                   [r[0] for r in recs], [r[1] for r in recs], seed, _REDUCE_OPS[reduce_op],
                                                                   _device_ptrs=True)

    def reduce_encode_grouped_rotated(self, bufs, acc: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int,
                                      seed: int) -> None:
        """encode_grouped(rotate(acc) + the wire buffers, added in order, in float32) into ``buf`` as one launch (at most 16 buffers; ``acc`` is
        only read)."""
        n = acc.numel()
        recs = [self._record(b, n, qdtype, group_size) for b in bufs]
        sc, zp, data = self._record(buf, n, qdtype, group_size)
        self._cx(acc).reduce_quantize_grouped_rotated_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), [r[2] for r in recs], [r[0] for r in recs],
                                                          [r[1] for r in recs], data, torch_to_piquant_dtype(qdtype), n, group_size, sc, zp, seed,
                                                          self._mode(round_mode), _device_ptrs=True)

    def encode_grouped_rotated_ef(self, x: torch.Tensor, residual: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str, group_size: int,
                                  seed: int) -> None:
        """encode_grouped_rotated(x) with error feedback in the rotated domain: the float32 ``residual`` (rotated values, whatever ``x``'s dtype) is
        added behind the rotation and then holds what the record lost, one launch."""
        sc, zp, data = self._record(buf, x.numel(), qdtype, group_size)
        self._cx(x).quantize_grouped_rotated_ef_ptr(x.data_ptr(), torch_to_piquant_dtype(x.dtype), residual.data_ptr(), data, torch_to_piquant_dtype(qdtype),
                                                    x.numel(), group_size, sc, zp, seed, self._mode(round_mode), _device_ptrs=True)

    def encode_batch_grouped_rotated_ef(self, xs, residuals, bufs, qdtype: torch.dtype, round_mode: str, group_size: int, seed: int) -> None:
        """encode_grouped_rotated_ef(xs[i], residuals[i], bufs[i]) for all i with one kernel launch per 16 chunks (float32 residuals)."""
        if xs:
            recs = [self._record(b, x.numel(), qdtype, group_size) for x, b in zip(xs, bufs)]
            self._cx(xs[0]).quantize_grouped_rotated_ef_batch_ptr([x.data_ptr() for x in xs], torch_to_piquant_dtype(xs[0].dtype),
                                                                  [r.data_ptr() for r in residuals], [r[2] for r in recs], torch_to_piquant_dtype(qdtype),
                                                                  [x.numel() for x in xs], group_size, [r[0] for r in recs], [r[1] for r in recs], seed,
                                                                  self._mode(round_mode), _device_ptrs=True)

    def reduce_encode_grouped_rotated_ef(self, bufs, acc: torch.Tensor, residual: torch.Tensor, buf: torch.Tensor, qdtype: torch.dtype, round_mode: str,
                                         group_size: int, seed: int) -> None:
        """reduce_encode_grouped_rotated with error feedback on the re-quantization: the terms are added first, then the float32 ``residual`` of the
        rotated domain, which then holds what the record lost; one launch (at most 16 buffers; ``acc`` is only read)."""
        n = acc.numel()
        recs = [self._record(b, n, qdtype, group_size) for b in bufs]
        sc, zp, data = self._record(buf, n, qdtype, group_size)
        self._cx(acc).reduce_quantize_grouped_rotated_ef_ptr(acc.data_ptr(), torch_to_piquant_dtype(acc.dtype), residual.data_ptr(), [r[2] for r in recs],
                                                             [r[0] for r in recs], [r[1] for r in recs], data, torch_to_piquant_dtype(qdtype), n, group_size,
                                                             sc, zp, seed, self._mode(round_mode), _device_ptrs=True)

    def decode_sum_grouped_rotated(self, bufs, out: torch.Tensor, qdtype: torch.dtype, reduce_op: str, group_size: int, seed: int) -> None:
        """out (op)= the inverse rotation of the float32 sum of the wire buffers, added in order: one launch (at most 16 buffers) and one pass
        over ``out``."""
        if bufs:
            n = out.numel()
            recs = [self._record(b, n, qdtype, group_size) for b in bufs]
            self._cx(out).dequantize_sum_grouped_rotated_ptr([r[2] for r in recs], torch_to_piquant_dtype(qdtype), [r[0] for r in recs],
                                                             [r[1] for r in recs], out.data_ptr(), torch_to_piquant_dtype(out.dtype), n, group_size, seed,
                                                             _REDUCE_OPS[reduce_op], _device_ptrs=True)


def _exchange(send: torch.Tensor, recv: torch.Tensor, nxt: int, prv: int, group) -> None:
    """Send `send` to the next rank of the ring while receiving `recv` from the previous one.  RCCL (backend nccl)
    moves device buffers directly over xGMI; other backends (gloo, used in tests) are staged through host memory."""
    if dist.get_backend(group) == 'nccl':
        ops = [dist.P2POp(dist.isend, send, nxt, group), dist.P2POp(dist.irecv, recv, prv, group)]
        for req in dist.batch_isend_irecv(ops):
            req.wait()
        return
    s_host = send.cpu()
    r_host = torch.empty(recv.shape, dtype=recv.dtype)
    req_s = dist.isend(s_host, nxt, group=group)
    req_r = dist.irecv(r_host, prv, group=group)
    req_s.wait()
    req_r.wait()
    recv.copy_(r_host)


def _all_to_all(send: torch.Tensor, recv: torch.Tensor, group) -> None:
    """Equal-split all-to-all of byte buffers (slot j of `send` goes to rank j).  RCCL moves device buffers peer to peer -- on
    MI355X every pair of GPUs has its own xGMI link, so all G-1 transfers of a rank run at once; other backends (gloo, tests)
    are staged through host memory."""
    if dist.get_backend(group) == 'nccl':
        dist.all_to_all_single(recv, send, group=group)
        return
    r_host = torch.empty(recv.shape, dtype=recv.dtype)
    dist.all_to_all_single(r_host, send.cpu(), group=group)
    recv.copy_(r_host)


def _all_gather(mine: torch.Tensor, everyone: torch.Tensor, group) -> None:
    """`everyone` = concatenation over ranks of equally sized `mine` buffers."""
    world = dist.get_world_size(group)
    if dist.get_backend(group) == 'nccl':
        dist.all_gather_into_tensor(everyone, mine, group=group)
        return
    parts = [torch.empty(mine.shape, dtype=mine.dtype) for _ in range(world)]
    dist.all_gather(parts, mine.cpu(), group=group)
    everyone.copy_(torch.cat(parts))


# -----------------------------------------------------------------------------------------------------------------
# Peer-to-peer transport of the mesh schedule: the encode kernels store straight into the peers' receive buffers.
# -----------------------------------------------------------------------------------------------------------------
class _PeerMesh:
    """Buffers of ``quantized_all_reduce_direct(transport='p2p')``, per rank one payload allocation and one small flag allocation, both mapped
    by every other rank (``_PeerMapped``):

        recv[2][world][slot]   chunk j of peer i lands in recv[parity][i] of rank j -- written by PEER i's encode kernel, no copy
        mine[2][slot]          the owner's finished chunk -- READ by every peer's decode kernel, no all-gather
        arrived[world]         uint32 sequence numbers: arrived[i] = s  <=>  peer i's chunk of exchange s is in recv[s & 1][i]
        finished[world]        finished[i] = s  <=>  owner i's mine[s & 1] holds its finished chunk of exchange s

    The payload is ordinary device memory: it is produced by one launch and consumed by a LATER one on the other side (the flag wait sits
    between them), and kernel boundaries are where ordinary device memory becomes coherent between GPUs.  The flags are polled by a running
    kernel while another GPU writes them: fine-grained memory.  Two parities suffice: a rank enters exchange s + 1 only behind its own decode
    of exchange s, a peer passes its wait of exchange s + 1 only after that rank's encode of s + 1 -- so when anybody writes parity
    (s + 2) & 1 = s & 1 again, every reader of exchange s is done.
    """

    _cache = {}

    def __init__(self, group, device: torch.device, slot: int, world: int, rank: int):
        self.world, self.rank, self.slot, self.device = world, rank, slot, device
        self.ctx = Context.get(device.index)
        self.off_mine = 2 * world * slot
        payload = -(-(self.off_mine + 2 * slot) // 256) * 256
        _check_peers_reachable(group, device, world, rank)
        self.data = _PeerMapped(self.ctx, group, payload, world, rank, fine_grained=False)
        self.flags = _PeerMapped(self.ctx, group, 8 * world, world, rank, fine_grained=True)     # arrived[world] then finished[world], all 0
        self.off_arrived, self.off_finished = 0, 4 * world
        torch.cuda.synchronize(device)
        dist.barrier(group=group)        # nobody signals into memory somebody has not finished mapping
        self.seq = 0
        self.order = _StreamOrder()
        self.poisoned = False            # a wait of an exchange on this device gave up (_raise_peer_timeout): late stores may land in these buffers

    @classmethod
    def get(cls, group, device, slot, world, rank):
        """The group's mesh on this device, grown when a tensor needs larger slots than it has (every rank sees the same sizes in the same order,
        so every rank grows at the same call).  Growing is a collective behind a device synchronisation: this rank's last decode -- the last
        reader of the peers' old buffers -- has finished before the barriers inside release() let anybody unmap or free them."""
        owner = group if group is not None else dist.group.WORLD
        key = (id(owner), device.index, world)
        m = cls._cache.get(key)
        if m is not None and m.owner is not owner:      # an id recycled by a later process group: those peers are gone
            m = cls._cache.pop(key)
            m.data.discard()
            m.flags.discard()
            m = None
        if m is None or m.slot < slot:
            if m is not None:
                cls._cache.pop(key).release(group)
            m = cls._cache[key] = cls(group, device, slot, world, rank)
            m.owner = owner
        return m

    def release(self, group) -> None:
        torch.cuda.synchronize(self.device)
        self.data.release(group)
        self.flags.release(group)

    def flag_ptr(self, j: int, which: str, i: int) -> int:
        return self.flags.ptrs[j] + (self.off_arrived if which == 'arrived' else self.off_finished) + 4 * i


def release_peer_meshes(group: Optional[dist.ProcessGroup] = None) -> None:
    """Drops the peer-mapped buffers of ``transport='p2p'`` for ``group`` (a collective: every rank calls it, e.g. before
    ``destroy_process_group``).  The next p2p all-reduce builds them again."""
    owner = group if group is not None else dist.group.WORLD
    for cache in (_PeerMesh._cache, _KeyMesh._cache):
        for key in [k for k, m in cache.items() if m.owner is owner]:
            cache.pop(key).release(group)


def ring_chunks(numel: int, world_size: int, packed_bits: int = 8, align: int = 4096):
    """Chunk boundaries of the ring: `world_size` contiguous chunks; interior boundaries are multiples of `align` elements
    (whole packed bytes and 16-byte vectors on both sides of every kernel); the last chunk keeps the ragged end."""
    if align % (8 // packed_bits if packed_bits < 8 else 1) != 0:
        raise ValueError(f'align={align} must be a multiple of the pack factor')
    per = -(-numel // world_size)
    per = -(-per // align) * align
    bounds = [min(i * per, numel) for i in range(world_size)] + [numel]
    return [(bounds[i], bounds[i + 1]) for i in range(world_size)]


class _Wire:
    """What every record of one collective call has in common -- the ops object, the quantized dtype, the rounding mode, the record format
    (``group_size`` None: 16-byte header + packed bytes; else ``grouped_wire_layout``), the flattened residual (or None) and whether the
    re-quantizations of partial sums feed it (``requantize``), the rotation's seed (``rotation_seed``, or None: the grouped wire then carries the
    records of the rotated values, and a residual is then the float32 one of the rotated domain, ``rotated_error_feedback``) -- and the only place that knows which ``ops.*`` method a step of a schedule maps
    to.  The schedules below are written once, on a wire.  ``chunk`` is the ``(begin, end)`` of the values a step works on: where a residual
    takes part, the step works on that slice of it."""

    def __init__(self, ops, quant_dtype: torch.dtype, round_mode: str, group_size: Optional[int] = None, residual: Optional[torch.Tensor] = None,
                 requantize: bool = False, rotation_seed: Optional[int] = None, clip_steps: Optional[int] = None):
        self.ops, self.round_mode, self.group_size = ops, round_mode, group_size
        self.seed = rotation_seed
        self.clip_steps = clip_steps             # the encodes search each group's clipping range (never with a seed or a residual: _check_clip_steps)
        self.quant_dtype, self.qdt = quant_dtype, torch_to_piquant_dtype(quant_dtype)     # the torch dtype the ops take, its DataType for the lengths
        self.residual = None if residual is None else residual.view(-1)
        self.requantize = requantize

    def nbytes(self, numel: int) -> int:
        """Length of the record of ``numel`` elements."""
        if self.group_size is None:
            return _HEADER_BYTES + self.qdt.packed_nbytes(numel)
        return grouped_wire_layout(numel, self.group_size, self.qdt.bit_size).nbytes

    def encode(self, x, buf, chunk, ef: bool = True) -> None:
        """``ef`` False: the rotated owner's encode without ``requantize``, which leaves the residual alone."""
        if self.group_size is None:
            self.ops.encode(x, buf, self.quant_dtype, self.round_mode)
        elif self.clip_steps is not None:
            self.ops.encode_grouped_clipped(x, buf, self.quant_dtype, self.round_mode, self.group_size, self.clip_steps)
        elif self.seed is not None and (self.residual is None or not ef):
            self.ops.encode_grouped_rotated(x, buf, self.quant_dtype, self.round_mode, self.group_size, self.seed)
        elif self.seed is not None:
            self.ops.encode_grouped_rotated_ef(x, self.residual[chunk[0]:chunk[1]], buf, self.quant_dtype, self.round_mode, self.group_size, self.seed)
        elif self.residual is None:
            self.ops.encode_grouped(x, buf, self.quant_dtype, self.round_mode, self.group_size)
        else:
            self.ops.encode_grouped_ef(x, self.residual[chunk[0]:chunk[1]], buf, self.quant_dtype, self.round_mode, self.group_size)

    def encode_batch(self, xs, bufs, chunks) -> None:
        if self.group_size is None:
            self.ops.encode_batch(xs, bufs, self.quant_dtype, self.round_mode)
        elif self.clip_steps is not None:
            self.ops.encode_batch_grouped_clipped(xs, bufs, self.quant_dtype, self.round_mode, self.group_size, self.clip_steps)
        elif self.seed is not None and self.residual is None:
            self.ops.encode_batch_grouped_rotated(xs, bufs, self.quant_dtype, self.round_mode, self.group_size, self.seed)
        elif self.seed is not None:
            self.ops.encode_batch_grouped_rotated_ef(xs, [self.residual[b:e] for b, e in chunks], bufs, self.quant_dtype, self.round_mode, self.group_size,
                                                     self.seed)
        elif self.residual is None:
            self.ops.encode_batch_grouped(xs, bufs, self.quant_dtype, self.round_mode, self.group_size)
        else:
            self.ops.encode_batch_grouped_ef(xs, [self.residual[b:e] for b, e in chunks], bufs, self.quant_dtype, self.round_mode, self.group_size)

    def reduce_encode(self, terms, acc, buf, chunk) -> None:
        """encode(acc + the records in ``terms``, added in order) into ``buf``, one launch; the residual takes part only with ``requantize``."""
        if self.group_size is None:
            self.ops.reduce_encode(terms, acc, buf, self.quant_dtype, self.round_mode)
        elif self.seed is not None and not self.requantize:
            self.ops.reduce_encode_grouped_rotated(terms, acc, buf, self.quant_dtype, self.round_mode, self.group_size, self.seed)
        elif self.seed is not None:
            self.ops.reduce_encode_grouped_rotated_ef(terms, acc, self.residual[chunk[0]:chunk[1]], buf, self.quant_dtype, self.round_mode, self.group_size,
                                                      self.seed)
        elif not self.requantize:
            self.ops.reduce_encode_grouped(terms, acc, buf, self.quant_dtype, self.round_mode, self.group_size)
        else:
            self.ops.reduce_encode_grouped_ef(terms, acc, self.residual[chunk[0]:chunk[1]], buf, self.quant_dtype, self.round_mode, self.group_size)

    def owner_encode(self, terms, acc, buf, chunk) -> None:
        """The mesh owner's step: ``reduce_encode``.  In the rotated domain it is the reduce-scatter's step followed by the all-gather's --
        ``decode_sum(terms, acc, 'add')``, which leaves the sum in ``acc``, then ``encode(acc)`` -- two launches: only so do reduce-scatter +
        all-gather leave the bytes of the direct all-reduce (the one-launch rotated reduce keeps the sum in the rotated domain, the two halves
        pass it through the original one and the tensor's type: equal in exact arithmetic, not in float32).  That encode feeds the owner's own
        chunk of a rotated residual only with ``requantize``."""
        if self.seed is None:
            self.reduce_encode(terms, acc, buf, chunk)
        else:
            if terms:
                self.decode_sum(terms, acc, 'add')
            self.encode(acc, buf, chunk, ef=self.requantize)

    def decode(self, buf, out, op: str) -> None:
        if self.group_size is None:
            self.ops.decode(buf, out, self.quant_dtype, op)
        elif self.seed is not None:
            self.ops.decode_grouped_rotated(buf, out, self.quant_dtype, op, self.group_size, self.seed)
        else:
            self.ops.decode_grouped(buf, out, self.quant_dtype, op, self.group_size)

    def decode_batch(self, bufs, outs, op: str) -> None:
        if self.group_size is None:
            self.ops.decode_batch(bufs, outs, self.quant_dtype, op)
        elif self.seed is not None:
            self.ops.decode_batch_grouped_rotated(bufs, outs, self.quant_dtype, op, self.group_size, self.seed)
        else:
            self.ops.decode_batch_grouped(bufs, outs, self.quant_dtype, op, self.group_size)

    def decode_sum(self, terms, out, op: str) -> None:
        """The grouped wire's only: nothing sums per-chunk records under a ``reduce_op``."""
        if self.seed is not None:
            self.ops.decode_sum_grouped_rotated(terms, out, self.quant_dtype, op, self.group_size, self.seed)
        else:
            self.ops.decode_sum_grouped(terms, out, self.quant_dtype, op, self.group_size)


class _Chunks(NamedTuple):
    """The chunk and slot arithmetic of one call: chunk j of the flat tensor, the length of its record, and the slot of the mesh's buffers."""
    bounds: list             # ring_chunks: (begin, end) per chunk
    views: list              # flat[begin:end] per chunk
    nbytes: list             # the record length per chunk (an empty chunk's per-chunk record is its header, its grouped record is empty)
    slot: int                # the longest record, rounded up: every slot starts on a 16-byte boundary (vector kernels on both sides)

    @classmethod
    def of(cls, wire: _Wire, flat: torch.Tensor, world: int) -> '_Chunks':
        bounds = ring_chunks(flat.numel(), world, wire.qdt.bit_size)
        nbytes = [wire.nbytes(e - b) for b, e in bounds]
        return cls(bounds, [flat[b:e] for b, e in bounds], nbytes, -(-max(nbytes) // 16) * 16)

    def record(self, buf: torch.Tensor, i: int, j: int) -> torch.Tensor:
        """The bytes of a record of chunk j in slot i of ``buf``."""
        return buf[i * self.slot: i * self.slot + self.nbytes[j]]


def _ring(wire: _Wire, ch: _Chunks, group, world: int, rank: int, device: torch.device) -> None:
    """The ring schedule of ``quantized_all_reduce`` on either wire."""
    nxt = dist.get_global_rank(group, (rank + 1) % world) if group is not None else (rank + 1) % world
    prv = dist.get_global_rank(group, (rank - 1) % world) if group is not None else (rank - 1) % world
    views, lens = ch.views, ch.nbytes
    send, recv, nxt_send = (torch.empty(max(lens), dtype=torch.uint8, device=device) for _ in range(3))
    # ---- reduce-scatter: after G-1 hops rank r owns the complete sum of chunk (r+1) % G ----
    # What arrives at a hop is added to the local chunk and the sum is what the next hop forwards: that is ONE call (and one
    # launch), reduce_encode = quantize(local + dequantize(received)); the local chunk itself need not be updated, the forwarded
    # buffer carries the sum and every chunk is overwritten by the all-gather at the end.  With a residual the first encode (chunk
    # ``rank``, this rank's own values) feeds that chunk of it; with ``requantize`` every hop feeds its chunk, each chunk exactly once.
    n_cur = lens[rank]
    if views[rank].numel():
        wire.encode(views[rank], send[:n_cur], ch.bounds[rank])
    for step in range(world - 1):
        j = (rank - step - 1) % world
        _exchange(send[:n_cur], recv[:lens[j]], nxt, prv, group)
        if views[j].numel():
            wire.reduce_encode([recv[:lens[j]]], views[j], nxt_send[:lens[j]], ch.bounds[j])
        send, nxt_send = nxt_send, send
        n_cur = lens[j]
    if world == 1 and n_cur:   # test hook only: the encoded chunk makes one trip through the transport, to this rank itself
        _exchange(send[:n_cur], recv[:n_cur], nxt, prv, group)
        send, recv = recv, send
    # ---- all-gather: the finished chunk's bytes (now in `send`) circulate unchanged ----
    own = (rank + 1) % world
    assert n_cur == lens[own]
    if views[own].numel():
        wire.decode(send[:n_cur], views[own], 'set')   # the owner keeps exactly what everyone else will see
    for step in range(world - 1):
        j = (rank - step) % world
        _exchange(send[:n_cur], recv[:lens[j]], nxt, prv, group)
        if views[j].numel():
            wire.decode(recv[:lens[j]], views[j], 'set')
        send, recv = recv, send          # forward the received bytes as they are
        n_cur = lens[j]


def _mesh_scatter(wire: _Wire, ch: _Chunks, group, world: int, rank: int, device: torch.device):
    """Reduce-scatter over the mesh up to the owner's step: this rank's values of every peer's non-empty chunk are encoded in ONE batched call
    (with a residual: feeding the peers' chunks of it), slot j of ``send`` goes to rank j, and what comes back -- the peers' records of this
    rank's own chunk, in increasing rank order -- is returned."""
    send = torch.zeros(world * ch.slot, dtype=torch.uint8, device=device)     # zeros: the padding between the records travels
    recv = torch.empty(world * ch.slot, dtype=torch.uint8, device=device)
    peers = [j for j in range(world) if j != rank and ch.views[j].numel()]
    wire.encode_batch([ch.views[j] for j in peers], [ch.record(send, j, j) for j in peers], [ch.bounds[j] for j in peers])
    _all_to_all(send, recv, group)
    return [ch.record(recv, i, rank) for i in range(world) if i != rank]


def _mesh_gather(wire: _Wire, ch: _Chunks, mine: torch.Tensor, group, world: int, device: torch.device) -> None:
    """All-gather over the mesh: ``mine`` (one slot holding the owner's finished record) is gathered and every non-empty chunk is stored from
    the gathered bytes in ONE batched SET decode -- the own chunk included, so all ranks end bit-identical."""
    gathered = torch.empty(world * ch.slot, dtype=torch.uint8, device=device)   # a fresh buffer: the owner's launch may still be reading the scatter's
    _all_gather(mine, gathered, group)
    full = [j for j in range(world) if ch.views[j].numel()]
    wire.decode_batch([ch.record(gathered, j, j) for j in full], [ch.views[j] for j in full], 'set')


def quantized_all_reduce(
    tensor: torch.Tensor,
    *,
    quant_dtype: torch.dtype = torch.uint8,
    round_mode: str = 'nearest',
    group: Optional[dist.ProcessGroup] = None,
    ctx: Optional[Context] = None,
    algorithm: str = 'direct',
    transport: str = 'collective',
    timeout: Optional[float] = None,
    group_size: Optional[int] = None,
    error_feedback: Optional[torch.Tensor] = None,
    error_feedback_requantize: bool = False,
    rotation_seed: Optional[int] = None,
    rotated_error_feedback: Optional[torch.Tensor] = None,
    clip_steps: Optional[int] = None,
    _ops=None,
    _single_rank_collectives: bool = False,
) -> torch.Tensor:
    """In-place SUM all-reduce of a contiguous float32/bfloat16 tensor whose wire format is quantized.

    ``group_size`` (None, or a power of two in [32, 4096]; 128 is the usual choice): None quantizes every chunk of the wire with one
    (scale, zero point) in a 16-byte header.  An int quantizes group-wise -- one (scale, zero point) per run of ``group_size`` elements, so
    that an outlier stretches the range of its own group only -- and a chunk's record becomes ``float32 scales[ng] | uint8 zero_points[ng] |
    pad to 16 | packed bytes`` (``grouped_wire_layout``; 5 bytes more per group).  ``ring_chunks`` puts every interior chunk boundary on a
    multiple of 4096 elements, so no group straddles two chunks: the wire groups are exactly the groups ``quantize_grouped`` forms on the
    whole tensor.  Every encode is ``quantize_grouped`` (the mesh's: one batched launch), every re-quantization of a partial sum is ONE
    ``reduce_quantize_grouped`` launch, every decode ``dequantize_grouped`` (the mesh's: one batched launch); the schedules, the launches
    per all-reduce and the bit-identity of all ranks are those of the per-chunk path.  ``transport='p2p'`` does not take grouped
    parameters.  (Unmeasured on more than one GPU, like the rest of this module's multi-GPU paths.)

    ``error_feedback`` (``group_size`` only): a contiguous tensor of the all-reduced tensor's dtype, device and numel that the caller keeps between
    steps (zeros before the first).  Every quantization this rank applies to ITS OWN contribution becomes ``quantize_grouped_ef`` on the matching
    slice: the slice of the residual is added to the values before they are quantized and then holds what the quantization lost, so that the loss
    is part of the next step's contribution instead of being thrown away.  In the mesh schedule that is the one batched encode of the peers' chunks
    (still one launch per 16 chunks); in the ring the first encode of chunk ``rank``.  Slices the schedule contributes unquantized -- the mesh's own
    chunk, the ring's other chunks -- are neither read nor written, and the re-quantizations of partial sums stay as they are.  A residual
    therefore belongs to one (world size, rank, algorithm, ``error_feedback_requantize``): carry it over only between all-reduces of the same
    shape in the same group with the same schedule and the same flag.  Without ``group_size``, or with ``transport='p2p'``, ``error_feedback``
    raises ValueError before anything moves; ``None`` (the default) leaves every byte and every launch as it was.  A one-rank group returns at
    once and leaves the residual alone.  A bfloat16 tensor also takes a FLOAT32 residual (same device and numel), in both schedules and with
    ``error_feedback_requantize``: the encodes then run in float32 on the widened values and the residual keeps what the wire loses to float32
    precision instead of rounding it to bfloat16 twice per step (each up to 2^-9 |y|, as much as a uint8 half step); the wire and what receivers
    decode into stay as they are.  No other pair of dtypes is accepted.

    ``error_feedback_requantize`` (``error_feedback`` only; default False: every byte and every launch as without it): the residual also covers
    the SECOND quantization every value meets, the re-quantization of a partial sum, whose rounding error is otherwise thrown away identically on
    every rank.  The mesh owner's ``reduce_quantize_grouped`` becomes ``reduce_quantize_grouped_ef`` on the rank's OWN chunk of the residual
    (still three launches per all-reduce, and every slice of the residual is now used); every hop of the ring becomes
    ``reduce_quantize_grouped_ef`` on chunk ``(rank - step - 1) % world`` of the residual, so that with the first encode each rank touches each
    chunk of its residual exactly once per all-reduce.  The residual is added after the received terms.  With it the sum over steps of the
    results differs from the sum of the inputs by what the ranks' residuals hold (up to roundings in the tensor's dtype): the all-reduce is
    conservative over steps.  ValueError before anything moves without ``error_feedback``, without ``group_size`` or with ``transport='p2p'``.

    ``rotation_seed`` (``group_size`` only; default None: every byte, every launch and every ``_ops`` call as without it): an int, taken modulo
    2^64, runs the whole collective in the domain of the randomized Hadamard rotation (``piquant.torch.hadamard_grouped``), for heavy-tailed
    values whose outliers would stretch their groups' steps.  Every encode becomes ``quantize_grouped_rotated``; every hop of the ring ONE
    ``reduce_quantize_grouped_rotated`` launch (the received record holds rotated values already: only the local chunk is rotated, and the sum
    stays float32 until it is quantized, also for a bfloat16 tensor); the mesh owner's step ``dequantize_sum_grouped_rotated(..., 'add')`` of
    the world - 1 received records into the own chunk followed by ``quantize_grouped_rotated`` of it -- the reduce-scatter's step and the
    all-gather's, two launches, so that ``quantized_reduce_scatter`` + ``quantized_all_gather`` leave exactly the bytes of the direct
    all-reduce (the one-launch reduce would not: it keeps the sum in the rotated domain); every decode ``dequantize_grouped_rotated`` 'set' of
    the same gathered bytes on every rank, the owner included: all ranks end bit-identical.  The wire format is unchanged; ``ring_chunks`` keeps
    every interior boundary on a multiple of 4096 elements, so every chunk rotates exactly as the whole tensor does.  ALL RANKS MUST PASS THE SAME
    SEED: the library does not check it, and ranks that disagree sum values of different domains.  The mesh encodes its world - 1 chunks with ONE
    ``quantize_grouped_rotated_batch`` launch and decodes its world chunks with ONE ``dequantize_grouped_rotated_batch`` launch (one per 16
    chunks), as the un-rotated grouped mesh does with its batches: with the owner's two launches, four launches per all-reduce.  One consequence,
    the un-rotated grouped mesh's rule: with ``round_mode='stochastic'`` and no pinned threshold a rotated mesh draws ONE threshold per batch,
    where it drew one per chunk while every chunk was a launch of its own; the bytes under nearest rounding, under a pinned threshold
    (``Context.set_stochastic_threshold``) and in per-element mode are what they were.  uint2 records gain nothing from the rotation in the
    all-reduce without error feedback.  ValueError before anything moves: without ``group_size``, with ``transport='p2p'``, with
    ``error_feedback`` (that residual lives in the original domain; ``rotated_error_feedback`` is the one that goes with a rotation), and in the
    direct schedule with more than 17 ranks (the owner's one launch sums at most 16 records).

    ``rotated_error_feedback`` (``group_size`` and ``rotation_seed`` only; default None: every byte, every launch and every ``_ops`` call as
    without it): error feedback with the residual kept in the ROTATED domain -- a contiguous FLOAT32 tensor (float32 also for a bfloat16 tensor)
    of the tensor's device and numel that the caller keeps between steps (zeros before the first).  It is a keyword of its own because it is a
    different object from ``error_feedback``'s residual: a record of rotated values.  Every encode of this rank's own contribution becomes
    ``quantize_grouped_rotated_ef`` on the matching slice (the ring's first encode; the mesh's peer chunks, ONE
    ``quantize_grouped_rotated_ef_batch`` launch per 16 of them); with
    ``error_feedback_requantize`` every hop of the ring becomes ONE ``reduce_quantize_grouped_rotated_ef`` launch on the hop's chunk, and the
    mesh owner's ``quantize_grouped_rotated`` becomes ``quantize_grouped_rotated_ef`` on the rank's own chunk: each chunk of the residual is then
    touched exactly once per call.  The residual belongs to one (world size, rank, algorithm, ``error_feedback_requantize``, SEED, GROUP SIZE):
    ``piquant.torch.hadamard_grouped(residual, seed=..., inverse=True)`` takes it to the original domain to change either.  One NaN makes its
    whole group's residual NaN until the caller zeroes it.  ValueError before anything moves: without ``group_size`` or ``rotation_seed``, with
    ``error_feedback``, with ``transport='p2p'``, or a residual that is not float32, contiguous, on the tensor's device and of its numel.

    ``transport='p2p'`` (``algorithm='direct'`` only, one node; EXPERIMENTAL until it has run between two GPUs): no collective at all -- the
    encode kernels store into the peers' receive buffers over xGMI and flags order the steps (``quantized_all_reduce_direct``).  ``timeout``
    (seconds; default ``PIQUANT_P2P_TIMEOUT_S`` or 10 minutes) bounds every wait for a peer; a rank that is later than that does not fault the
    GPU: the NEXT p2p call on the device (or ``check_peer_timeouts``) raises RuntimeError naming it.  The all-reduce is asynchronous, so a caller of
    ``transport='p2p'`` MUST call ``check_peer_timeouts()`` (it synchronises) before it consumes the result -- e.g. at the step's synchronisation point,
    in front of the optimizer step: behind a wait that ran out the tensor holds sums of stale bytes.  After such a failure the rank signals nothing
    more (its peers give up on it in turn, so every rank learns of it) and the group's peer-mapped buffers stay refused until every rank has called
    ``release_peer_meshes(group)``.

    (``_single_rank_collectives`` is a test hook: with a one-rank group the function normally returns at once; with the hook it
    runs the whole schedule -- encode, the group's collectives with the rank as its own only peer, decode -- so that the RCCL
    branches execute on a box with one GPU.  The result is then ``dequantize(quantize(x))``.)

    ``algorithm='direct'`` (the default: MI355X's xGMI is a point-to-point mesh) is the schedule of
    ``quantized_all_reduce_direct`` -- one all-to-all + one all-gather, every value quantized exactly twice, 78 us of kernel
    time per rank for an 8-way all-reduce of 109 MB against 152 us for the ring.  ``algorithm='ring'`` is the schedule described
    here, for topologies where one neighbour link is all there is.

    Ring reduce-scatter: at every hop a rank receives ``header + packed bytes`` of a chunk's partial sum from its predecessor, adds
    them to its own values of that chunk and quantizes the new partial sum -- parameters from the sum itself, computed on the device
    into the 16-byte wire header -- for its successor: ONE kernel launch per hop (``reduce_quantize_dynamic``) and no host round trip.
    Ring all-gather: the owner of a
    finished chunk quantizes it once; the bytes travel round the ring unchanged and every rank (the owner included)
    stores ``dequantize(..., 'set')`` of the same bytes, so all ranks end bit-identical.  Wire traffic per element is
    1 byte (uint8) / 0.5 (uint4) instead of 4, over the same 2(G-1)/G ring schedule; each xGMI link carries one
    point-to-point stream, which is what the per-link (not NVSwitch-style) bandwidth of MI355X wants.

    ``clip_steps`` must stay None: the per-group clip search serves ``quantized_reduce_scatter`` and ``quantized_all_gather``, where no partial sum
    is re-quantized; here it raises ValueError before anything moves.
    """
    if not (tensor.is_contiguous() and tensor.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError('quantized_all_reduce needs a contiguous float32 or bfloat16 tensor')
    _check_clip_steps(clip_steps, group_size, all_reduce=True)
    if algorithm not in ('ring', 'direct'):
        raise ValueError(f"algorithm must be 'ring' or 'direct', got {algorithm!r}")
    if transport not in ('collective', 'p2p'):
        raise ValueError(f"transport must be 'collective' or 'p2p', got {transport!r}")
    _check_all_reduce_group_size(group_size, transport)
    _check_error_feedback(error_feedback, tensor, group_size, transport)
    _check_error_feedback_requantize(error_feedback_requantize, error_feedback if error_feedback is not None else rotated_error_feedback, group_size,
                                     transport)
    seed = _check_rotation_seed(rotation_seed, group_size, transport, error_feedback)
    _check_rotated_error_feedback(rotated_error_feedback, tensor, group_size, rotation_seed, transport, error_feedback)
    if algorithm == 'direct':
        return quantized_all_reduce_direct(tensor, quant_dtype=quant_dtype, round_mode=round_mode, group=group, ctx=ctx, transport=transport, timeout=timeout,
                                           group_size=group_size, error_feedback=error_feedback, error_feedback_requantize=error_feedback_requantize,
                                           rotation_seed=rotation_seed, rotated_error_feedback=rotated_error_feedback, _ops=_ops, _single_rank_collectives=_single_rank_collectives)
    if transport != 'collective':
        raise ValueError("transport='p2p' is the mesh schedule's (algorithm='direct'); the ring forwards through its neighbours")
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if world == 1 and not _single_rank_collectives:
        return tensor
    wire = _Wire(_ops or _DeviceOps(ctx), quant_dtype, round_mode, group_size, error_feedback if seed is None else rotated_error_feedback,
                 error_feedback_requantize, seed)
    _ring(wire, _Chunks.of(wire, tensor.view(-1), world), group, world, rank, tensor.device)
    return tensor


def quantized_all_reduce_direct(
    tensor: torch.Tensor,
    *,
    quant_dtype: torch.dtype = torch.uint8,
    round_mode: str = 'nearest',
    group: Optional[dist.ProcessGroup] = None,
    ctx: Optional[Context] = None,
    transport: str = 'collective',
    timeout: Optional[float] = None,
    group_size: Optional[int] = None,
    error_feedback: Optional[torch.Tensor] = None,
    error_feedback_requantize: bool = False,
    rotation_seed: Optional[int] = None,
    rotated_error_feedback: Optional[torch.Tensor] = None,
    clip_steps: Optional[int] = None,
    _ops=None,
    _single_rank_collectives: bool = False,
) -> torch.Tensor:
    """In-place quantized SUM all-reduce for a point-to-point mesh (MI355X: every GPU has its own xGMI link to each of its 7 peers).

    A ring keeps one link per direction busy and re-quantizes a partial sum at each of its G-1 hops.  Here rank r owns chunk r:

    1. every rank quantizes chunk j of its tensor for every peer j (parameters from that chunk, 16-byte header + packed bytes;
       all G-1 chunks in ONE kernel launch, ``quantize_dynamic_batch``),
    2. ONE all-to-all delivers them -- G-1 transfers per rank, each on its own link, all at once,
    3. the owner adds the G-1 received chunks to its own (unquantized) values and
    4. quantizes the finished chunk -- both in ONE launch that keeps the sum on chip (``reduce_quantize_dynamic``); ONE all-gather
       distributes it, and every rank (the owner included) stores
       ``dequantize(..., 'set')`` of the same bytes (all G chunks in one launch), so all ranks end bit-identical.

    Every value is quantized exactly twice whatever the world size (a ring: up to G times), the wire carries the same
    2(G-1)/G x packed bytes per element, and the two collectives are what RCCL implements natively over the mesh.

    ``transport='p2p'``: the same four steps and the same bytes with NO collective.  Step 1's kernel stores chunk j straight into rank j's
    receive buffer (an address of rank j's memory mapped here once: HIP IPC, ``_PeerMesh``) and a flag store behind it says so; step 3 waits for its
    G-1 flags on the stream; step 4 leaves the finished chunk in the owner's own buffer, and every rank's decode kernel READS the G finished
    chunks from their owners.  Against the collective transport that is one HBM write and one read of the wire bytes less per phase on every
    rank, no staging copy inside RCCL and no RCCL launch: 4 kernel launches + 2 flag stores + 2 flag waits per all-reduce.  One node only
    (IPC-mapped device memory); results are bit-identical to the collective transport (tests/test_gpu_distributed.py).

    ``group_size``: group-wise parameters on the wire (``quantized_all_reduce``); step 1 is one batched ``quantize_grouped`` launch, steps 3-4
    one ``reduce_quantize_grouped`` launch over the G-1 received chunks in increasing rank order, the decode one batched ``dequantize_grouped``
    launch.  Collective transport only.

    ``error_feedback``: the residual of ``quantized_all_reduce`` (the tensor's dtype, or float32 for a bfloat16 tensor) -- step 1 becomes one batched ``quantize_grouped_ef`` launch on the peers'
    chunks of the tensor and of the residual; the rank's own chunk of the residual is neither read nor written.

    ``error_feedback_requantize``: steps 3-4 become one ``reduce_quantize_grouped_ef`` launch on the rank's own chunk of the residual (added
    after the G-1 received chunks), which then holds what the owner's quantization lost; every slice of the residual is used.  A residual
    belongs to one (world size, rank, algorithm, ``error_feedback_requantize``).

    ``rotation_seed``: the rotated domain of ``quantized_all_reduce`` (the same seed on all ranks; not checked) -- step 1 is world - 1
    ``quantize_grouped_rotated`` launches, steps 3-4 ``dequantize_sum_grouped_rotated(..., 'add')`` into the own chunk and
    ``quantize_grouped_rotated`` of it (the steps of ``quantized_reduce_scatter`` and ``quantized_all_gather``: the same bytes), the decode world
    ``dequantize_grouped_rotated`` launches.  At most 17 ranks; not with ``error_feedback`` or ``transport='p2p'``.

    ``rotated_error_feedback``: the float32 rotated-domain residual of ``quantized_all_reduce`` -- step 1's launches become
    ``quantize_grouped_rotated_ef`` on the peers' chunks of it; with ``error_feedback_requantize`` the owner's ``quantize_grouped_rotated`` becomes
    ``quantize_grouped_rotated_ef`` on the rank's own chunk.  It belongs to one (world size, rank, algorithm, ``error_feedback_requantize``, seed,
    group size).
    """
    if not (tensor.is_contiguous() and tensor.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError('quantized_all_reduce needs a contiguous float32 or bfloat16 tensor')
    _check_clip_steps(clip_steps, group_size, all_reduce=True)
    _check_all_reduce_group_size(group_size, transport)
    _check_error_feedback(error_feedback, tensor, group_size, transport)
    _check_error_feedback_requantize(error_feedback_requantize, error_feedback if error_feedback is not None else rotated_error_feedback, group_size,
                                     transport)
    seed = _check_rotation_seed(rotation_seed, group_size, transport, error_feedback)
    _check_rotated_error_feedback(rotated_error_feedback, tensor, group_size, rotation_seed, transport, error_feedback)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    _check_rotated_terms(seed, world, 'the direct schedule')
    if world == 1 and not _single_rank_collectives:
        return tensor
    wire = _Wire(_ops or _DeviceOps(ctx), quant_dtype, round_mode, group_size, error_feedback if seed is None else rotated_error_feedback,
                 error_feedback_requantize, seed)
    flat = tensor.view(-1)
    ch = _Chunks.of(wire, flat, world)
    if transport == 'p2p':
        if world == 1:
            raise ValueError("transport='p2p' needs peers (a one-rank group has none)")
        return _all_reduce_direct_p2p(tensor, flat, ch.bounds, ch.slot, quant_dtype, wire.qdt, round_mode, group, ctx, wire.ops, world, rank, _p2p_timeout_us(timeout))
    if transport != 'collective':
        raise ValueError(f"transport must be 'collective' or 'p2p', got {transport!r}")
    terms = _mesh_scatter(wire, ch, group, world, rank, tensor.device)
    # ---- the owner's sum, quantized for the all-gather in the same launch (the sum itself is never stored: the final value of the
    # own chunk, too, comes from decoding the gathered bytes); with ``requantize`` it feeds the rank's own chunk of the residual ----
    mine = torch.zeros(ch.slot, dtype=torch.uint8, device=tensor.device)
    if ch.views[rank].numel():
        wire.owner_encode(terms, ch.views[rank], ch.record(mine, 0, rank), ch.bounds[rank])
    _mesh_gather(wire, ch, mine, group, world, tensor.device)
    return tensor


def _check_all_reduce_group_size(group_size, transport: str) -> None:
    """ValueError before anything moves: an invalid group size, or grouped parameters over the peer-to-peer transport."""
    if group_size is None:
        return
    from .torch import _check_group_size

    _check_group_size(group_size)
    if transport == 'p2p':
        raise ValueError("group_size= is not supported with transport='p2p' (its peer-mapped slots carry the per-chunk record); use transport='collective'")


def _check_error_feedback(residual, tensor: torch.Tensor, group_size, transport: str) -> None:
    """ValueError before anything moves: a residual without the grouped wire or over the peer-to-peer transport, or one that does not match the
    tensor (it is written by raw pointer)."""
    if residual is None:
        return
    if group_size is None:
        raise ValueError('error_feedback= needs the grouped wire: pass group_size= (the per-chunk wire has no error-feedback quantize)')
    if transport == 'p2p':
        raise ValueError("error_feedback= is not supported with transport='p2p'; use transport='collective'")
    from .torch import _check_residual

    _check_residual(residual, tensor, 'error_feedback')


def _check_error_feedback_requantize(requantize: bool, residual, group_size, transport: str) -> None:
    """ValueError before anything moves: error feedback on the re-quantizations without a residual, without the grouped wire or over the
    peer-to-peer transport."""
    if not requantize:
        return
    if residual is None:
        raise ValueError('error_feedback_requantize=True needs error_feedback= (the residual that takes what the re-quantizations lose)')
    if group_size is None:
        raise ValueError('error_feedback_requantize=True needs the grouped wire: pass group_size=')
    if transport == 'p2p':
        raise ValueError("error_feedback_requantize=True is not supported with transport='p2p'; use transport='collective'")


_ROTATED_MAX_TERMS = 16   # piquant_hip_reduce_quantize_grouped_rotated / piquant_hip_dequantize_sum_grouped_rotated: one launch, no spill


def _check_rotation_seed(seed, group_size, transport: str, error_feedback) -> Optional[int]:
    """ValueError before anything moves: a rotation without the grouped wire, over the peer-to-peer transport or with a residual (which lives in
    the original domain; ``rotated_error_feedback=`` is the residual that goes with a rotation).  Returns the seed modulo 2^64, or None."""
    if seed is None:
        return None
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise ValueError(f'rotation_seed must be an int or None, got {seed!r}')
    if group_size is None:
        raise ValueError('rotation_seed= needs the grouped wire: pass group_size= (whole groups are what is rotated)')
    if transport == 'p2p':
        raise ValueError("rotation_seed= is not supported with transport='p2p'; use transport='collective'")
    if error_feedback is not None:
        raise ValueError('rotation_seed= is not supported with error_feedback= (the residual lives in the original domain); '
                         'rotated_error_feedback= takes a float32 residual of the rotated domain')
    return seed & 0xFFFFFFFFFFFFFFFF


def _check_rotated_error_feedback(residual, tensor: torch.Tensor, group_size, rotation_seed, transport: str, error_feedback) -> None:
    """ValueError before anything moves: a rotated-domain residual without the grouped wire, without a rotation, over the peer-to-peer transport,
    next to ``error_feedback=`` (a residual of the original domain: a different object), or one that does not match the tensor -- float32 whatever
    the tensor's dtype, contiguous, of its device and numel (it is written by raw pointer)."""
    if residual is None:
        return
    if group_size is None:
        raise ValueError('rotated_error_feedback= needs the grouped wire: pass group_size=')
    if rotation_seed is None:
        raise ValueError('rotated_error_feedback= needs rotation_seed= (the residual holds values of that rotation; error_feedback= is the residual '
                         'of the original domain)')
    if transport == 'p2p':
        raise ValueError("rotated_error_feedback= is not supported with transport='p2p'; use transport='collective'")
    if error_feedback is not None:
        raise ValueError('rotated_error_feedback= cannot be combined with error_feedback= (one residual a call: of the rotated domain or of the '
                         'original one)')
    from .torch import _check_rotated_residual

    _check_rotated_residual(residual, tensor, 'rotated_error_feedback')


def _check_rotated_terms(seed, world: int, what: str) -> None:
    """ValueError before anything moves: the owner's step of a rotated mesh schedule is one launch over world - 1 records, at most 16."""
    if seed is not None and world - 1 > _ROTATED_MAX_TERMS:
        raise ValueError(f'rotation_seed= with {what} takes at most {_ROTATED_MAX_TERMS + 1} ranks (the owner sums world - 1 records in one launch), '
                         f'got {world}')


def _check_clip_steps(clip_steps, group_size, rotation_seed=None, error_feedback=None, rotated_error_feedback=None, transport: str = 'collective',
                      all_reduce: bool = False) -> None:
    """ValueError before anything moves: ``clip_steps`` is None or an int in [1, 12], on the grouped wire, where no partial sum is re-quantized
    and nothing else changes what is encoded."""
    if clip_steps is None:
        return
    if all_reduce:
        raise ValueError('clip_steps= is not supported by quantized_all_reduce: its ring hops and its owner step re-quantize partial sums, which needs '
                         'a clipped fused reduce; use quantized_reduce_scatter / quantized_all_gather')
    if not (isinstance(clip_steps, int) and not isinstance(clip_steps, bool) and 1 <= clip_steps <= 12):
        raise ValueError(f'clip_steps must be None or an int in [1, 12], got {clip_steps!r}')
    if group_size is None:
        raise ValueError('clip_steps= needs the grouped wire: pass group_size= (the search is per group)')
    if rotation_seed is not None:
        raise ValueError('clip_steps= is not supported with rotation_seed=')
    if error_feedback is not None or rotated_error_feedback is not None:
        raise ValueError('clip_steps= is not supported with error_feedback= or rotated_error_feedback= (the clipped mass would have to be carried forward)')
    if transport == 'p2p':
        raise ValueError("clip_steps= is not supported with transport='p2p'; use transport='collective'")


def _check_sharded_collective(name: str, tensor: torch.Tensor, group_size, error_feedback) -> None:
    """ValueError before anything moves, for ``quantized_reduce_scatter`` and ``quantized_all_gather``: the tensor, a group size that is no group
    size (``None`` included: they have the grouped wire only) and a residual that does not match the tensor."""
    if not (isinstance(tensor, torch.Tensor) and tensor.is_contiguous() and tensor.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError(f'{name} needs a contiguous float32 or bfloat16 tensor')
    if group_size is None:
        raise ValueError(f'{name} has the grouped wire only: group_size= must be a power of two in [32, 4096], got None')
    _check_all_reduce_group_size(group_size, 'collective')
    _check_error_feedback(error_feedback, tensor, group_size, 'collective')


def quantized_reduce_scatter(
    tensor: torch.Tensor,
    *,
    quant_dtype: torch.dtype = torch.uint8,
    round_mode: str = 'nearest',
    group: Optional[dist.ProcessGroup] = None,
    ctx: Optional[Context] = None,
    group_size: int = 128,
    error_feedback: Optional[torch.Tensor] = None,
    rotation_seed: Optional[int] = None,
    rotated_error_feedback: Optional[torch.Tensor] = None,
    clip_steps: Optional[int] = None,
    _ops=None,
    _single_rank_collectives: bool = False,
) -> torch.Tensor:
    """SUM reduce-scatter of a contiguous float32/bfloat16 tensor over the grouped wire: the reduce-scatter half of
    ``quantized_all_reduce(algorithm='direct', group_size=...)`` on its own, for sharded data parallelism and for an outer optimizer that owns
    one shard.  The chunks are ``ring_chunks(numel, world, bits)`` and chunk r belongs to rank r.  Collective transport only.

    1. ONE batched ``quantize_grouped`` launch encodes this rank's values of every peer's chunk (``grouped_wire_layout`` records),
    2. ONE all-to-all delivers them,
    3. ONE ``dequantize_sum_grouped(..., 'add')`` launch adds the world - 1 received records, in increasing rank order, into the rank's own chunk
       of ``tensor``, in one pass over it.

    Returns the view ``tensor.view(-1)[b_r:e_r]`` of the rank's own chunk (empty when the tensor is shorter than the chunks in front of it), now
    holding the sum in full precision: every peer's contribution was quantized once, the owner's own values never, and the sum is not quantized
    again.  The other chunks of ``tensor`` are left as they were.  Two kernel launches per call.

    ``error_feedback``: the residual of ``quantized_all_reduce`` (the tensor's dtype, device and numel; float32 also for a bfloat16 tensor).  Step 1
    becomes one batched ``quantize_grouped_ef`` launch on the peers' chunks of the tensor and of the residual; the rank's own chunk of the
    residual is neither read nor written.  EVERY quantization this collective performs is covered by ``error_feedback``: there is no
    re-quantization of a partial sum here, so there is nothing for an ``error_feedback_requantize`` to add.

    ``quantized_reduce_scatter`` followed by ``quantized_all_gather`` on the same inputs leaves exactly the bytes of
    ``quantized_all_reduce(algorithm='direct', group_size=group_size)``: that schedule's ``reduce_quantize_grouped`` is defined as these ADDs
    followed by ``quantize_grouped``.

    ``rotation_seed`` (the same int on all ranks; not checked): the peers' chunks are encoded by ONE ``quantize_grouped_rotated_batch``
    launch per 16 chunks,
    and step 3 is ONE ``dequantize_sum_grouped_rotated(..., 'add')`` launch: the received records are summed in float32 in the rotated domain
    and the sum is rotated back once and added into the own chunk.  Followed by ``quantized_all_gather`` with the same seed it leaves exactly the bytes
    of ``quantized_all_reduce(algorithm='direct', rotation_seed=...)``, whose owner's step is these two.  At most 17 ranks; not with ``error_feedback``.

    ``rotated_error_feedback`` (``rotation_seed`` only): the float32 rotated-domain residual of ``quantized_all_reduce``; the peers' chunks are
    encoded by ONE ``quantize_grouped_rotated_ef_batch`` launch per 16 on their chunks of it, the rank's own chunk of it is neither read nor written.  Followed by
    ``quantized_all_gather`` with the same residual it leaves exactly the tensor bytes and residual bytes of ``quantized_all_reduce(algorithm='direct',
    error_feedback_requantize=True)``.  The residual belongs to one (world size, rank, seed, group size).

    ``clip_steps`` (None, or an int in [1, 12]; the same value on all ranks, not checked): step 1 becomes ONE ``quantize_grouped_clipped_batch``
    launch per 16 chunks -- every group of every record is quantized with the best of ``clip_steps`` shrunk ranges (``piquant.torch.quantize_grouped_clipped``);
    the records, the all-to-all and step 3 are unchanged.  Not with ``rotation_seed``, ``error_feedback`` or ``rotated_error_feedback``.

    ``group_size`` must be a group size (``None`` raises); every argument check raises ValueError before anything moves.  A one-rank group
    returns at once (``_ops`` and ``_single_rank_collectives`` as in ``quantized_all_reduce``).  (Unmeasured on more than one GPU, like the rest
    of this module's multi-GPU paths.)"""
    _check_sharded_collective('quantized_reduce_scatter', tensor, group_size, error_feedback)
    seed = _check_rotation_seed(rotation_seed, group_size, 'collective', error_feedback)
    _check_rotated_error_feedback(rotated_error_feedback, tensor, group_size, rotation_seed, 'collective', error_feedback)
    _check_clip_steps(clip_steps, group_size, rotation_seed, error_feedback, rotated_error_feedback)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    _check_rotated_terms(seed, world, 'quantized_reduce_scatter')
    flat = tensor.view(-1)
    if world == 1 and not _single_rank_collectives:
        b_own, e_own = ring_chunks(flat.numel(), world, torch_to_piquant_dtype(quant_dtype).bit_size)[rank]
        return flat[b_own:e_own]
    wire = _Wire(_ops or _DeviceOps(ctx), quant_dtype, round_mode, group_size, error_feedback if seed is None else rotated_error_feedback,
                 rotation_seed=seed, clip_steps=clip_steps)
    ch = _Chunks.of(wire, flat, world)
    x_own = ch.views[rank]
    terms = _mesh_scatter(wire, ch, group, world, rank, tensor.device)
    if x_own.numel() and terms:
        wire.decode_sum(terms, x_own, 'add')
    return x_own


def quantized_all_gather(
    tensor: torch.Tensor,
    *,
    quant_dtype: torch.dtype = torch.uint8,
    round_mode: str = 'nearest',
    group: Optional[dist.ProcessGroup] = None,
    ctx: Optional[Context] = None,
    group_size: int = 128,
    error_feedback: Optional[torch.Tensor] = None,
    rotation_seed: Optional[int] = None,
    rotated_error_feedback: Optional[torch.Tensor] = None,
    clip_steps: Optional[int] = None,
    _ops=None,
    _single_rank_collectives: bool = False,
) -> torch.Tensor:
    """In-place all-gather of a contiguous float32/bfloat16 tensor over the grouped wire: the all-gather half of
    ``quantized_all_reduce(algorithm='direct', group_size=...)`` on its own.  The chunks are ``ring_chunks(numel, world, bits)``; rank r's chunk r
    of ``tensor`` is its input, whatever its other chunks hold.  Collective transport only.

    1. ONE ``quantize_grouped`` launch encodes the rank's own chunk (a ``grouped_wire_layout`` record),
    2. ONE all-gather distributes the records,
    3. ONE batched ``dequantize_grouped(..., 'set')`` launch stores all chunks into ``tensor`` -- the own chunk included, from the same bytes
       every other rank decodes, so all ranks end bit-identical.

    Returns ``tensor``.  ``error_feedback`` (as in ``quantized_reduce_scatter``): step 1 becomes ``quantize_grouped_ef`` on the rank's own chunk of
    the residual; no other chunk of it is touched.  A residual belongs to one collective, world size and rank: do not share one between
    ``quantized_reduce_scatter`` (which uses the peers' chunks) and this call unless that is the intent -- together the two touch every chunk
    exactly once, as ``quantized_all_reduce`` with ``error_feedback_requantize`` does.

    ``rotation_seed`` (the same int on all ranks; not checked): step 1 is ``quantize_grouped_rotated``, step 3 ONE
    ``dequantize_grouped_rotated_batch(..., 'set')`` launch per 16 chunks.  Not with ``error_feedback``.

    ``rotated_error_feedback`` (``rotation_seed`` only): the float32 rotated-domain residual of ``quantized_all_reduce``; step 1 becomes
    ``quantize_grouped_rotated_ef`` on the rank's own chunk of it, no other chunk is touched.  It belongs to one (world size, rank, seed, group
    size).

    ``clip_steps`` (as in ``quantized_reduce_scatter``): step 1 becomes ``quantize_grouped_clipped`` on the rank's own chunk; steps 2 and 3 are
    unchanged.  Not with ``rotation_seed``, ``error_feedback`` or ``rotated_error_feedback``.

    ``group_size`` must be a group size (``None`` raises); every argument check raises ValueError before anything moves.  A one-rank group
    returns at once (``_ops`` and ``_single_rank_collectives`` as in ``quantized_all_reduce``).  (Unmeasured on more than one GPU.)"""
    _check_sharded_collective('quantized_all_gather', tensor, group_size, error_feedback)
    seed = _check_rotation_seed(rotation_seed, group_size, 'collective', error_feedback)
    _check_rotated_error_feedback(rotated_error_feedback, tensor, group_size, rotation_seed, 'collective', error_feedback)
    _check_clip_steps(clip_steps, group_size, rotation_seed, error_feedback, rotated_error_feedback)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if world == 1 and not _single_rank_collectives:
        return tensor
    wire = _Wire(_ops or _DeviceOps(ctx), quant_dtype, round_mode, group_size, error_feedback if seed is None else rotated_error_feedback,
                 rotation_seed=seed, clip_steps=clip_steps)
    ch = _Chunks.of(wire, tensor.view(-1), world)
    mine = torch.zeros(ch.slot, dtype=torch.uint8, device=tensor.device)
    if ch.views[rank].numel():
        wire.encode(ch.views[rank], ch.record(mine, 0, rank), ch.bounds[rank])
    _mesh_gather(wire, ch, mine, group, world, tensor.device)
    return tensor


def _all_reduce_direct_p2p(tensor, flat, chunks, slot, quant_dtype, qdt, round_mode, group, ctx, ops, world, rank, timeout_us=0):
    """The mesh schedule over peer-mapped buffers (``quantized_all_reduce_direct``, ``transport='p2p'``).  The calls go through the context's
    raw-pointer entry points: the peers' buffers are addresses of THEIR devices' memory, which the tensor-level wrappers (one device per
    call, by design) would refuse."""
    if not tensor.is_cuda:
        raise RuntimeError("transport='p2p' moves device memory between GPUs: the tensor must live on one")
    slot = -(-slot // 65536) * 65536    # coarse sizes: a mesh is grown (an IPC exchange and a barrier) only when a tensor needs more than any before it
    mesh = _PeerMesh.get(group, tensor.device, slot, world, rank)      # its own slot size lays the buffers out (>= what this tensor needs)
    cx = _ctx_for(tensor, ctx)          # the tensor's device, PyTorch's current stream, stream-ordered
    _raise_peer_timeout(cx, "an earlier quantized_all_reduce(transport='p2p')")
    if mesh.poisoned:
        raise RuntimeError("quantized_all_reduce(transport='p2p'): an earlier exchange of this group gave up on a late rank, whose stores may still land in the "
                           "peer-mapped buffers; every rank must call piquant.distributed.release_peer_meshes(group) before the group uses transport='p2p' again")
    with mesh.order.lock:               # one exchange of a mesh at a time on the host, whatever thread it comes from ...
        mesh.order.enter(tensor.device)     # ... and behind the mesh's previous exchange on the device, whatever stream that ran on
        _all_reduce_direct_p2p_locked(tensor, flat, chunks, mesh, cx, qdt, round_mode, world, rank, timeout_us)
        mesh.order.leave(tensor.device)
    return tensor


def _all_reduce_direct_p2p_locked(tensor, flat, chunks, mesh, cx, qdt, round_mode, world, rank, timeout_us):
    from . import ReduceOp, RoundMode

    slot = mesh.slot
    fdt = torch_to_piquant_dtype(tensor.dtype)
    rmode = RoundMode.NEAREST if round_mode == 'nearest' else RoundMode.STOCHASTIC
    mesh.seq += 1
    seq, par = mesh.seq, mesh.seq & 1
    esize = tensor.element_size()
    base = flat.data_ptr()

    def chunk_ptr(j):
        return base + chunks[j][0] * esize

    def chunk_len(j):
        return chunks[j][1] - chunks[j][0]

    def recv_ptr(j, i):                 # recv[par][i] of rank j: 16-byte header (the parameter record), then the packed bytes
        return mesh.data.ptrs[j] + (par * world + i) * slot

    def mine_ptr(j):
        return mesh.data.ptrs[j] + mesh.off_mine + par * slot

    def wait_for_everybody(offset):     # ONE wait over all `world` flags (the own one is signalled with the peers'): flag index == rank, which is what a timeout reports
        cx.wait_flags_ptr(mesh.flags.own + offset, world, seq, timeout_us)

    peers = [j for j in range(world) if j != rank]
    everybody = list(range(world))
    # ---- 1. every peer's chunk, quantized straight into that peer's recv[par][rank]; then the flags ----
    full = [j for j in peers if chunk_len(j) > 0]
    cx.quantize_dynamic_batch_ptr([chunk_ptr(j) for j in full], fdt, [recv_ptr(j, rank) + _HEADER_BYTES for j in full], qdt, [chunk_len(j) for j in full],
                                  [recv_ptr(j, rank) for j in full], rmode, _device_ptrs=True)
    cx.signal_flags_ptr([mesh.flag_ptr(j, 'arrived', rank) for j in everybody], seq)
    # ---- 2./3. wait for the G-1 chunks of MY range, add them to my own values, quantize the finished chunk into mine[par] ----
    wait_for_everybody(mesh.off_arrived)
    if chunk_len(rank) > 0:
        cx.reduce_quantize_dynamic_ptr(chunk_ptr(rank), fdt, [recv_ptr(rank, i) + _HEADER_BYTES for i in peers], [recv_ptr(rank, i) for i in peers],
                                       mine_ptr(rank) + _HEADER_BYTES, qdt, chunk_len(rank), mine_ptr(rank), rmode, _device_ptrs=True)
    cx.signal_flags_ptr([mesh.flag_ptr(j, 'finished', rank) for j in everybody], seq)
    # ---- 4. every finished chunk, read from its owner (the own one from this rank's buffer: all ranks decode the same bytes) ----
    wait_for_everybody(mesh.off_finished)
    everyone = [j for j in range(world) if chunk_len(j) > 0]
    cx.dequantize_dp_batch_ptr([mine_ptr(j) + _HEADER_BYTES for j in everyone], qdt, [chunk_ptr(j) for j in everyone], fdt, [chunk_len(j) for j in everyone],
                               [mine_ptr(j) for j in everyone], ReduceOp.SET, _device_ptrs=True)


def check_peer_timeouts(device: Optional[torch.device] = None, ctx: Optional[Context] = None) -> None:
    """Synchronises the device and raises RuntimeError if a wait of a ``transport='p2p'`` call issued on it ran out (the asynchronous all-reduce
    cannot raise by itself: a late rank is found at the next p2p call, or here)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    torch.cuda.synchronize(device)
    _raise_peer_timeout(ctx if ctx is not None else Context.get(device.index), "quantized_all_reduce / compute_quant_params (transport='p2p')")
