"""Cases, model and fault models of the host-memory calls at their seams (tests/test_gpu_host_boundary.py, tests/test_host_boundary_cases_cpu.py).

A call whose buffers are pageable host memory is either handed to libpiquant_cpu.so or staged over PCIe in chunks of C = 2^24 elements on two
alternating stage slots (csrc/capi.cpp).  Every kernel behind these calls is position independent (FORM_UNIFORM), so the model of a call is ONE
oracle call over the whole tensor: O.quantize, O.quantize_per_element, O.dequantize, O.compute_quant_params.

The inputs are made so that a staging loop that goes wrong at a seam changes the result:
  * every chunk differs from every other (a slow ramp times noise; random bytes for the quantized side),
  * at C - 1, C, C + 1, 2C - 1, 2C and n - 1 sit a half-step tie, NaN, +inf, -inf, -0.0 and a denormal (a tensor of two chunks has no 2C - 1
    and 2C: those two values move to C - 2 and C + 2), and an ADD accumulator carries NaN, +-inf and -0.0 at the same places,
  * N2 ends inside a packed byte of uint4 and of uint2, N3 has three chunks, so stage slot 0 is used twice.

`staged_quantize`, `staged_dequantize` and `staged_scan` restate the staging loop over the oracle, chunk by chunk, with ONE fault switched on
(FAULTS).  Without a fault they give the whole-call model; tests/test_host_boundary_cases_cpu.py proves that each fault changes the bytes, the
floats or the parameters of a case the GPU file runs.
"""
from functools import lru_cache

import numpy as np

import oracle as O

C = 1 << 24                # kStageChunkElems (csrc/context.hpp); the CPU test reads the header and compares
N2 = C + 4099              # two chunks; 4099 = 2 * 2049 + 1 = 4 * 1024 + 3: the tail ends inside a packed byte of uint4 and uint2
N3 = 2 * C + 37            # three chunks: slot 0 is reused
M64 = (1 << 64) - 1

F32, BF16, UINT2, UINT4, UINT8 = O.F32, O.BF16, O.UINT2, O.UINT4, O.UINT8
BITS = {UINT8: 8, UINT4: 4, UINT2: 2}
PACK = {UINT8: 1, UINT4: 2, UINT2: 4}
ESIZE = {F32: 4, BF16: 2}
NP_OF = {F32: np.float32, BF16: np.uint16}
NAME = {F32: "fp32", BF16: "bf16", UINT8: "uint8", UINT4: "uint4", UINT2: "uint2"}

QUANT_PAIRS = [(f, q) for f in (F32, BF16) for q in (UINT8, UINT4, UINT2)]
DEQUANT_FORMS = [(q, f, op) for q in (UINT8, UINT4, UINT2) for f in (F32, BF16) for op in (O.SET, O.ADD)]

# power-of-two scales: 2.5 * scale is exact in fp32 and in bf16, so the planted tie is a tie (x / scale = 2.5) for both input types
QUANT_PARAMS = {UINT8: (2.0 ** -7, 128), UINT4: (2.0 ** -3, 8), UINT2: (0.5, 2)}
DEQUANT_PARAMS = {UINT8: (0.0123, 131), UINT4: (0.2, 7), UINT2: (0.7, 1)}
TAU = 0.37                 # the pinned per-call threshold
TAU_REDRAWN = 0.81         # what the fault "threshold redrawn for the second chunk" draws
SEED = 0x5EED5EED1234
INDEX_BASE = (1 << 32) - C - 2000   # index 2^32 falls 2000 elements into the second chunk of N2
INDEX_BASE_BELOW = (1 << 32) - C - 5000   # every index of N2 stays below 2^32, the last one by 902

NEAREST = ("nearest",)
STOCHASTIC = ("call", TAU)
PER_ELEMENT = ("element", SEED, INDEX_BASE)
PER_ELEMENT_BELOW = ("element", SEED, INDEX_BASE_BELOW)

FAULTS = ("index_restarted", "threshold_redrawn", "stale_slot", "acc_not_uploaded", "acc_from_offset_0", "tail_byte_dropped", "seam_early", "seam_late",
          "device_offset_twice", "device_offset_missing", "scan_chunk_left_out", "scan_last_chunk_only")


def packed(n, dt_q):
    return (n + PACK[dt_q] - 1) // PACK[dt_q]


def seam_positions(n):
    """six positions, one per planted value; the seams a tensor does not have fold back to its first seam"""
    assert n > C + 8
    return [C - 1, C, C + 1, 2 * C - 1 if 2 * C - 1 < n - 1 else C - 2, 2 * C if 2 * C < n - 1 else C + 2, n - 1]


@lru_cache(maxsize=2)
def _ramp_times_noise(n):
    u = np.random.default_rng(n).random(n, dtype=np.float32)
    u *= 2.0
    u -= 1.0
    u *= np.linspace(0.25, 1.0, n, dtype=np.float32)
    u.setflags(write=False)
    return u


def _frozen(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=3)
def quant_input(n, dt_f, dt_q):
    """the tensor a quantize case reads: |x| <= 1, every chunk different, the six edge values at the seams"""
    scale, _ = QUANT_PARAMS[dt_q]
    x = _ramp_times_noise(n).copy()
    x[seam_positions(n)] = np.array([2.5 * scale, np.nan, np.inf, -np.inf, -0.0, 1e-40], dtype=np.float32)
    return _frozen(x if dt_f == F32 else O.f32_to_bf16(x))


@lru_cache(maxsize=3)
def codes_input(n, dt_q):
    return _frozen(np.random.default_rng(n + BITS[dt_q]).integers(0, 256, packed(n, dt_q), dtype=np.uint8))


@lru_cache(maxsize=3)
def accumulator(n, dt_f):
    """what an ADD adds to (and what a SET overwrites): NaN, +-inf and -0.0 at the seams"""
    a = _ramp_times_noise(n) * np.float32(3.0)
    a[seam_positions(n)] = np.array([np.nan, np.inf, -np.inf, -0.0, np.nan, np.inf], dtype=np.float32)
    return _frozen(a if dt_f == F32 else O.f32_to_bf16(a))


# ---- the scan: one minimum and one maximum, at the seams
SCAN_MIN, SCAN_MAX = -7.5, 9.25       # exact in bf16


def scan_positions(n):
    return [0, C - 1, C, 2 * C - 1, 2 * C, n - 1]


def scan_pairs(n):
    """(position of the minimum, position of the maximum): every chunk of N3 holds each extremum at least once"""
    p = scan_positions(n)
    return [(p[0], p[2]), (p[1], p[4]), (p[2], p[5]), (p[3], p[0]), (p[4], p[1]), (p[5], p[3])]


@lru_cache(maxsize=2)
def _scan_base(n, dt_f):
    x = _ramp_times_noise(n).copy()
    x[::1_000_003] = np.nan
    x[[C - 2, C + 1, 2 * C - 2, 2 * C + 1]] = np.nan        # NaNs next to the seams too
    return _frozen(x if dt_f == F32 else O.f32_to_bf16(x))


def scan_input(n, dt_f, pos_min, pos_max):
    x = _scan_base(n, dt_f).copy()
    lo, hi = np.array([SCAN_MIN, SCAN_MAX], dtype=np.float32)
    x[pos_min], x[pos_max] = (lo, hi) if dt_f == F32 else O.f32_to_bf16(np.array([lo, hi]))
    return x


# ---- the model: one oracle call over the whole tensor
def quantize_model(x, dt_f, dt_q, rounding, scale=None, zp=None):
    s, z = QUANT_PARAMS[dt_q]
    scale, zp = (s if scale is None else scale), (z if zp is None else zp)
    if rounding[0] == "nearest":
        return O.quantize(x, dt_f, dt_q, scale, zp, O.NEAREST, 0.0, form=O.FORM_UNIFORM)
    if rounding[0] == "call":
        return O.quantize(x, dt_f, dt_q, scale, zp, O.STOCHASTIC, rounding[1], form=O.FORM_UNIFORM)
    return O.quantize_per_element(x, dt_f, dt_q, scale, zp, rounding[1], rounding[2] & M64)


def dequantize_model(q, dt_q, dt_f, n, op, acc):
    """acc: the previous contents of the output (copied); SET overwrites all of it"""
    scale, zp = DEQUANT_PARAMS[dt_q]
    return O.dequantize(q, dt_q, dt_f, n, scale, zp, op, form=O.FORM_UNIFORM, out=acc.copy())


def scan_model(x, dt_f, target):
    return O.compute_quant_params(x, dt_f, target)


# ---- the staging loop of csrc/capi.cpp restated over the oracle, one fault at a time
def _chunk_of(fault):
    return C + {"seam_early": -1, "seam_late": 1}.get(fault, 0)


def _read(buf, begin, count):
    """count items of a device buffer from `begin`; past its end a wrong offset finds other memory (zeros here)"""
    got = np.zeros(count, dtype=buf.dtype)
    have = buf[begin: begin + count]
    got[: have.size] = have
    return got


def _device_offset(fault, off):
    return {"device_offset_twice": 2 * off, "device_offset_missing": 0}.get(fault, off)


def staged_quantize(x, dt_f, dt_q, rounding, fault=None, device=None, prefill=0xAA):
    """device: None (both buffers pageable), 'in' or 'out' (that side lives in device memory and is addressed by offset)"""
    assert fault is None or fault in FAULTS
    n, (scale, zp), chunk = x.size, QUANT_PARAMS[dt_q], min(x.size, _chunk_of(fault))
    out = np.full(packed(n, dt_q), prefill, dtype=np.uint8)
    slot_in = [None, None]
    for k, off in enumerate(range(0, n, chunk)):
        m, slot = min(chunk, n - off), k & 1
        if device == "in":
            xs = _read(x, _device_offset(fault, off), m)
        else:
            xs = x[off: off + m]
            if fault == "stale_slot" and slot_in[slot] is not None:
                xs = slot_in[slot][:m]       # the copy in never landed: the slot still holds the chunk before last
            else:
                slot_in[slot] = xs
        r = rounding
        if r[0] == "element":
            r = ("element", r[1], r[2] + (0 if fault == "index_restarted" else off))
        elif r[0] == "call" and fault == "threshold_redrawn" and k == 1:
            r = ("call", TAU_REDRAWN)
        got = quantize_model(xs, dt_f, dt_q, r, scale, zp)
        nbytes = got.size - (1 if fault == "tail_byte_dropped" and off + m == n and m % PACK[dt_q] else 0)
        at = packed(off, dt_q)
        if device == "out":
            at = _device_offset(fault, at)
        nbytes = max(0, min(nbytes, out.size - at))   # a wrong offset writes other memory: nothing of it arrives here
        out[at: at + nbytes] = got[:nbytes]
    return out


def staged_dequantize(q, dt_q, dt_f, n, op, acc, fault=None, device=None):
    assert fault is None or fault in FAULTS
    scale, zp = DEQUANT_PARAMS[dt_q]
    chunk = min(n, _chunk_of(fault))
    out = acc.copy()
    slot_in, slot_out = [None, None], [np.zeros(chunk, dtype=acc.dtype), np.zeros(chunk, dtype=acc.dtype)]
    for k, off in enumerate(range(0, n, chunk)):
        m, slot = min(chunk, n - off), k & 1
        begin, nbytes = packed(off, dt_q), packed(m, dt_q)
        if device == "in":
            qs = _read(q, _device_offset(fault, begin), nbytes)
        else:
            qs = q[begin: begin + nbytes]
            if fault == "stale_slot" and slot_in[slot] is not None:
                qs = slot_in[slot][:nbytes]
            else:
                slot_in[slot] = qs
        if fault == "tail_byte_dropped" and off + m == n and m % PACK[dt_q]:
            qs = qs.copy()
            qs[-1] = 0                        # the last byte never travelled
        at = _device_offset(fault, off) if device == "out" else off
        if device == "out":
            prev = _read(out, at, m)          # the kernel adds in place, wherever the offset points
        elif fault == "acc_not_uploaded":
            prev = slot_out[slot][:m].copy()
        elif fault == "acc_from_offset_0":
            prev = acc[:m].copy()
        else:
            prev = acc[off: off + m].copy()
        got = O.dequantize(qs, dt_q, dt_f, m, scale, zp, op, form=O.FORM_UNIFORM, out=prev)
        slot_out[slot][:m] = got
        count = max(0, min(m, n - at))
        out[at: at + count] = got[:count]
    return out


def staged_scan(x, dt_f, target, fault=None, left_out=0):
    """min/max chunk by chunk, folded once at the end"""
    n = x.size
    parts = [O.minmax(x[off: off + C], dt_f) for off in range(0, n, C)]
    if fault == "scan_chunk_left_out":
        del parts[left_out]
    elif fault == "scan_last_chunk_only":
        parts = parts[-1:]
    return O.quant_params_from_minmax(min(p[0] for p in parts), max(p[1] for p in parts), target)
