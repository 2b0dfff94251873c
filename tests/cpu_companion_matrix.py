"""Child process of tests/test_cpu_companion_seams.py: libpiquant_cpu.so against the oracle over a matrix of sizes, pairs and buffer offsets.

    python tests/cpu_companion_matrix.py quantize|dequantize|natural_quantize|natural_dequantize avx512|scalar THREADS

The library reads PIQUANT_CPU_NT_STORES once per process (1: every call streams its output past the caches, 0: none does, unset: outputs of 4 MiB
and more do), so each arm of the matrix needs a process of its own; the parent sets the variable.  Sizes sit around the 65 536-element chunks the
pool hands out (one chunk, one more element, THREADS chunks +- 1, more chunks than workers); output offsets reach every head length of the
streaming bodies (quantize: bytes up to a 16-byte line; dequantize: elements up to a 64- or 32-byte line, 1 and 3 of them being no whole packed
byte of uint4 / uint2, which is the kernel's fallback to ordinary stores).  Exit status 0: every comparison was exact; 77: no AVX-512 on this host.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "pi-quant_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import oracle as O                      # noqa: E402
from helpers import same_floats         # noqa: E402
from piquant import cpu                 # noqa: E402

CHUNK = 65536                           # kChunkElems (csrc/cpu/piquant_cpu.cpp)
FILL = 0xAA
TAU = 0.37
QMAX = {O.UINT8: 255, O.UINT4: 15, O.UINT2: 3}
PACK = {O.UINT8: 1, O.UINT4: 2, O.UINT2: 4}
NP_OF = {O.F32: np.float32, O.BF16: np.uint16}
QUANT_OFFSETS = [(0, 0), (1, 0), (5, 1), (15, 1), (0, 1)]      # (output bytes off a 64-byte boundary, input elements off one)
DEQUANT_OFFSETS = [0, 1, 3, 8]                                  # output elements off a 64-byte boundary


def sizes(threads):
    return sorted({1, 17, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, threads * CHUNK - 1, threads * CHUNK + 1, 14 * CHUNK + 33})


def guarded(nbytes, misalign):
    """-> (whole buffer, payload view): nbytes that start `misalign` bytes behind a 64-byte boundary, 0xAA around them"""
    raw = np.full(nbytes + misalign + 3 * 64, FILL, dtype=np.uint8)
    begin = (-raw.ctypes.data) % 64 + 64 + misalign
    return raw, raw[begin: begin + nbytes]


def guards_intact(raw, view):
    begin = view.ctypes.data - raw.ctypes.data
    return bool((raw[:begin] == FILL).all() and (raw[begin + view.size:] == FILL).all())


def placed(a, elements_off):
    """a copy of `a` that starts `elements_off` elements behind a 64-byte boundary"""
    raw, view = guarded(a.nbytes, elements_off * a.itemsize)
    view[:] = a.view(np.uint8)
    return raw, view.view(a.dtype)


def fail(*what):
    print("MISMATCH", *what, flush=True)
    sys.exit(1)


def data(rng, n):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if n > 60:
        x[rng.choice(n, 7, replace=False)] = [np.nan, np.inf, -np.inf, 1e30, -3e9, 0.49999997, -0.0]
        x[[0, n - 1]] = [0.5 / 127.5 * 5, 1e-40]
    return x


def quantize_matrix(ctx, threads, ns=None, offsets=QUANT_OFFSETS, roundings=((0, 0.0), (1, TAU))):
    rng = np.random.default_rng(threads)
    checked = 0
    for k, n in enumerate(ns or sizes(threads)):
        x = data(rng, n)
        for dt_in, xin in ((O.F32, x), (O.BF16, O.f32_to_bf16(x))):
            sources = {off: placed(xin, off) for off in {o[1] for o in offsets}}
            for dt_out in (O.UINT8, O.UINT4, O.UINT2):
                scale = float(np.float32(2.0 / QMAX[dt_out]))
                zp = (QMAX[dt_out] // 2, -3, QMAX[dt_out] + 10, 2 ** 40 + 5)[k % 4] if n > 60 else QMAX[dt_out] // 2
                for rm, tau in roundings:
                    want = O.quantize(xin, dt_in, dt_out, scale, zp, rm, tau, form=O.FORM_UNIFORM)
                    for out_off, in_off in offsets:
                        raw, out = guarded(want.size, out_off)
                        src = sources[in_off][1]
                        ctx.quantize_ptr(src.ctypes.data, dt_in, out.ctypes.data, dt_out, n, scale, zp, rm, tau)
                        if not np.array_equal(out, want):
                            fail("quantize", threads, n, dt_in, dt_out, rm, out_off, in_off, np.flatnonzero(out != want)[:5])
                        if not guards_intact(raw, out) or not np.array_equal(src.view(np.uint8), xin.view(np.uint8)):
                            fail("quantize wrote outside its output or changed its input", threads, n, dt_in, dt_out, rm, out_off, in_off)
                        checked += 1
    return checked


def dequantize_matrix(ctx, threads, ns=None, offsets=DEQUANT_OFFSETS, ops=(O.SET, O.ADD)):
    rng = np.random.default_rng(100 + threads)
    checked = 0
    for k, n in enumerate(ns or sizes(threads)):
        prev32 = rng.uniform(-3, 3, n).astype(np.float32)
        if n > 60:
            prev32[rng.choice(n, 4, replace=False)] = [np.nan, np.inf, -np.inf, -0.0]
        for dt_q in (O.UINT8, O.UINT4, O.UINT2):
            q = rng.integers(0, 256, O.packed_numel(n, dt_q), dtype=np.uint8)
            zp = (9, -4, 2 ** 33 + 1)[k % 3]
            for dt_f in (O.F32, O.BF16):
                prev = prev32 if dt_f == O.F32 else O.f32_to_bf16(prev32)
                for op in ops:
                    want = O.dequantize(q, dt_q, dt_f, n, 0.02, zp, op, form=O.FORM_UNIFORM, out=prev.copy())
                    for off in offsets:
                        raw, out = placed(prev, off)
                        ctx.dequantize_ptr(q.ctypes.data, dt_q, out.ctypes.data, dt_f, n, 0.02, zp, op)
                        if not same_floats(out, want):
                            fail("dequantize", threads, n, dt_q, dt_f, op, off)
                        if not guards_intact(raw, out.view(np.uint8)):
                            fail("dequantize wrote outside its output", threads, n, dt_q, dt_f, op, off)
                        checked += 1
    return checked


MiB4 = 4 << 20                          # kStreamOutputBytes (csrc/cpu/piquant_cpu.cpp)


def natural_quantize(ctx, threads):
    """no override: outputs of 4 MiB - 1 byte and of 4 MiB, so both sides of the library's own threshold run under the checker"""
    assert "PIQUANT_CPU_NT_STORES" not in os.environ
    checked = quantize_matrix(ctx, threads, ns=[MiB4 - 1, MiB4], offsets=[(0, 0), (5, 1)], roundings=((0, 0.0),))       # uint8: 4 MiB - 1 and 4 MiB bytes
    return checked + quantize_matrix(ctx, threads, ns=[2 * MiB4 - 2, 2 * MiB4], offsets=[(1, 0)], roundings=((0, 0.0),))  # uint4: the same two


def natural_dequantize(ctx, threads):
    assert "PIQUANT_CPU_NT_STORES" not in os.environ
    checked = dequantize_matrix(ctx, threads, ns=[MiB4 // 4 - 1, MiB4 // 4], offsets=[0, 8], ops=(O.SET,))               # fp32: 4 MiB - 4 bytes and 4 MiB
    return checked + dequantize_matrix(ctx, threads, ns=[MiB4 // 2 - 1, MiB4 // 2], offsets=[0, 3], ops=(O.SET,))         # bf16: 4 MiB - 2 bytes and 4 MiB


KINDS = {"quantize": quantize_matrix, "dequantize": dequantize_matrix, "natural_quantize": natural_quantize, "natural_dequantize": natural_dequantize}


def main():
    kind, form, threads = sys.argv[1], sys.argv[2], int(sys.argv[3])
    assert kind in KINDS and form in ("avx512", "scalar") and 1 <= threads <= 16
    if form == "avx512" and not cpu.use_avx512(True):
        print("no AVX-512 on this host")
        sys.exit(77)
    cpu.use_avx512(form == "avx512")
    ctx = cpu.CpuContext(threads)
    checked = KINDS[kind](ctx, threads)
    ctx.close()
    print(f"checked {checked}")


if __name__ == "__main__":
    main()
