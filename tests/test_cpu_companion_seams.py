"""CPU: libpiquant_cpu.so at its own seams -- the non-temporal store branches (forced on and off, and around the library's own 4 MiB
threshold), the chunked work hand-out with more workers than elements and with the number of active workers changed between calls, the
caller's affinity mask after a pinned call, and concurrent callers.  Everything against the oracle, exactly; the matrix itself lives in
tests/cpu_companion_matrix.py, which runs in a child process because PIQUANT_CPU_NT_STORES is read once per process."""
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

from helpers import same_floats

ROOT = Path(__file__).resolve().parent.parent
MATRIX = Path(__file__).resolve().parent / "cpu_companion_matrix.py"
CHUNK = 65536


@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


@pytest.fixture(scope="module")
def cpu():
    from piquant import cpu as pc

    return pc


def run_matrix(kind, form, threads, nt_stores):
    env = {k: v for k, v in os.environ.items() if k not in ("PIQUANT_CPU_NT_STORES", "PIQUANT_CPU_SCALAR")}
    if nt_stores is not None:
        env["PIQUANT_CPU_NT_STORES"] = nt_stores
    r = subprocess.run([sys.executable, str(MATRIX), kind, form, str(threads)], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=300)
    if r.returncode == 77:
        pytest.skip("host without AVX-512")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    checked = int(r.stdout.split()[-1])
    assert r.stdout.split()[-2] == "checked" and checked > 0
    return checked


@pytest.mark.parametrize("threads", [1, 3, 7, 16])
@pytest.mark.parametrize("form", ["avx512", "scalar"])
@pytest.mark.parametrize("nt_stores", ["1", "0"], ids=["streaming_on", "streaming_off"])
@pytest.mark.parametrize("kind", ["quantize", "dequantize"])
def test_streaming_stores_forced_on_and_off(O, kind, nt_stores, form, threads):
    """six pairs x nearest / stochastic x output 0, 1, 5, 15 bytes off a 64-byte boundary x input one element off (quantize: 60 calls per size); twelve
    forms x output 0, 1, 3, 8 elements off (dequantize: 48 calls per size)"""
    sizes = {1, 17, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, threads * CHUNK - 1, threads * CHUNK + 1, 14 * CHUNK + 33}   # one thread: 7 of them
    assert run_matrix(kind, form, threads, nt_stores) == len(sizes) * (60 if kind == "quantize" else 48)


@pytest.mark.parametrize("kind,form,threads", [("natural_quantize", "avx512", 7), ("natural_dequantize", "avx512", 7), ("natural_quantize", "scalar", 3), ("natural_dequantize", "scalar", 3)])
def test_around_the_librarys_own_streaming_threshold(O, kind, form, threads):
    """no override: one output just under 4 MiB and one of 4 MiB, uint8 and uint4 bytes, float32 and bfloat16 elements"""
    assert run_matrix(kind, form, threads, None) > 0


# ---- the work hand-out
def quantize_all_pairs(O, ctx, x, tau=0.37):
    """-> {(pair, rounding): bytes} through the companion, each compared with the oracle"""
    got = {}
    for dt_in, xin in ((O.F32, x), (O.BF16, O.f32_to_bf16(x))):
        for dt_out, qmax in ((O.UINT8, 255), (O.UINT4, 15), (O.UINT2, 3)):
            scale = float(np.float32(2.0 / qmax))
            for rm in (0, 1):
                nbytes = O.packed_numel(x.size, dt_out)
                buf = np.full(nbytes + 16, 0xAA, dtype=np.uint8)
                ctx.quantize_ptr(xin.ctypes.data, dt_in, buf[8:].ctypes.data, dt_out, x.size, scale, qmax // 2, rm, tau)
                assert np.array_equal(buf[8: 8 + nbytes], O.quantize(xin, dt_in, dt_out, scale, qmax // 2, rm, tau, form=O.FORM_UNIFORM)), (x.size, dt_in, dt_out, rm)
                assert (buf[:8] == 0xAA).all() and (buf[8 + nbytes:] == 0xAA).all()
                got[dt_in, dt_out, rm] = buf[8: 8 + nbytes].copy()
    return got


def dequantize_all_forms(O, ctx, codes, prev32):
    got = {}
    n = prev32.size
    for dt_q in (O.UINT8, O.UINT4, O.UINT2):
        q = codes[: O.packed_numel(n, dt_q)]
        for dt_f in (O.F32, O.BF16):
            prev = prev32 if dt_f == O.F32 else O.f32_to_bf16(prev32)
            for op in (0, 1):
                out = prev.copy()
                ctx.dequantize_ptr(q.ctypes.data, dt_q, out.ctypes.data, dt_f, n, 0.02, 9, op)
                assert same_floats(out, O.dequantize(q, dt_q, dt_f, n, 0.02, 9, op, out=prev.copy())), (n, dt_q, dt_f, op)
                got[dt_q, dt_f, op] = out
    return got


@pytest.mark.parametrize("vector", [True, False], ids=["avx512", "scalar"])
def test_more_workers_than_elements(O, cpu, vector):
    """16 workers and 1, 3 or 15 elements: most shares are empty, and the shares that are not end inside a packed byte"""
    if vector and not cpu.use_avx512(True):
        pytest.skip("host without AVX-512")
    cpu.use_avx512(vector)
    rng = np.random.default_rng(16)
    try:
        ctx = cpu.CpuContext(16)
        for n in (1, 3, 15):
            x = rng.uniform(-1, 1, n).astype(np.float32)
            quantize_all_pairs(O, ctx, x)
            dequantize_all_forms(O, ctx, rng.integers(0, 256, n, dtype=np.uint8), rng.uniform(-3, 3, n).astype(np.float32))
            for dt, xin in ((O.F32, x), (O.BF16, O.f32_to_bf16(x))):
                assert ctx.minmax_ptr(xin.ctypes.data, dt, n) == O.minmax(xin, dt)
        ctx.close()
    finally:
        cpu.use_avx512(True)


def test_active_threads_changed_between_calls(O, cpu):
    """16 -> 2 -> 5 -> 1 -> 16 active workers of one pool: the same bytes every time (and the oracle's), at a size of several chunks per share and at
    one smaller than the pool"""
    rng = np.random.default_rng(17)
    ctx = cpu.CpuContext(16)
    assert ctx.num_threads == 16
    for n in (15, 3 * CHUNK + 5, 14 * CHUNK + 33):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        x[rng.choice(n, 3, replace=False)] = [np.nan, np.inf, -0.0]
        codes, prev = rng.integers(0, 256, n, dtype=np.uint8), rng.uniform(-3, 3, n).astype(np.float32)
        first = None
        for active in (16, 2, 5, 1, 16):
            ctx.set_active_threads(active)
            assert ctx.num_threads == 16, "the pool keeps all of its workers"
            got = (quantize_all_pairs(O, ctx, x), dequantize_all_forms(O, ctx, codes, prev), ctx.minmax_ptr(x.ctypes.data, O.F32, n))
            if first is None:
                first = got
            assert all(np.array_equal(got[0][k], first[0][k]) for k in first[0]) and all(same_floats(got[1][k], first[1][k]) for k in first[1]) and got[2] == first[2], (n, active)
    ctx.close()


# ---- affinity
def test_a_pinned_call_gives_the_caller_its_own_affinity_mask_back(O, cpu):
    """worker 0 is the caller, pinned to cpus[0] only while a call runs"""
    before = os.sched_getaffinity(0)
    cpus = sorted(before)[:4]
    rng = np.random.default_rng(18)
    ctx = cpu.CpuContext(max(len(cpus), 2))
    try:
        ctx.set_affinity(cpus)
        for n in (15, 5 * CHUNK + 7):
            x = rng.uniform(-1, 1, n).astype(np.float32)
            quantize_all_pairs(O, ctx, x)
            assert os.sched_getaffinity(0) == before, "a call left the caller pinned"
            dequantize_all_forms(O, ctx, rng.integers(0, 256, n, dtype=np.uint8), rng.uniform(-3, 3, n).astype(np.float32))
            assert ctx.minmax_ptr(x.ctypes.data, O.F32, n) == O.minmax(x, O.F32)
            assert os.sched_getaffinity(0) == before
        ctx.set_active_threads(1)          # one worker: the caller alone
        quantize_all_pairs(O, ctx, x)
        assert os.sched_getaffinity(0) == before
        ctx.set_active_threads(len(cpus))
        ctx.set_affinity([])               # removes the pinning
        quantize_all_pairs(O, ctx, x)
        assert os.sched_getaffinity(0) == before
    finally:
        os.sched_setaffinity(0, before)
        ctx.close()


# ---- concurrent callers (ctypes releases the GIL during a call: the Python threads below are inside the library at the same time)
def _caller(O, ctx, jobs, rounds, errors, barrier):
    try:
        barrier.wait()
        for _ in range(rounds):
            for kind, args, want in jobs:
                if kind == "quantize":
                    xin, dt_in, dt_out, scale, zp, rm = args
                    out = np.full(want.size, 0xAA, dtype=np.uint8)
                    ctx.quantize_ptr(xin.ctypes.data, dt_in, out.ctypes.data, dt_out, xin.size, scale, zp, rm, 0.37)
                    if not np.array_equal(out, want):
                        errors.append(("quantize", xin.size, dt_in, dt_out, rm))
                elif kind == "dequantize":
                    q, dt_q, dt_f, prev, op = args
                    out = prev.copy()
                    ctx.dequantize_ptr(q.ctypes.data, dt_q, out.ctypes.data, dt_f, prev.size, 0.02, 9, op)
                    if not same_floats(out, want):
                        errors.append(("dequantize", prev.size, dt_q, dt_f, op))
                else:
                    xin, dt = args
                    if ctx.minmax_ptr(xin.ctypes.data, dt, xin.size) != want:
                        errors.append(("minmax", xin.size, dt))
    except BaseException as e:   # noqa: BLE001  (reported by the parent thread)
        errors.append(repr(e))


def _jobs(O, seed):
    """a caller's calls with the oracle's answers, made before the threads start"""
    rng = np.random.default_rng(seed)
    jobs = []
    for n in (17, CHUNK + 1, 5 * CHUNK + 3):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        xb = O.f32_to_bf16(x)
        for xin, dt_in, dt_out, qmax, rm in ((x, O.F32, O.UINT8, 255, 0), (xb, O.BF16, O.UINT4, 15, 1), (x, O.F32, O.UINT2, 3, 0)):
            scale = float(np.float32(2.0 / qmax))
            jobs.append(("quantize", (xin, dt_in, dt_out, scale, qmax // 2, rm), O.quantize(xin, dt_in, dt_out, scale, qmax // 2, rm, 0.37, form=O.FORM_UNIFORM)))
        prev = rng.uniform(-3, 3, n).astype(np.float32)
        for dt_q, dt_f, op in ((O.UINT8, O.F32, 1), (O.UINT4, O.BF16, 0), (O.UINT2, O.BF16, 1)):
            q = rng.integers(0, 256, O.packed_numel(n, dt_q), dtype=np.uint8)
            pv = prev if dt_f == O.F32 else O.f32_to_bf16(prev)
            jobs.append(("dequantize", (q, dt_q, dt_f, pv, op), O.dequantize(q, dt_q, dt_f, n, 0.02, 9, op, out=pv.copy())))
        jobs.append(("minmax", (x, O.F32), O.minmax(x, O.F32)))
    return jobs


@pytest.mark.parametrize("shared", [True, False], ids=["one_context", "a_context_each"])
def test_two_caller_threads(O, cpu, shared):
    contexts = [cpu.CpuContext(4)] if shared else [cpu.CpuContext(3), cpu.CpuContext(4)]
    errors, barrier = [], threading.Barrier(2)
    threads = [threading.Thread(target=_caller, args=(O, contexts[k % len(contexts)], _jobs(O, 20 + k), 6, errors, barrier)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
        assert not t.is_alive(), "a caller never came back"
    assert not errors, errors[:5]
    for c in contexts:
        c.close()
