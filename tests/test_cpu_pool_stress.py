"""CPU: the worker pool of libpiquant_cpu.so under the thread sanitizer and under the address + undefined-behaviour sanitizers, as a stand-alone
program (tests/cpu_pool_stress.cpp, with its own main) built from the library's two sources with the flags of csrc/cpu/Makefile at -O1 -g.
Nothing is loaded into Python and nothing is preloaded: the sanitizer's runtime is linked into the program.  The program must end with status 0
and without a sanitizer report."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CPU_DIR = ROOT / "pi-quant_amd" / "csrc" / "cpu"
PROGRAM = Path(__file__).resolve().parent / "cpu_pool_stress.cpp"
SANITIZERS = {"thread": ["-fsanitize=thread"], "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def makefile_flags():
    """FLAGS and AVX512 of csrc/cpu/Makefile, the optimisation level replaced by -O1 -g"""
    text = (CPU_DIR / "Makefile").read_text()
    flags = re.search(r"^FLAGS\s*:=\s*(.+)$", text, re.M).group(1).split()
    avx512 = re.search(r"^AVX512\s*:=\s*(.+)$", text, re.M).group(1).split()
    tu = re.search(r"\$\(AVX512\)\s+(-D\S+)", text).group(1)
    assert "-O3" in flags and "-ffp-contract=off" in flags and all(f.startswith("-mavx512") for f in avx512)
    flags = [f for f in flags if f != "-O3" and not f.startswith("-I")] + ["-O1", "-g", f"-I{ROOT / 'include'}", f"-I{CPU_DIR}"]
    return flags, avx512 + [tu]


def compiler():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this host")
    return cxx


def build(tmp_path, sanitize):
    cxx = compiler()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *sanitize, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"{cxx} cannot link the runtime of {sanitize[0]}: {r.stderr.strip()[-300:]}")
    flags, avx512 = makefile_flags()
    units = [(CPU_DIR / "piquant_cpu.cpp", []), (CPU_DIR / "cpu_avx512.cpp", avx512), (PROGRAM, [])]
    jobs = [(tmp_path / (src.stem + ".o"), subprocess.Popen([cxx, *flags, *extra, *sanitize, "-c", str(src), "-o", str(tmp_path / (src.stem + ".o"))],
                                                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for src, extra in units]
    for obj, job in jobs:
        out, _ = job.communicate(timeout=600)
        assert job.returncode == 0, out[-3000:]
    exe = tmp_path / "cpu_pool_stress"
    r = subprocess.run([cxx, "-pthread", *sanitize, *[str(obj) for obj, _ in jobs], "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name", list(SANITIZERS))
def test_pool_stress_program_is_clean_under_the_sanitizer(tmp_path, name):
    exe = build(tmp_path, SANITIZERS[name])
    env = {"PATH": "/usr/bin:/bin", "TSAN_OPTIONS": "halt_on_error=1 exitcode=66 second_deadlock_stack=1", "ASAN_OPTIONS": "detect_leaks=1 exitcode=67",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    if name == "thread" and r.returncode != 0 and "unexpected memory mapping" in r.stderr:
        # this runtime does not know the kernel's address-space layout; the same program with the layout randomisation off, where that is to be had
        setarch = shutil.which("setarch")
        if setarch is None:
            pytest.skip("the thread sanitizer's runtime cannot map its shadow memory on this kernel, and there is no setarch to switch randomisation off")
        r = subprocess.run([setarch, "-R", str(exe)], capture_output=True, text=True, env=env, timeout=600)
        if "unexpected memory mapping" in r.stderr or "Operation not permitted" in r.stderr:
            pytest.skip("the thread sanitizer's runtime cannot map its shadow memory on this kernel, with or without address-space randomisation")
    report = [line for line in r.stderr.splitlines() if "Sanitizer" in line or "runtime error" in line or "MISMATCH" in line]
    assert r.returncode == 0 and not report, (r.returncode, report[:10], r.stderr[-3000:])
    assert r.stdout.startswith("ok")
