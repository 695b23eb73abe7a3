"""The call arithmetic of a circuit run (csrc/circuit.h: circuit_level_call, circuit_job_chunk, circuit_pack_runs,
circuit_run_sizes) without a device: a stand-alone program compares each function with a
row-by-row restatement under ASan / UBSan (tests/native/circuit_calls_sanitized.cpp)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_arithmetic_under_asan_and_ubsan(tmp_path):
    """Rows, nodes, jobs and sum flag of every level call, the grids of a job range, the runs of every pack group,
    the buffer sizes and the number of call numbers a run consumes, over fixed and seeded random plans of every node
    and output kind; the plain build prints the same digest."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_calls_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_calls_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    digest = r.stdout.strip()
    assert len(digest) == 16
    exe2 = str(tmp_path / "circuit_calls_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout.strip() == digest
