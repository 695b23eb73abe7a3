"""The chunk policy of a bootstrap call (csrc/chunking.h: default_chunk, call_chunks, chunk_rows, max_chunk_rows;
DESIGN.md section 4) without a device: a stand-alone program holds it to the worked cases of its comments and to its
properties over a sweep, under ASan / UBSan (tests/native/chunking_sanitized.cpp)."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_policy_under_asan_and_ubsan(tmp_path):
    """How a batch is cut across the lanes: the worked cases (256 = 128 + 128, 49 = 32 + 17, 8 = 4 + 4, 13 = 7 + 6 with
    the fused kernel, ...), the chunks cover every batch up to 10000 exactly once under every setting of the sweep, and
    the rows a circuit run sizes its work buffers with suffice for every call of the run; the plain build prints the
    same line."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "chunking_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "chunking_sanitized")
    # (the sanitizer runtimes are linked into the program, so that it starts in any environment: a dynamic ASan runtime
    #  refuses to start behind a library the environment preloads)
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                        "-I", inc, src, "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)   # (the environment as it is)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = r.stdout.strip()
    assert re.fullmatch(r"ok [1-9][0-9]*", line), line
    exe2 = str(tmp_path / "chunking_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe2], check=True,
                   timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout.strip() == line
