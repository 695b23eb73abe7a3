"""The one judge of a run's arguments (csrc/circuit.h: CircuitRequest, circuit_request_check) without
a device: a stand-alone program makes every case of tests/run_error_cases.py into a request against a small plan, every
pointer a dummy address, under ASan / UBSan (tests/native/circuit_request_sanitized.cpp), and its answers are those the
library gave on the GPU at the commit tests/golden/circuit_run_errors.json was recorded at."""

import json
import os
import re
import shutil
import subprocess

import pytest

import run_error_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRS = ("in", "in_a", "in_b", "state_in", "state_a", "state_b", "data", "emit", "out", "out_w", "out_v", "state_out", "sk",
        "in_bits", "stats")
M = 512   # Params(64).m
# a ctx whose primes miss the exactness bound of pack_encrypted_bits (no valid parameter set has one): refused behind
# the key check and before an empty run returns OK; the text as sgfhe_circuit_run_ct_ex gives it
PACK_BOUND = (-2, "pack_encrypted_bits: exactness bound of the RNS primes")   # SGFHE_ERR_UNSUPPORTED


def _line(entry, case, pack_exact=True):
    E = RC.ENTRIES[entry]
    given = [a for a in RC.shapes(entry, case) if a not in case.null and (a not in RC.OPTIONAL or a in case.given)
             and (a != "data" or RC.PLAN_FACTS[case.plan][2])]
    mask = sum(1 << PTRS.index(a) for a in given)
    fields = [entry, case.name, case.plan, int("circ" not in case.null), int(case.key), int(pack_exact), int(E.ct),
              int(E.stepped), int(E.probe), int(E.device), int(E.data), case.count, case.steps,
              RC.N + (case.N == "n+1"), case.flags, mask]
    return " ".join(str(f) for f in fields)


def _build(tmp_path, gxx, name, flags):
    src = os.path.join(ROOT, "tests", "native", "circuit_request_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / name)
    b = subprocess.run([gxx, "-std=c++17"] + flags + ["-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def test_request_check_under_asan_and_ubsan(tmp_path):
    """Every case's code and message equal the fixture's; the pack bound; `device` and the stream change no verdict; a
    seeded sweep of accepted requests returns count or count * n instances; a request with a script is judged as on a ctx
    with a key, but for the refusals of its own; the plain build prints the same."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    with open(os.path.join(ROOT, "sgfhe.jl_amd", "csrc", "kernels.h")) as fh:
        split_rows = int(re.search(r"constexpr uint32_t CIRC_SPLIT_ROWS = (\d+);", fh.read()).group(1))
    with open(os.path.join(ROOT, "tests", "golden", "circuit_run_errors.json")) as fh:
        golden = json.load(fh)["cases"]
    assert set(golden) == {RC.case_id(e, c) for e, c in RC.CASES}
    bound = [(e, RC.Case(name, "plain", True, count, 1, "n", 0, (), (), "refused"))
             for e in RC.ENTRIES if RC.ENTRIES[e].ct for name, count in (("pack_bound", 1), ("pack_bound_and_count_0", 0))]
    text = "env %d %d %d\n" % (RC.N, M, -(-RC.N // split_rows))
    text += "\n".join([_line(e, c) for e, c in RC.CASES] + [_line(e, c, pack_exact=False) for e, c in bound]) + "\n"
    exe = _build(tmp_path, gxx, "circuit_request_sanitized",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.rstrip("\n").split("\n")
    assert lines[-1].split()[:2] == ["ok", str(len(RC.CASES) + len(bound))] and int(lines[-1].split()[2]) >= 500
    got = {}
    for ln in lines[:-1]:
        entry, name, code, msg = (ln.split(" ", 3) + [""])[:4]
        got[(entry, name)] = [int(code), msg]
    for e, c in RC.CASES:
        assert got[(e, c.name)] == golden[RC.case_id(e, c)], (e, c.name)
        assert (got[(e, c.name)][0] == 0) == (c.expect == "empty"), (e, c.name)
    for e, c in bound:
        assert got[(e, c.name)] == list(PACK_BOUND), e
    # the scripted form (sgfhe_debug_circuit_script): the refusals of its own, in the hook's name and saying why
    assert got[("script", "null_script")] == [-1, "sgfhe_debug_circuit_script: NULL script: the calls' results, the staged log "
                                              "and the descriptor log are needed"]
    assert got[("script", "probe_form")] == [-1, "sgfhe_debug_circuit_script: the host forms only: no probe, no device form"]
    code, why = got[("script", "live_sibling")]
    assert code == -1 and why.startswith("sgfhe_debug_circuit_script: a plan with a live LUT sibling") and "inside the bootstrap call" in why
    exe2 = _build(tmp_path, gxx, "circuit_request_plain", ["-O2"])
    r2 = subprocess.run([exe2], input=text, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
