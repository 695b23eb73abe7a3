"""The scripted circuit run (sgfhe_debug_circuit_script) without a device: the layout of a script -- csrc/circuit.h's
circuit_script_calls, reached through a stand-alone program under ASan / UBSan (tests/native/circuit_script_sanitized.cpp)
-- against its restatement from Circuit.schedule() and CALL_ROWS (tests/circuit_script_cases.py), and the case tables of
tests/test_gpu_circuit_script.py against Python integers, so that a wrong table cannot make a GPU case vacuous."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import circuit_script_cases as SC
import ring_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT = 0x80000000


def _circuit(S, n_inputs, n_regs, gates, outputs, nexts):
    c = S.Circuit(n_inputs, registers=n_regs)
    for x, y in gates:
        c.gate(S.Wire(x), S.Wire(y))
    c.output(*[S.Wire(o) for o in outputs])
    if n_regs:
        c.next_state(*[S.Wire(x) for x in nexts])
    return c


# name, n_inputs, n_regs, gates, outputs, next states: wires 0 .. n_inputs the inputs, node g's wires n_inputs + 3 g ..
PLANS = {
    "empty": (2, 0, [], [0, 1 | NOT], []),
    "one": (2, 0, [(0, 1)], [2], []),
    "mixed": (2, 0, [(0, 1), (2, 1 | NOT), (0, 4)], [5, 0, 5 | NOT, 10, 8], []),     # levels 1, 2, 2; outputs: gate, input, ...
    "three": (2, 0, [(0, 1), (0, 1 | NOT), (0 | NOT, 1)], [2, 5, 8], []),            # one level of three nodes
    "regs": (2, 1, [(0, 1)], [2], [4]),
    "regs2": (3, 2, [(0, 2), (1, 3)], [6 | NOT, 0], [1, 8]),
}


def _runs():
    """(name, plan, n, count, ct, steps or None, emit or None, pack, flags)"""
    out = []
    for plan in ("empty", "one", "mixed"):
        out.append((plan + "_lwe", plan, 64, 8, 0, None, None, 0, 0))
        for flags in (0, 1, 3):
            out.append(("%s_ct_%d" % (plan, flags), plan, 8, 2, 1, None, None, 1, flags))
        out.append((plan + "_ct_nopack", plan, 8, 2, 1, None, None, 0, 0))
    for inst in (8192, 8193, 2736):                       # a level of exactly one call, of one row more, of 8208 rows in three nodes
        out.append(("one_%d" % inst, "one", 64, inst, 0, None, None, 0, 0))
        out.append(("three_%d" % inst, "three", 64, inst, 0, None, None, 0, 0))
    out.append(("three_direct_split", "three", 8, 342, 1, None, None, 1, 1))      # 3 x 2736 rows: the boundary inside a producing node
    for blocks in (128, 129):                             # n = 64: 128 ciphertexts a pack group
        for flags in (0, 1, 3):
            out.append(("pack_%d_%d" % (blocks, flags), "one", 64, blocks, 1, None, None, 1, flags))
    out.append(("pack_alternating", "mixed", 64, 66, 1, None, None, 1, 1))        # 5 outputs x 66: three groups, direct and fresh
    for emit in (None, "1010", "0000", "0001"):
        tag = emit or "all"
        out.append(("regs_lwe_" + tag, "regs", 64, 8, 0, 4, emit, 0, 0))
        for flags in (0, 1, 3):
            out.append(("regs2_ct_%s_%d" % (tag, flags), "regs2", 8, 3, 1, 4, emit, 1, flags))
    return out


def _build(tmp_path, gxx, name, flags):
    src = os.path.join(ROOT, "tests", "native", "circuit_script_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / name)
    b = subprocess.run([gxx, "-std=c++17"] + flags + ["-Wall", "-Wextra", "-Werror", "-I", inc, "-I", os.path.dirname(src), src,
                                                       "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def test_script_layout_under_asan_and_ubsan_equals_the_python_restatement(S, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    runs = _runs()
    text = ""
    for name, plan, n, count, ct, steps, emit, pack, flags in runs:
        n_inputs, n_regs, gates, outputs, nexts = PLANS[plan]
        text += "%s %d %d %d %d %d %s %d %d %d %d %d %d\n" % (name, n, count, ct, steps is not None, steps or 0, emit or "-", pack,
                                                           flags, n_inputs, n_regs, len(gates), len(outputs))
        text += " ".join(str(x) for g in gates for x in g) + "\n" + " ".join(str(x) for x in outputs) + "\n"
        text += " ".join(str(x) for x in nexts) + "\n"
    exe = _build(tmp_path, gxx, "circuit_script_sanitized",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.rstrip("\n").split("\n")
    assert lines[-1] == "ok %d" % len(runs)
    seen_raw = seen_two = seen_pack = 0
    for (name, plan, n, count, ct, steps, emit, pack, flags), line in zip(runs, lines):
        f = line.split()
        got = [(int(x.split(":")[0]), x.split(":")[1] == "1") for x in f[2:]]
        assert f[0] == name and int(f[1]) == len(got)
        c = _circuit(S, *PLANS[plan])
        want = SC.script_calls(c, n, count, ct=bool(ct), steps=steps, emit=None if emit is None else [int(x) for x in emit],
                               pack=bool(pack), direct=bool(flags & 1), lift=bool(flags & 2))
        assert got == want, (name, got, want)
        seen_raw += any(raw for _, raw in got)
        seen_two += any(rows == 8192 for rows, _ in got) and len(got) > 1
        seen_pack += ct and pack and not flags & 2
    assert seen_raw >= 10 and seen_two >= 3 and seen_pack >= 10
    by = dict(zip([x[0] for x in runs], lines))
    assert by["one_8192"].split()[1:] == ["1", "8192:0"] and by["one_8193"].split()[1:] == ["2", "8192:0", "1:0"]
    assert by["three_2736"].split()[1:] == ["2", "8192:0", "16:0"]
    assert by["three_direct_split"].split()[1:] == ["2", "8192:1", "16:1"]          # no refresh call: every output direct
    assert by["pack_128_0"].split()[1:] == ["2", "8192:0", "8192:1"]
    assert by["pack_129_0"].split()[1:] == ["4", "8192:0", "64:0", "8192:1", "64:1"]
    assert by["pack_129_1"].split()[1:] == ["2", "8192:1", "64:1"]                  # direct: the gate's rows, nothing refreshed
    assert by["regs2_ct_0000_0"].split()[1] == "8" and by["regs2_ct_1010_0"].split()[1] == "10"   # 4 steps x 2 levels, + 2 groups
    exe2 = _build(tmp_path, gxx, "circuit_script_plain", ["-O2"])
    r2 = subprocess.run([exe2], input=text, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout


def _rings(S):
    out = {name: RC.ring(S, name).params for name in ("tiny", "wide", "composite", "m128")}
    out["params64"] = S.Params(64)
    return out


def test_modred_boundaries_round_as_labelled_on_every_ring(S):
    """Every listed residue is in [0, Q), the two of a pair are neighbours that round to k + 1 and to k in exact
    rational arithmetic, and modred_words, lift_words and lwe_not_modq of circuit.py agree with Python integers there."""
    from fractions import Fraction
    cm = S.circuit
    for name, p in _rings(S).items():
        Q, r, DQ = p.Q, p.r, p.DQ_tilde
        table = SC.modred_boundaries(Q, r)
        assert len(table) == 16
        for (la, x, ka), (lb, y, kb) in zip(table[0::2], table[1::2]):
            assert 0 <= y < x < Q and y == x - 1, (name, la)
            assert ka == (kb + 1) % r
            # round-half-up of the exact quotient
            for v, k in ((x, ka), (y, kb)):
                exact = Fraction(v * r, Q)
                assert (exact + Fraction(1, 2)).__floor__() % r == k == SC.modred_int(v, Q, r), (name, la, lb)
        assert {k for _, _, k in table} >= {0, 1, r // 4, r // 2, r - 1}
        every = SC.residue_table(Q, r, DQ)
        assert all(0 <= v < Q for v in every) and {0, 1, Q - 1, (2 * DQ) % Q, (2 * DQ + 1) % Q} <= set(every)
        if Q > 1 << 64:
            assert {(1 << 64) - 1, 1 << 64} <= set(every)
        res = SC.from_int(every)
        assert [int(v) for v in SC.to_int(res)] == every
        assert [int(v) for v in cm.modred_words(res, Q, r)] == [SC.modred_int(v, Q, r) for v in every], name
        rows = SC.from_int([[v, w] for v in every for w in every])
        got = SC.to_int(cm.lwe_not_modq(rows, Q, DQ))
        assert [[int(a), int(b)] for a, b in got] == [SC.not_q_int([v, w], Q, DQ) for v in every for w in every], name
        assert SC.not_q_int([0, (2 * DQ) % Q], Q, DQ) == [0, 0] and SC.not_q_int([0, (2 * DQ + 1) % Q], Q, DQ) == [0, Q - 1]
        words = list(SC.EDGE_WORDS(r)) + [r // 2 - 1, r // 2 + 1, r - 2]
        lifted = SC.to_int(cm.lift_words(np.array(words, dtype=np.uint64), Q, r))
        assert [int(v) for v in lifted] == [SC.lift_int(v, Q, r) for v in words], name
        assert all(SC.modred_int(SC.lift_int(v, Q, r), Q, r) == v for v in range(r)), name


def test_sum_tables_hit_their_values_and_not_its_codewords(S):
    cm = S.circuit
    for r in (1024, _rings(S)["tiny"].r, _rings(S)["m128"].r):
        cases = SC.sum_cases(r)
        assert {u for _, _, u in cases} >= {0, r - 1, (-128) % r, 128 % r}
        for label, terms, u in cases:
            assert 1 <= len(terms) <= 64 and all(w in (-2, -1, 1, 2) and 0 <= x < r for w, x in terms)
            assert sum(w * x for w, x in terms) % r == u, (r, label)
        assert len(cases[0][1]) == len(cases[1][1]) == 64
        # NOT over Z_r at the three codewords a reference can be read at
        for one in (r // 4, r // 8, r // 16):
            for b in (0, one, one + 1):
                row = np.array([0, 1, r - 1, b], dtype=np.uint64)
                assert [int(x) for x in cm.lwe_not(row, r, one)] == SC.not_r_int([0, 1, r - 1, b], r, one)
        assert SC.EDGE_WORDS(r) == (0, 1, r // 4 - 1, r // 4, r // 2, r - 1)


def test_fill_separates_wires_instances_and_words():
    f = SC.fill(3, 40, 64, 1024)
    assert f.shape == (3, 40, 65) and f.max() < 1024
    assert f[1, 2, 3] == (37 + 22 + 15) % 1024 and f[2, 39, 64] == (74 + 11 * 39 + 5 * 64) % 1024
    assert len({tuple(row) for w in f for row in w}) == 120


def test_hook_is_declared_bound_and_documented(S):
    hdr = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    for name in ("sgfhe_debug_circuit_script", "sgfhe_debug_circuit_script_calls"):
        assert name in S.EXPORTED_SYMBOLS and re.search(r"int32_t %s\(" % name, hdr)
    assert len(S.lib().sgfhe_debug_circuit_script.argtypes) == 19
    assert "#define SGFHE_ABI_VERSION 7u" in hdr
    assert "sgfhe_debug_circuit_script" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert (S.engine.SCRIPT_CT, S.engine.SCRIPT_STEPPED, S.engine.SCRIPT_PROBE, S.engine.SCRIPT_DEVICE) == tuple(
        int(re.search(r"#define SGFHE_SCRIPT_%s (\d+)u" % k, hdr).group(1)) for k in ("CT", "STEPPED", "PROBE", "DEVICE"))
