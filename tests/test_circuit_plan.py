"""The gate-circuit planner (csrc/circuit.h, sgfhe_circuit_create / _info of include/sgfhe_hip.h) and the host
statements of the model in sgfhe.jl_amd/circuit.py.  No GPU: the plan is host data."""

import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT = 0x7FFFFFFF, 0x80000000
ERR_INVALID_ARG = -1


def _create(S, n_inputs, gates, outputs, null_gates=False, null_outputs=False, null_out=False):
    L = S.lib()
    g = np.ascontiguousarray(np.array(gates, dtype=np.uint32).reshape(-1, 2))
    o = np.ascontiguousarray(np.array(outputs, dtype=np.uint32))
    h = ctypes.c_void_p()
    rc = L.sgfhe_circuit_create(n_inputs, None if null_gates else g.ctypes.data_as(ctypes.c_void_p), len(g),
                                None if null_outputs else o.ctypes.data_as(ctypes.c_void_p), len(o),
                                None if null_out else ctypes.byref(h))
    return rc, h


def _info(S, n_inputs, gates, outputs):
    rc, h = _create(S, n_inputs, gates, outputs)
    assert rc == 0
    info = (ctypes.c_uint64 * 4)()
    assert S.lib().sgfhe_circuit_info(h, info) == 0
    assert S.lib().sgfhe_circuit_destroy(h) == 0
    return tuple(int(v) for v in info)


def test_malformed_circuits_are_refused(S):
    # node 0's inputs: its own wire (2), a later node's wire, an id past the end, NOT on an id past the end
    assert _create(S, 2, [[2, 0]], [2])[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 1], [0, 6]], [2])[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 5]], [2])[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 5 | NOT]], [2])[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 1]], [5])[0] == ERR_INVALID_ARG                 # output past the end
    assert _create(S, 2, [[0, 1]], [0x7FFFFFFE | NOT])[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 1]], [])[0] == ERR_INVALID_ARG                  # zero outputs
    assert _create(S, 2, [[0, 1]], [2], null_gates=True)[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 1]], [2], null_outputs=True)[0] == ERR_INVALID_ARG
    assert _create(S, 2, [[0, 1]], [2], null_out=True)[0] == ERR_INVALID_ARG
    assert S.lib().sgfhe_circuit_info(None, (ctypes.c_uint64 * 4)()) == ERR_INVALID_ARG
    # and the well-formed neighbours of those are accepted
    assert _create(S, 2, [[0, 1], [2 | NOT, 4]], [5, FALSE | NOT, 1])[0] == 0
    assert _create(S, 0, [[FALSE, FALSE | NOT]], [0])[0] == 0


def test_info_of_small_circuits(S):
    # one node: 1 level, 1 node, width 1; slots: both inputs + the one output wire read
    assert _info(S, 2, [[0, 1]], [2]) == (1, 1, 1, 3)
    # only inputs and constants as outputs: nothing to evaluate, the two inputs read keep a slot each
    assert _info(S, 3, [[0, 1]], [1, FALSE, 2 | NOT]) == (0, 0, 0, 2)
    # a chain of 3 with a dead node beside it: levels 3, nodes 3; x and y die after level 1 and their slots
    # take the level-2 / level-3 wires: 2 inputs + AND of node 0 = 3 slots
    gates = [[0, 1], [2, 1 | NOT], [0, 0], [5 | NOT, FALSE]]
    #  node 0 (x, y) -> 2, 3, 4; node 1 (AND0, ~y) -> 5, 6, 7; node 2 dead; node 3 (~AND1, FALSE) -> 11, 12, 13
    assert _info(S, 2, gates, [13]) == (3, 3, 1, 3)
    # two independent nodes on level 1, one joining them on level 2; an output on an input keeps it alive.
    # Slots: the 4 inputs, then AND0, OR0 (an output) and XOR1 on level 1 -- the inputs level 1 reads are
    # free only after it -- and node 2's XOR takes a freed one: 7
    gates = [[0, 1], [2, 3], [4 | NOT, 9]]
    assert _info(S, 4, gates, [12, 0, 5 | NOT]) == (2, 3, 2, 7)


def test_python_schedule_matches_the_planner(S):
    rng = np.random.default_rng(5)
    for _ in range(40):
        c = _random_circuit(S, rng, int(rng.integers(1, 8)), int(rng.integers(0, 60)))
        sched = c.schedule()
        info = c.info()
        assert info["levels"] == len(sched)
        assert info["nodes"] == sum(len(l) for l in sched)
        assert info["widest"] == max((len(l) for l in sched), default=0)


def _random_circuit(S, rng, n_inputs, n_gates):
    c = S.Circuit(n_inputs)
    wires = list(c.inputs) + [S.Circuit.FALSE]
    for _ in range(n_gates):
        x, y = (wires[int(rng.integers(len(wires)))] for _ in range(2))
        x = ~x if rng.integers(2) else x
        y = ~y if rng.integers(2) else y
        wires.extend(c.gate(x, y))
    outs = [wires[int(rng.integers(len(wires)))] for _ in range(int(rng.integers(1, 6)))]
    c.output(*[~w if rng.integers(2) else w for w in outs])
    return c


def test_evaluate_plain_truth_tables(S):
    """Every gate of a node with every NOT pattern on its inputs and its output, and the constants."""
    x = np.array([0, 0, 1, 1], dtype=bool)
    y = np.array([0, 1, 0, 1], dtype=bool)
    for nx, ny, nout in itertools.product((False, True), repeat=3):
        c = S.Circuit(2)
        a, b = c.inputs
        outs = c.gate(~a if nx else a, ~b if ny else b)
        c.output(*[~w if nout else w for w in outs], S.Circuit.FALSE, S.Circuit.TRUE, ~a)
        got = c.evaluate_plain(np.stack([x, y]))
        xi, yi = (~x if nx else x), (~y if ny else y)
        want = [xi & yi, xi | yi, xi ^ yi]
        for g in range(3):
            assert np.array_equal(got[g], ~want[g] if nout else want[g]), (nx, ny, nout, g)
        assert not got[3].any() and got[4].all() and np.array_equal(got[5], ~x)


def test_evaluate_plain_adder(S):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import encrypted_adder
    bits = 8
    c = encrypted_adder.adder_circuit(S, bits)
    rng = np.random.default_rng(11)
    xs = rng.integers(0, 1 << bits, size=200)
    ys = rng.integers(0, 1 << bits, size=200)
    inp = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=bool)
    out = c.evaluate_plain(inp)
    sums = sum(out[i].astype(np.int64) << i for i in range(bits + 1))
    assert np.array_equal(sums, xs + ys)
    info = c.info()
    assert info["nodes"] == 3 * bits and info["levels"] == 2 * bits + 1


def test_replay_levels_composes_like_evaluate_plain(S):
    """replay_levels (the host composition the GPU tests compare with) on a stand-in bootstrap that works on
    clear bits encoded as b = bit * Dr: its call order and NOT arithmetic agree with evaluate_plain."""
    from sgfhe_jl_amd import circuit as C
    r, n = 64, 3
    rng = np.random.default_rng(3)
    c = _random_circuit(S, rng, 4, 40)
    inst = 5
    bits = rng.integers(0, 2, size=(4, inst)).astype(bool)
    inputs = np.zeros((4, inst, n + 1), dtype=np.uint64)
    inputs[:, :, n] = bits * (r // 4)
    calls = []

    def boot(call, a1, b1, a2, b2):
        calls.append(call)
        x, y = (b1 == r // 4), (b2 == r // 4)
        assert np.all((b1 == 0) | (b1 == r // 4)) and not a1.any()
        out = np.zeros((len(b1), 3, n + 1), dtype=np.uint64)
        for g, v in enumerate((x & y, x | y, x ^ y)):
            out[:, g, n] = v * (r // 4)
        return out

    out = C.replay_levels(c, inputs, r, boot)
    assert calls == list(range(len(c.schedule())))
    assert np.array_equal(out[:, :, n] == r // 4, c.evaluate_plain(bits))


def test_planner_under_asan_and_ubsan(tmp_path):
    """csrc/circuit.h under the sanitizers over a few thousand seeded random DAGs
    (tests/native/circuit_plan_sanitized.cpp): levels, pruning, slot liveness, outputs kept, rows and calls."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_plan_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_plan_sanitized")
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
    exe2 = str(tmp_path / "circuit_plan_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout.strip() == digest
