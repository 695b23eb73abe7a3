"""Three-input nodes (sgfhe_circuit_create3, include/sgfhe_hip.h) without a device: the
planner's validation through ctypes, the all-NONE plan against sgfhe_circuit_create_lanes, Circuit.gate3 /
full_adder / ripple_adder against truth tables and integer addition, and the planner with circuit_plain_bits under
ASan / UBSan (tests/native/circuit_gate3_sanitized.cpp)."""

import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1
NONE = 0x7FFFFFFE
FALSE = 0x7FFFFFFF
NOT = 0x80000000


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _create3(L, n_inputs, gates, gshift, outs, oshift, group):
    g = np.ascontiguousarray(np.array(gates, dtype=np.uint32).reshape(-1, 3))
    o = np.ascontiguousarray(np.array(outs, dtype=np.uint32))
    gs = None if gshift is None else np.ascontiguousarray(np.array(gshift, dtype=np.int32).reshape(-1, 3))
    os_ = None if oshift is None else np.ascontiguousarray(np.array(oshift, dtype=np.int32))
    h = ctypes.c_void_p(0xDEAD)
    rc = L.sgfhe_circuit_create3(n_inputs, _p(g), _p(gs), len(g), _p(o), _p(os_), len(o), group, ctypes.byref(h))
    return rc, h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def test_create3_validation(S):
    L = S.lib()
    assert "sgfhe_circuit_create3" in S.EXPORTED_SYMBOLS
    assert L.sgfhe_abi_version() == 7          # functions are only added
    hdr = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    assert "#define SGFHE_CIRCUIT_NONE 0x7FFFFFFEu" in hdr
    # 2 inputs; node 0 = (0, 1, ~0), node 1 = (MAJ of 0, 0, XOR3 of 0): wires 2..4 and 5..7
    good = [(0, 1, NOT | 0), (2, 0, 4)]
    outs = [5, NOT | 7, 0]

    def refused(gates, gshift, outputs, oshift, group):
        rc, h = _create3(L, 2, gates, gshift, outputs, oshift, group)
        assert rc == ERR_INVALID_ARG and h.value is None, (gates, gshift, outputs, oshift, group)

    refused([(NONE, 1, 0), (2, 0, NONE)], None, outs, None, 8)           # NONE as the first input
    refused([(0, NONE, 0), (2, 0, NONE)], None, outs, None, 8)           # ... the second
    refused([(0, NONE, NONE), (2, 0, NONE)], None, outs, None, 8)
    refused([(0, 1, NOT | NONE), (2, 0, 4)], None, outs, None, 8)        # NONE with the NOT bit
    refused(good, None, [5, NONE, 0], None, 8)                           # NONE as an output
    refused(good, None, [5, NOT | NONE, 0], None, 8)
    refused([(0, 1, 2), (2, 0, 4)], None, outs, None, 8)                 # the third reference names the node's own wire
    refused([(0, 1, 5), (2, 0, 4)], None, outs, None, 8)                 # ... a later node's
    refused([(0, 1, 0), (2, 0, 8)], None, outs, None, 8)                 # ... no wire at all
    for d in (8, -8, 2 ** 31 - 1, -2 ** 31):                             # |d| >= group on the third input
        refused(good, [(0, 0, d), (0, 0, 0)], outs, None, 8)
        refused(good, [(0, 0, 0), (0, 0, d)], outs, None, 8)
    refused(good, [(0, 0, 1), (0, 0, 0)], outs, None, 1)                 # group = 1 admits no shift but 0
    refused(good, None, outs, None, 0)
    refused(good, None, [], None, 8)
    assert L.sgfhe_circuit_create3(2, None, None, 0, None, None, 0, 1, None) == ERR_INVALID_ARG
    # accepted: the largest shifts, any shift beside NONE, a constant third input with a shift, NULL arrays
    for gates, gshift, group in ((good, None, 1), (good, [(7, -7, -7), (0, 0, 7)], 8),
                                 ([(0, 1, NONE), (2, 0, 4)], [(0, 0, -2 ** 31), (0, 0, 0)], 8),
                                 ([(0, 1, NOT | FALSE), (2, 0, FALSE)], [(0, 0, 3), (0, 0, -3)], 4)):
        rc, h = _create3(L, 2, gates, gshift, outs, None, group)
        assert rc == 0 and h.value, (gates, gshift, group)
        assert _info(L, h)[:3] == [2, 2, 1]
        g = ctypes.c_uint32(0)
        assert L.sgfhe_circuit_group(h, ctypes.byref(g)) == 0 and g.value == group
        L.sgfhe_circuit_destroy(h)
    # a node that is reached through a third reference only stays alive, and sets the level
    rc, h = _create3(L, 2, [(0, 1, NONE), (0, 1, NONE), (0, 0, NOT | 5)], None, [10], None, 1)
    assert rc == 0 and _info(L, h)[:3] == [2, 2, 1]
    L.sgfhe_circuit_destroy(h)


def test_all_none_create3_is_the_create_lanes_plan(S):
    """The same arrays through sgfhe_circuit_create_lanes and, padded with SGFHE_CIRCUIT_NONE (and shifts that are
    ignored), through sgfhe_circuit_create3: the same sgfhe_circuit_info and group."""
    L = S.lib()
    rng = np.random.default_rng(7)
    for n_gates, group in ((1, 1), (7, 1), (40, 1), (25, 8)):
        def shift():
            return int(rng.integers(-(group - 1), group))
        gates = [(int(rng.integers(3 + 3 * g)) | (NOT if rng.integers(2) else 0),
                  FALSE if rng.integers(9) == 0 else int(rng.integers(3 + 3 * g))) for g in range(n_gates)]
        gsh = [(shift(), shift()) for _ in range(n_gates)]
        outs = [3 + 3 * n_gates - 1, NOT | 1, FALSE, 3 + int(rng.integers(3 * n_gates))]
        osh = [shift() for _ in outs]
        g = np.ascontiguousarray(np.array(gates, dtype=np.uint32))
        gs = np.ascontiguousarray(np.array(gsh, dtype=np.int32))
        o = np.ascontiguousarray(np.array(outs, dtype=np.uint32))
        os_ = np.ascontiguousarray(np.array(osh, dtype=np.int32))
        h0 = ctypes.c_void_p()
        assert L.sgfhe_circuit_create_lanes(3, _p(g), _p(gs), n_gates, _p(o), _p(os_), len(outs), group, ctypes.byref(h0)) == 0
        rc, h1 = _create3(L, 3, [p + (NONE,) for p in gates], [s + (int(rng.integers(-99, 99)),) for s in gsh], outs, osh, group)
        assert rc == 0 and _info(L, h1) == _info(L, h0)
        grp = ctypes.c_uint32()
        assert L.sgfhe_circuit_group(h1, ctypes.byref(grp)) == 0 and grp.value == group
        L.sgfhe_circuit_destroy(h1)
        L.sgfhe_circuit_destroy(h0)


def test_gate3_truth_table_every_not_pattern(S):
    """evaluate_plain of gate3 over all 8 input patterns x the 8 NOT patterns: MAJ, ONE_OR_TWO and XOR3 from the
    count of true inputs after NOT."""
    c = S.Circuit(3)
    x, y, z = c.inputs
    outs = []
    for pat in range(8):
        outs.extend(c.gate3(~x if pat & 1 else x, ~y if pat & 2 else y, ~z if pat & 4 else z))
    c.output(*outs)
    assert c.has_gate3 and c.n_gates == 8 and c.info() == dict(levels=1, nodes=8, widest=8, slots=27)
    bits = np.array(list(itertools.product([0, 1], repeat=3)), dtype=bool).T         # [3][8]
    got = c.evaluate_plain(bits)
    for pat in range(8):
        v = bits ^ np.array([[pat & 1], [pat & 2], [pat & 4]], dtype=bool)
        s = v.sum(axis=0)
        assert np.array_equal(got[3 * pat], s >= 2), pat
        assert np.array_equal(got[3 * pat + 1], (s == 1) | (s == 2)), pat
        assert np.array_equal(got[3 * pat + 2], s % 2 == 1), pat
    # constants as the third input: FALSE leaves AND, OR, XOR; TRUE gives OR, NAND, XNOR
    d = S.Circuit(2)
    p, q = d.inputs
    d.output(*(d.gate(p, q) + d.gate3(p, q, S.Circuit.FALSE) + d.gate3(p, q, S.Circuit.TRUE)))
    two = np.array(list(itertools.product([0, 1], repeat=2)), dtype=bool).T
    t = d.evaluate_plain(two)
    assert np.array_equal(t[3:6], t[0:3])
    assert np.array_equal(t[6], t[1]) and np.array_equal(t[7], ~t[0]) and np.array_equal(t[8], ~t[2])
    # a circuit without gate3 still takes the old entry points (handle() calls create3 only when a gate3 exists)
    assert not S.Circuit(2).has_gate3 and d.gates[0] == (0, 1) and d.gates[1] == (0, 1, 0x7FFFFFFF)


def test_gate3_schedule_and_lanes_in_the_plain_model(S):
    """The third input counts for liveness and levels in Circuit.schedule as in the C planner, and carries a lane
    shift in evaluate_plain."""
    c = S.Circuit(2, group=4)
    x, y = c.inputs
    a = c.gate(x, y)
    dead = c.gate(x, ~y)
    b = c.gate(x, x)
    top = c.gate3(x, y.lane(1), ~b[2].lane(-1))
    c.output(top[2], a[0])
    assert c.schedule() == [[0, 2], [3]] and dead
    info = c.info()
    assert (info["levels"], info["nodes"], info["widest"]) == (2, 3, 2)
    bits = np.random.default_rng(3).integers(0, 2, size=(2, 12)).astype(bool)
    got = c.evaluate_plain(bits)
    for t in range(12):
        xv = bits[0, t]
        yv = bits[1, t + 1] if t % 4 + 1 < 4 else False
        zv = not (False if t % 4 == 0 else (bits[0, t - 1] ^ bits[0, t - 1]))
        assert got[0, t] == (int(xv) + int(yv) + int(zv)) % 2 and got[1, t] == (bits[0, t] and bits[1, t])


@pytest.mark.parametrize("width", [1, 5, 16])
def test_ripple_adder_is_integer_addition(S, width):
    c = S.ripple_adder(width)
    assert c.n_inputs == 2 * width and c.n_outputs == width + 1 and c.n_gates == width and c.has_gate3
    info = c.info()
    assert info["levels"] == width and info["nodes"] == width and info["widest"] == 1
    assert c.schedule() == [[g] for g in range(width)]
    rng = np.random.default_rng(width)
    inst = 40
    xs, ys = rng.integers(0, 2 ** width, size=inst), rng.integers(0, 2 ** width, size=inst)
    xs[0], ys[0] = 2 ** width - 1, 1
    xs[1], ys[1] = 2 ** width - 1, 2 ** width - 1
    xs[2], ys[2] = 0, 0
    bits = np.array([(xs >> i) & 1 for i in range(width)] + [(ys >> i) & 1 for i in range(width)], dtype=bool)
    out = c.evaluate_plain(bits).astype(np.int64)
    assert np.array_equal((out << np.arange(width + 1)[:, None]).sum(axis=0), xs + ys)
    # full_adder returns (sum, carry) = (XOR3, MAJ) of one node
    f = S.Circuit(3)
    s, carry = f.full_adder(*f.inputs)
    assert (s.id, carry.id) == (3 + 2, 3 + 0) and f.n_gates == 1


def test_gate3_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_gate3_sanitized.cpp: circuit_plain_bits of plans with three-input nodes against a
    per-instance evaluation at (G, instances) = (1, 5), (8, 72), (1, 72), (8, 8); the all-NONE plan; refused inputs
    return without allocating.  A child process of its own; the same program without the sanitizers compares as many
    bits."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_gate3_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_gate3_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    tag, compared = r.stdout.split()
    assert tag == "ok" and int(compared) > 50000
    exe2 = str(tmp_path / "circuit_gate3_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
