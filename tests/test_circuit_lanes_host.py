"""Lane-shifted wire references (sgfhe_circuit_create_lanes, include/sgfhe_hip.h) without a
device: the planner's validation through ctypes, Circuit.evaluate_plain against a per-lane loop, packed_adder
against integer addition, and the planner with circuit_plain_bits under ASan / UBSan
(tests/native/circuit_lanes_sanitized.cpp)."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1


def _create_lanes(L, n_inputs, gates, gshift, outs, oshift, group):
    g = np.ascontiguousarray(np.array(gates, dtype=np.uint32).reshape(-1, 2))
    o = np.ascontiguousarray(np.array(outs, dtype=np.uint32))
    gs = None if gshift is None else np.ascontiguousarray(np.array(gshift, dtype=np.int32).reshape(-1, 2))
    os_ = None if oshift is None else np.ascontiguousarray(np.array(oshift, dtype=np.int32))
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p(0xDEAD)
    rc = L.sgfhe_circuit_create_lanes(n_inputs, p(g), p(gs), len(g), p(o), p(os_), len(o), group, ctypes.byref(h))
    return rc, h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def _group(L, h):
    g = ctypes.c_uint32(0)
    assert L.sgfhe_circuit_group(h, ctypes.byref(g)) == 0
    return g.value


def test_create_lanes_validation(S):
    L = S.lib()
    assert "sgfhe_circuit_create_lanes" in S.EXPORTED_SYMBOLS and "sgfhe_circuit_group" in S.EXPORTED_SYMBOLS
    assert L.sgfhe_abi_version() == 7          # functions are only added
    gates = [(0, 1), (2, 0x80000000 | 0), (4, 6)]        # three nodes in a chain, 2 inputs
    outs = [8, 0x80000000 | 9, 0]
    zero_g, zero_o = [(0, 0)] * 3, [0, 0, 0]

    def refused(gshift, oshift, group):
        rc, h = _create_lanes(L, 2, gates, gshift, outs, oshift, group)
        assert rc == ERR_INVALID_ARG and h.value is None, (gshift, oshift, group)

    refused(None, None, 0)                                # group = 0
    refused(zero_g, zero_o, 0)
    for d in (8, -8):                                     # |d| = G
        refused([(0, 0), (d, 0), (0, 0)], None, 8)
        refused([(0, 0), (0, 0), (0, d)], zero_o, 8)
        refused(None, [0, 0, d], 8)
    for d in (1, -1):                                     # group = 1 admits no shift but 0
        refused([(d, 0), (0, 0), (0, 0)], None, 1)
        refused(None, [d, 0, 0], 1)
    refused(None, [0, -2 ** 31, 0], 8)                    # (no |d| in 32 bits)
    # what sgfhe_circuit_create refuses: a node reading its own wire, no outputs
    rc, h = _create_lanes(L, 2, [(0, 2)], None, [2], None, 8)
    assert rc == ERR_INVALID_ARG and h.value is None
    rc, h = _create_lanes(L, 2, gates, None, [], None, 8)
    assert rc == ERR_INVALID_ARG and h.value is None
    assert L.sgfhe_circuit_create_lanes(2, None, None, 0, None, None, 0, 1, None) == ERR_INVALID_ARG
    # accepted: NULL shift arrays, the largest shifts, a shift on the constant; shifts change nothing in the plan's shape
    c = S.Circuit(2)
    c.gates, c.gate_shifts, c.outputs, c.output_shifts = gates, zero_g, outs, zero_o
    base = [c.info()[k] for k in ("levels", "nodes", "widest", "slots")]
    assert base[:3] == [3, 3, 1]
    for gshift, oshift, group in ((None, None, 8), (zero_g, None, 8), (None, zero_o, 1),
                                  ([(7, -7), (0, 0), (-7, 7)], [7, -7, 0], 8), (None, None, 2 ** 32 - 1)):
        rc, h = _create_lanes(L, 2, gates, gshift, outs, oshift, group)
        assert rc == 0 and h.value, (gshift, oshift, group)
        assert _group(L, h) == group
        assert _info(L, h) == base
        L.sgfhe_circuit_destroy(h)
    rc, h = _create_lanes(L, 1, [(0x7FFFFFFF, 0)], [(3, 0)], [0xFFFFFFFF, 1], [-3, 0], 4)
    assert rc == 0 and _group(L, h) == 4
    g = ctypes.c_uint32(5)
    assert L.sgfhe_circuit_group(None, ctypes.byref(g)) == ERR_INVALID_ARG
    assert L.sgfhe_circuit_group(h, None) == ERR_INVALID_ARG
    L.sgfhe_circuit_destroy(h)


def test_zero_shift_group_1_is_the_plain_plan(S):
    """The same arrays through both entries: the same sgfhe_circuit_info, and group 1 from either."""
    L = S.lib()
    rng = np.random.default_rng(5)
    for n_gates in (1, 7, 40):
        gates = [(int(rng.integers(3 + 3 * g)) | (0x80000000 if rng.integers(2) else 0), int(rng.integers(3 + 3 * g)))
                 for g in range(n_gates)]
        outs = [3 + 3 * n_gates - 1, 0x80000000 | 1, 0x7FFFFFFF, 3 + int(rng.integers(3 * n_gates))]
        g = np.ascontiguousarray(np.array(gates, dtype=np.uint32))
        o = np.ascontiguousarray(np.array(outs, dtype=np.uint32))
        h0 = ctypes.c_void_p()
        assert L.sgfhe_circuit_create(3, g.ctypes.data_as(ctypes.c_void_p), n_gates, o.ctypes.data_as(ctypes.c_void_p),
                                      len(outs), ctypes.byref(h0)) == 0
        for gshift, oshift in ((None, None), ([(0, 0)] * n_gates, [0] * len(outs))):
            rc, h1 = _create_lanes(L, 3, gates, gshift, outs, oshift, 1)
            assert rc == 0 and _info(L, h1) == _info(L, h0) and _group(L, h1) == 1
            L.sgfhe_circuit_destroy(h1)
        assert _group(L, h0) == 1
        L.sgfhe_circuit_destroy(h0)


def test_wire_lane_and_circuit_builder(S):
    w = S.Wire(5)
    assert w.lane(0) == w and w.lane(2) != w and w.lane(2).lane(-3) == w.lane(-1)
    assert (~w).lane(3) == ~(w.lane(3)) and (~w.lane(3)).negated and (~w.lane(3)).shift == 3 and w.lane(3).id == 5
    assert hash(w.lane(1)) == hash(S.Wire(5).lane(1)) and len({w, w.lane(1), w.lane(1), ~w.lane(1)}) == 3
    assert "-2" in repr(w.lane(-2)) and repr(w) == "Wire(5)"
    c = S.Circuit(2, group=4)
    x, y = c.inputs
    a, o, xo = c.gate(x.lane(1), ~y.lane(-3))
    c.gate(a, xo.lane(2))
    c.output(~o.lane(-1), x, S.Circuit.TRUE.lane(2))
    assert c.group == 4 and c.gates == [(0, 0x80000001), (2, 4)] and c.gate_shifts == [(1, -3), (0, 2)]
    assert c.outputs == [0x80000003, 0, 0xFFFFFFFF] and c.output_shifts == [-1, 0, 2]
    ctypes_group = ctypes.c_uint32()
    assert S.lib().sgfhe_circuit_group(c.handle(), ctypes.byref(ctypes_group)) == 0 and ctypes_group.value == 4
    with pytest.raises(ValueError):
        c.gate(x.lane(4), y)
    with pytest.raises(ValueError):
        S.Circuit(1).output(S.Wire(0).lane(1))
    with pytest.raises(ValueError):
        S.Circuit(1, group=0)
    plain = S.Circuit(1)                                          # the old entry: group 1
    plain.output(plain.inputs[0])
    assert S.lib().sgfhe_circuit_group(plain.handle(), ctypes.byref(ctypes_group)) == 0 and ctypes_group.value == 1
    with pytest.raises(ValueError):
        c.evaluate_plain(np.zeros((2, 6), bool))                  # 6 instances are no multiple of 4


def _random_lanes_circuit(S, rng, n_inputs, n_gates, group):
    """Random inputs among all earlier wires and the constant, every NOT pattern, shifts from {0, +-1, +-(G - 1),
    anything inside the group}; outputs shifted and negated alike."""
    c = S.Circuit(n_inputs, group=group)
    wires = list(c.inputs)

    def shift():
        if group == 1:
            return 0
        u = int(rng.integers(6))
        return (0, 1, -1, group - 1, -(group - 1), int(rng.integers(-(group - 1), group)))[u]

    def pick():
        w = S.Circuit.FALSE if rng.integers(12) == 0 else wires[int(rng.integers(len(wires)))]
        w = w.lane(shift())
        return ~w if rng.integers(2) else w

    for _ in range(n_gates):
        wires.extend(c.gate(pick(), pick()))
    c.output(*([wires[-1], ~wires[-2].lane(shift()), wires[0].lane(shift())] + [pick() for _ in range(5)]))
    return c


def _brute_force(c, bits):
    """The model of include/sgfhe_hip.h, one lane at a time, over every node in index order."""
    G, inst = c.group, bits.shape[1]
    wire = {i: [bool(v) for v in bits[i]] for i in range(c.n_inputs)}

    def read(ref, d, t):
        i = ref & 0x7FFFFFFF
        v = False
        if i != 0x7FFFFFFF and 0 <= t % G + d < G:
            v = wire[i][t + d]
        return (not v) if ref & 0x80000000 else v

    for g, ((rx, ry), (dx, dy)) in enumerate(zip(c.gates, c.gate_shifts)):
        base = c.n_inputs + 3 * g
        wire[base], wire[base + 1], wire[base + 2] = [], [], []
        for t in range(inst):
            x, y = read(rx, dx, t), read(ry, dy, t)
            wire[base].append(x and y)
            wire[base + 1].append(x or y)
            wire[base + 2].append(x != y)
    return np.array([[read(ref, d, t) for t in range(inst)] for ref, d in zip(c.outputs, c.output_shifts)])


@pytest.mark.parametrize("group", [1, 2, 8, 24])
def test_evaluate_plain_equals_a_per_lane_loop(S, group):
    rng = np.random.default_rng(100 + group)
    for trial in range(6):
        c = _random_lanes_circuit(S, rng, 3, 14, group)
        if group > 1:
            assert any(d for pair in c.gate_shifts for d in pair)
        bits = rng.integers(0, 2, size=(3, 3 * group)).astype(bool)      # three groups
        assert np.array_equal(c.evaluate_plain(bits), _brute_force(c, bits)), (group, trial)


@pytest.mark.parametrize("width", [4, 8, 16])
def test_packed_adder_is_integer_addition(S, width):
    from sgfhe_jl_amd import circuit as C
    c = C.packed_adder(width)
    stages = width.bit_length() - 1
    assert c.group == width and c.n_inputs == 2 and c.n_outputs == 2
    assert c.info()["levels"] == 2 + 2 * stages and c.info()["nodes"] == 1 + 3 * stages    # the last (p, p) is pruned
    assert len(c.schedule()[0]) == 1
    rng = np.random.default_rng(width)
    groups = 9
    xs, ys = rng.integers(0, 2 ** width, size=groups), rng.integers(0, 2 ** width, size=groups)
    xs[0], ys[0] = 2 ** width - 1, 1                                      # all-ones + 1: the carry runs the whole word
    xs[1], ys[1] = 1, 2 ** width - 1
    xs[2], ys[2] = 2 ** width - 1, 2 ** width - 1
    xs[3], ys[3] = 0, 0
    bits = np.array([[(int(v) >> i) & 1 for v in vals for i in range(width)] for vals in (xs, ys)], dtype=bool)
    out = c.evaluate_plain(bits).reshape(2, groups, width).astype(np.int64)
    total = (out[0] << np.arange(width)).sum(axis=1)
    assert np.array_equal(total, (xs + ys) % 2 ** width)
    assert np.array_equal(out[1, :, width - 1], (xs + ys) >> width)


def test_lanes_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_lanes_sanitized.cpp: circuit_plain_bits of lane plans against a per-instance evaluation at
    (G, instances) = (8, 72), (24, 120), (64, 192), (1, 5); refused inputs return without allocating.  A child
    process of its own; the same program without the sanitizers compares as many bits."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_lanes_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_lanes_sanitized")
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
    exe2 = str(tmp_path / "circuit_lanes_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
