"""Registers and stepped runs without a GPU (sgfhe_circuit_create_seq, include/sgfhe_hip.h): the
new symbols and the ABI revision; the create entry's validation through ctypes, case by case; a plan with n_regs = 0
against the sgfhe_circuit_create_data plan; the sequential plan's info against the step plan's; sgfhe_circuit_registers;
Circuit(registers=...), next_state, step_plan, scale and the creator a circuit takes; evaluate_plain_steps of
serial_adder and crc16_stream against Python integers and binascii.crc_hqx; replay_steps against a hand composition of
replay_levels; the run entries' argument errors that need no device; and the planner with registers under ASan / UBSan
(tests/native/circuit_steps_sanitized.cpp)."""

import binascii
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT, NONE = 0x7FFFFFFF, 0x80000000, 0x7FFFFFFE
INVALID = -1
SEQ, DATA = "sgfhe_circuit_create_seq", "sgfhe_circuit_create_data"


def _create(L, n_inputs, nodes, outputs, regs=None, group=1, planes=0, out_shift=None):
    """nodes: [(kind, table or plane, [ref, ...])], unit weights, no shifts; regs: None for sgfhe_circuit_create_data, or
    (next_ref, next_shift or None, reg_scale or None) for sgfhe_circuit_create_seq -> (rc, handle)."""
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    kind = np.array([k for k, _, _ in nodes], dtype=np.uint32)
    table = np.array([t for _, t, _ in nodes], dtype=np.uint32)
    start = np.cumsum([0] + [len(r) for _, _, r in nodes]).astype(np.uint32)
    refs = np.array([x for _, _, r in nodes for x in r] + [0], dtype=np.uint32)
    shifts = np.zeros(len(refs), dtype=np.int32)
    weights = np.ones(len(refs), dtype=np.int32)
    outs = np.array(outputs, dtype=np.uint32)
    oshift = np.array(out_shift if out_shift is not None else [0] * len(outs), dtype=np.int32)
    h = ctypes.c_void_p(0xDEAD)
    head = (n_inputs, planes, vp(kind), vp(start), vp(refs), vp(shifts), vp(weights), vp(table), len(nodes), vp(outs),
            vp(oshift), len(outs), group)
    if regs is None:
        return L.sgfhe_circuit_create_data(*head, ctypes.byref(h)), h
    nref, nshift, scale = regs
    keep = [np.array(nref + [0], dtype=np.uint32), None if nshift is None else np.array(nshift + [0], dtype=np.int32),
            None if scale is None else np.array(scale + [0], dtype=np.uint32)]
    return L.sgfhe_circuit_create_seq(*head, len(nref), vp(keep[0]), vp(keep[1]), vp(keep[2]), ctypes.byref(h)), h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def _regs(L, h):
    r = ctypes.c_uint32(0xDEAD)
    assert L.sgfhe_circuit_registers(h, ctypes.byref(r)) == 0
    return r.value


# 3 inputs, registers 0 and 1, stream input 2; node 0 = (input 2, register 0): wires 3, 4, 5; node 1 = (3, register 1):
# wires 6, 7, 8
SMALL = [(0, 0, [2, 0]), (0, 0, [3, 1])]
# 4 inputs: registers 0, 1, 2 of scales 2, 1, 0 and a stream input; node 0 = lut(0x96; reg 0, reg 1, reg 2): wires 4, 5, 6 at
# scales 0, 1, 2; node 1 = classic (stream input, wire 4): wires 7, 8, 9
SCALED = [(2, 0x96, [0, 1, 2]), (0, 0, [3, 4])]


def test_abi_and_declarations(S):
    L = S.lib()
    assert L.sgfhe_abi_version() == 7 == S.ABI_VERSION              # functions are only added
    for name in (SEQ, "sgfhe_circuit_registers", "sgfhe_circuit_run_steps", "sgfhe_circuit_run_steps_ct"):
        assert name in S.EXPORTED_SYMBOLS and getattr(L, name)
    assert len(getattr(L, SEQ).argtypes) == len(getattr(L, DATA).argtypes) + 4 == 18
    assert len(L.sgfhe_circuit_run_steps.argtypes) == 10 and len(L.sgfhe_circuit_run_steps_ct.argtypes) == 16
    header = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    assert "#define SGFHE_ABI_VERSION 7u" in header and "MEASURED, NOT PROVED" in header


def test_a_sequential_plan_its_info_and_its_registers(S):
    L = S.lib()
    rc, h = _create(L, 3, SMALL, [3], regs=([6 | NOT, 0], [0, 0], [0, 0]))
    assert rc == 0 and h.value and _regs(L, h) == 2
    # the step plan: no registers, outputs ++ next_ref -- the same levels, nodes, widest level and slots
    rc2, h2 = _create(L, 3, SMALL, [3, 6 | NOT, 0])
    assert rc2 == 0 and _info(L, h) == _info(L, h2) == [2, 2, 1, _info(L, h)[3]] and _regs(L, h2) == 0
    L.sgfhe_circuit_destroy(h)
    L.sgfhe_circuit_destroy(h2)
    # node 1 is reached only through next_ref: without it, it is pruned
    rc, h = _create(L, 3, SMALL, [3], regs=([3, 0], None, None))
    assert rc == 0 and _info(L, h)[:2] == [1, 1]
    L.sgfhe_circuit_destroy(h)
    # n_regs = 0: the sgfhe_circuit_create_data plan
    for outputs in ([3], [6 | NOT, 0], [8, FALSE]):
        rc, h = _create(L, 3, SMALL, outputs, regs=([], None, None))
        rc2, h2 = _create(L, 3, SMALL, outputs)
        assert rc == 0 and rc2 == 0 and _info(L, h) == _info(L, h2) and _regs(L, h) == 0
        L.sgfhe_circuit_destroy(h)
        L.sgfhe_circuit_destroy(h2)
    # every input a register; a lane-shifted next state at the edge of the group
    rc, h = _create(L, 3, SMALL, [3], regs=([6, 2, 1 | NOT], [3, -3, 0], None), group=4)
    assert rc == 0 and _regs(L, h) == 3
    L.sgfhe_circuit_destroy(h)
    # scaled registers, a constant at any scale, a register holding itself
    for nref in ([6, 5 | NOT, 4], [FALSE, FALSE | NOT, FALSE], [0, 1 | NOT, 2]):
        rc, h = _create(L, 4, SCALED, [7], regs=(nref, None, [2, 1, 0]))
        assert rc == 0 and _regs(L, h) == 3, nref
        L.sgfhe_circuit_destroy(h)
    assert L.sgfhe_circuit_registers(None, ctypes.byref(ctypes.c_uint32())) == INVALID
    rc, h = _create(L, 3, SMALL, [3])
    assert L.sgfhe_circuit_registers(h, None) == INVALID
    L.sgfhe_circuit_destroy(h)


@pytest.mark.parametrize("what, n_inputs, nodes, outputs, regs, group", [
    ("n_regs above n_inputs", 3, SMALL, [3], ([6, 0, 0, 0], None, None), 1),
    ("a next state out of range", 3, SMALL, [3], ([9, 0], None, None), 1),
    ("a negated next state out of range", 3, SMALL, [3], ([6, 9 | NOT], None, None), 1),
    ("a next state carrying SGFHE_CIRCUIT_NONE", 3, SMALL, [3], ([NONE, 0], None, None), 1),
    ("a negated SGFHE_CIRCUIT_NONE", 3, SMALL, [3], ([6, NONE | NOT], None, None), 1),
    ("a shift of the group size", 3, SMALL, [3], ([6, 0], [4, 0], None), 4),
    ("a shift below minus the group", 3, SMALL, [3], ([6, 0], [0, -5], None), 4),
    ("any shift without a group", 3, SMALL, [3], ([6, 0], [1, 0], None), 1),
    ("reg_scale 3", 3, SMALL, [3], ([6, 0], None, [0, 3]), 1),
    ("no outputs", 3, SMALL, [], ([6, 0], None, None), 1),
    ("a scale-2 register fed a scale-1 wire", 4, SCALED, [7], ([5, 5, 4], None, [2, 1, 0]), 1),
    ("a scale-0 register fed a scale-2 wire", 4, SCALED, [7], ([6, 5, 6], None, [2, 1, 0]), 1),
    ("a scale-0 register fed a scale-1 register", 4, SCALED, [7], ([6, 5, 1], None, [2, 1, 0]), 1),
    ("a scale-1 register fed the stream input", 4, SCALED, [7], ([6, 3, 4], None, [2, 1, 0]), 1),
    ("a scale-1 register read by a classic node", 4, [SCALED[0], (0, 0, [3, 1])], [7], ([6, 5, 4], None, [2, 1, 0]), 1),
    ("a scale-1 register read by a classic node, no LUT node", 3, SMALL, [3], ([FALSE, 0], None, [1, 0]), 1),
    ("position 0 reads a scale-0 register", 4, [(2, 0x96, [2, 1, 2]), SCALED[1]], [7], ([6, 5, 4], None, [2, 1, 0]), 1),
    ("an output names a scale-2 register", 4, SCALED, [0], ([6, 5, 4], None, [2, 1, 0]), 1),
])
def test_validation(S, what, n_inputs, nodes, outputs, regs, group):
    L = S.lib()
    rc, h = _create(L, n_inputs, nodes, outputs, regs=regs, group=group)
    assert rc == INVALID and h.value is None, what


def test_null_next_ref_and_null_out(S):
    L = S.lib()
    z = np.zeros(4, dtype=np.uint32)
    p = z.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p(0xDEAD)
    kind, start = np.zeros(1, np.uint32), np.array([0, 2], np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    w = np.ones(2, np.int32)
    args = (2, 0, vp(kind), vp(start), p, None, vp(w), p, 1, p, None, 1, 1)
    assert L.sgfhe_circuit_create_seq(*args, 1, None, None, None, ctypes.byref(h)) == INVALID and h.value is None
    assert L.sgfhe_circuit_create_seq(*args, 0, None, None, None, None) == INVALID
    h = ctypes.c_void_p(0xDEAD)
    assert L.sgfhe_circuit_create_seq(*args, 0, None, None, None, ctypes.byref(h)) == 0 and h.value   # no registers: no arrays
    L.sgfhe_circuit_destroy(h)


def test_run_entries_refuse_without_a_device(S):
    """What the run entries answer before they look at the ctx's device state: a NULL ctx."""
    L = S.lib()
    assert L.sgfhe_circuit_run_steps(None, None, 0, 0, None, None, None, None, None, None) == INVALID
    assert L.sgfhe_circuit_run_steps_ct(None, None, 0, 0, None, None, None, None, 64, None, None, None, None, None, None,
                                        0) == INVALID


def test_circuit_registers_next_state_and_the_creator(S, monkeypatch):
    c = S.Circuit(4, group=4, registers=2)
    assert c.n_regs == 2 and c.registers == c.inputs[:2] and c.stream_inputs == c.inputs[2:]
    a, o, x = c.gate(c.registers[0], c.stream_inputs[0])
    hi, mid, low = c.sum_node([(1, c.registers[1]), (2, a)])
    c.output(x, c.registers[1])
    assert c.schedule() == [[0]]                                     # the sum node waits for next_state
    c.next_state(~mid.lane(-1), c.stream_inputs[1].lane(2))
    assert c.schedule() == [[0], [1]] and c.node_levels() == [1, 2]
    assert c.next_refs == [mid.id | NOT, 3] and c.next_shifts == [-1, 2]
    sp = c.step_plan()
    assert sp.n_regs == 0 and sp.outputs == c.outputs + c.next_refs and sp.output_shifts == [0, 0, -1, 2]
    assert sp.schedule() == c.schedule()
    called = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("sgfhe_circuit_create"):
                called.append(name)
            return getattr(S.lib(), name)

    import sgfhe_jl_amd._lib as lib_mod
    monkeypatch.setattr(lib_mod, "lib", lambda spy=Spy(): spy)
    assert c.info() == sp.info() == dict(levels=2, nodes=2, widest=1, slots=c.info()["slots"])
    d = S.Circuit(2)
    d.output(d.gate(*d.inputs)[0])
    d.info()
    assert called == [SEQ, "sgfhe_circuit_create_w", "sgfhe_circuit_create"]   # only a circuit with registers takes the new one
    with pytest.raises(ValueError):
        c.next_state(mid)                                            # one wire per register
    with pytest.raises(ValueError):
        c.next_state(mid.lane(4), mid)                               # a shift outside the group
    with pytest.raises(ValueError):
        S.Circuit(2, registers=3)
    with pytest.raises(ValueError):
        S.Circuit(2, registers=1, reg_scales=[3])
    with pytest.raises(ValueError):
        S.Circuit(2, registers=2, reg_scales=[0])
    # scales
    e = S.Circuit(4, registers=3, reg_scales=[2, 1, 0])
    assert [e.scale(w) for w in e.inputs] == [2, 1, 0, 0]
    f0, f1, f2 = e.lut(0x96, *e.registers)                           # a scale-2 register at position 0, no fan
    e.output(e.gate(e.stream_inputs[0], f0)[0])
    e.next_state(f2, ~f1, f0)
    assert e.info()["nodes"] == 2
    with pytest.raises(ValueError):
        e.next_state(f0, f1, f2)                                     # scale 0 into the scale-2 register
    with pytest.raises(ValueError):
        e.gate(e.registers[1], e.stream_inputs[0])                   # a classic node reads scale 0 only
    with pytest.raises(ValueError):
        e.step_plan()
    e.next_state(S.Circuit.FALSE, S.Circuit.TRUE, S.Circuit.FALSE)   # a constant fits every scale


def test_serial_adder_adds_16_bit_numbers(S):
    c = S.serial_adder()
    assert c.n_regs == 1 and c.n_inputs == 3 and c.info() == dict(levels=1, nodes=1, widest=1, slots=c.info()["slots"])
    rng = np.random.default_rng(5)
    x = np.concatenate([[0, 0xFFFF, 0xFFFF, 0x8000], rng.integers(0, 1 << 16, 60)])
    y = np.concatenate([[0, 0xFFFF, 1, 0x8000], rng.integers(0, 1 << 16, 60)])
    stream = np.array([[(x >> i) & 1, (y >> i) & 1] for i in range(16)], dtype=bool)
    outs, state = c.evaluate_plain_steps(None, stream)
    assert outs.shape == (16, 1, 64) and state.shape == (1, 64)
    total = sum(outs[i, 0].astype(np.int64) << i for i in range(16)) + (state[0].astype(np.int64) << 16)
    assert (total == x + y).all()
    # a carry-in of 1, and a run in two parts through the state
    outs1, st1 = c.evaluate_plain_steps(np.ones((1, 64), dtype=bool), stream[:7])
    outs2, st2 = c.evaluate_plain_steps(st1, stream[7:])
    total = sum(np.concatenate([outs1, outs2])[i, 0].astype(np.int64) << i for i in range(16)) + (st2[0].astype(np.int64) << 16)
    assert (total == x + y + 1).all()


@pytest.mark.parametrize("chunk_bits", [8, 16])
def test_crc16_stream_against_binascii(S, chunk_bits):
    c = S.crc16_stream(chunk_bits)
    assert c.n_regs == 16 and c.n_inputs == 16 + chunk_bits and c.n_outputs == 16
    assert c.info()["nodes"] == 16 + chunk_bits and c.info()["levels"] == 2
    assert c.outputs == c.next_refs
    rng = np.random.default_rng(chunk_bits)
    msgs = [bytes(rng.integers(0, 256, 8).astype(np.uint8)) for _ in range(24)] + [bytes(8), b"\xff" * 8]
    bits = np.stack([np.unpackbits(np.frombuffer(m, np.uint8)) for m in msgs], axis=1)      # [64][instances]
    stream = bits.reshape(64 // chunk_bits, chunk_bits, len(msgs)).astype(bool)
    outs, state = c.evaluate_plain_steps(None, stream)
    crc = [sum(int(state[k, t]) << k for k in range(16)) for t in range(len(msgs))]
    assert crc == [binascii.crc_hqx(m, 0) for m in msgs]
    assert (outs[-1] == state).all()
    # every prefix: the outputs of step s are the CRC of the first s + 1 chunks
    for s in range(stream.shape[0]):
        got = [sum(int(outs[s, k, t]) << k for k in range(16)) for t in range(len(msgs))]
        assert got == [binascii.crc_hqx(m[:(s + 1) * chunk_bits // 8], 0) for m in msgs]
    # a non-zero initial value
    init = np.array([[(0x1D0F >> k) & 1] * len(msgs) for k in range(16)], dtype=bool)
    _, state = c.evaluate_plain_steps(init, stream)
    assert [sum(int(state[k, t]) << k for k in range(16)) for t in range(len(msgs))] == [binascii.crc_hqx(m, 0x1D0F) for m in msgs]


def test_evaluate_plain_steps_outputs_before_feedback_lanes_and_data(S):
    """Outputs show the registers the step started with; a swap, a held register, NOT, a lane-shifted stream input and
    TRUE as next states; per-step planes."""
    c = S.Circuit(6, group=4, registers=5)
    r, (x,) = c.registers, c.stream_inputs
    c.output(*r)
    c.next_state(r[1], r[0], ~r[2], x.lane(1), S.Circuit.TRUE)
    rng = np.random.default_rng(3)
    st = rng.integers(0, 2, (5, 8)).astype(bool)
    xs = rng.integers(0, 2, (4, 1, 8)).astype(bool)
    outs, end = c.evaluate_plain_steps(st, xs)
    want = st.copy()
    for s in range(4):
        assert (outs[s] == want).all()
        sh = np.zeros(8, dtype=bool)
        sh[[0, 1, 2, 4, 5, 6]] = xs[s, 0][[1, 2, 3, 5, 6, 7]]
        want = np.stack([want[1], want[0], ~want[2], sh, np.ones(8, dtype=bool)])
    assert (end == want).all()
    # planes per step
    d = S.Circuit(2, planes=1, registers=1)
    f = d.fan(d.stream_inputs[0])
    g = d.fan(d.registers[0])
    t = d.lut_data(0, S.Circuit.FALSE, g[1], f[0])
    d.output(t[0])
    d.next_state(t[0])
    data = rng.integers(0, 256, (3, 1, 5)).astype(np.uint8)
    xs = rng.integers(0, 2, (3, 1, 5)).astype(bool)
    outs, end = d.evaluate_plain_steps(None, xs, data=data)
    reg = np.zeros(5, dtype=np.int64)
    for s in range(3):
        reg = (data[s, 0].astype(np.int64) >> (2 * reg + 4 * xs[s, 0])) & 1
        assert (outs[s, 0] == reg.astype(bool)).all()
    with pytest.raises(ValueError):
        d.evaluate_plain_steps(None, xs, data=data[:2])
    with pytest.raises(ValueError):
        d.evaluate_plain_steps(None, xs)


def test_replay_steps_against_hand_composition(S):
    """replay_steps is replay_levels of the step plan, step by step, the call counter running on; NOT of a next state
    at the register's codeword."""
    from sgfhe_jl_amd import circuit as C
    r, n, inst = 1 << 10, 4, 3
    rng = np.random.default_rng(11)
    c = S.Circuit(3, registers=2)
    a, o, x = c.gate(c.registers[0], c.stream_inputs[0])
    b = c.gate(a, c.registers[1])
    c.output(x, c.registers[0])
    c.next_state(~b[1], a)
    calls = []

    def boot(call, a1, b1, a2, b2):   # a deterministic stand-in: three affine images of the inputs, keyed by the call
        calls.append(call)
        rows = np.concatenate([a1 + a2, (b1 + b2)[:, None]], axis=1).astype(np.uint64)
        return np.stack([(rows * np.uint64(3 + g) + np.uint64(call + g)) & np.uint64(r - 1) for g in range(3)], axis=1)

    state = rng.integers(0, r, (2, inst, n + 1)).astype(np.uint64)
    stream = rng.integers(0, r, (3, 1, inst, n + 1)).astype(np.uint64)
    outs, end = C.replay_steps(c, state, stream, r, boot)
    assert calls == [0, 1, 2, 3, 4, 5]
    sp, cur, at = c.step_plan(), state, [0]

    def boot_from(call, *args):
        return boot(call + at[0], *args)

    for s in range(3):
        res = C.replay_levels(sp, np.concatenate([cur, stream[s]]), r, boot_from)
        at[0] += 2
        assert (outs[s] == res[:2]).all() and (outs[s, 1] == cur[0]).all()
        cur = res[2:]
    assert (end == cur).all()
    outs2, end2 = C.replay_steps(c, state, stream, r, boot, emit=[0, 1, 0])
    assert outs2.shape[0] == 1 and (outs2[0] == outs[1]).all() and (end2 == end).all()
    # a scaled register: NOT at Dr/4, not at Dr
    e = S.Circuit(1, registers=1, reg_scales=[2])
    e.output(S.Circuit.FALSE)
    e.next_state(~e.registers[0])
    st = rng.integers(0, r, (1, inst, n + 1)).astype(np.uint64)
    _, end = C.replay_steps(e, st, np.zeros((1, 0, inst, n + 1), np.uint64), r, boot)
    assert (end == C.lwe_not(st, r, one=r // 16)).all()


def test_seq_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_steps_sanitized.cpp: random circuits with registers against their step plans, n_regs = 0
    against the data plan, and the refused inputs.  A stand-alone program run as a child process, the sanitizers' runtimes
    linked into it; the same program without sanitizers counts the allocations of the refusals and compares as much."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_steps_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_steps_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                        "-I", inc, src, "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("sanitize" in b.stderr or "libasan" in b.stderr or "libubsan" in b.stderr) and \
            "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    tag, compared = r.stdout.split()
    assert tag == "ok" and int(compared) > 50000
    exe2 = str(tmp_path / "circuit_steps_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-DCOUNT_ALLOCATIONS", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe2],
                   check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
