"""LUT families without a GPU (sgfhe_circuit_create_lut_multi, include/sgfhe_hip.h): the create
entry's validation through ctypes, case by case; sgfhe_circuit_create_lut still refuses kind 3; the ABI revision;
Circuit.lut_multi, info, schedule, evaluate_plain and circuit.shannon against brute-force truth tables; replay_levels
with families against a hand composition; and the planner, circuit_plain_bits and the call arithmetic under ASan / UBSan
(tests/native/circuit_lut_multi_sanitized.cpp)."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT = 0x7FFFFFFF, 0x80000000
INVALID = -1


def _create(L, fn, n_inputs, nodes, outputs, group=1):
    """nodes: [(kind, table, [ref, ...])], unit weights, no shifts -> (rc, handle)."""
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kind = np.array([k for k, _, _ in nodes], dtype=np.uint32)
    table = np.array([t for _, t, _ in nodes], dtype=np.uint32)
    start = np.cumsum([0] + [len(r) for _, _, r in nodes]).astype(np.uint32)
    refs = np.array([x for _, _, r in nodes for x in r] + [0], dtype=np.uint32)
    shifts = np.zeros(len(refs), dtype=np.int32)
    weights = np.ones(len(refs), dtype=np.int32)
    outs = np.array(outputs, dtype=np.uint32)
    oshift = np.zeros(len(outs), dtype=np.int32)
    h = ctypes.c_void_p(0xDEAD)
    rc = getattr(L, fn)(n_inputs, vp(kind), vp(start), vp(refs), vp(shifts), vp(weights), vp(table), len(nodes), vp(outs),
                        vp(oshift), len(outs), group, ctypes.byref(h))
    return rc, h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


# 3 inputs; node 0 = fan(input 0): wires 3, 4, 5 at scales 0, 1, 2; node 1 = lut(5, ~4, 3): wires 6, 7, 8; node 2 its
# sibling: wires 9, 10, 11; node 3 = lut(11, ~10, 9): wires 12, 13, 14
GOOD = [(2, 0xF0, [FALSE, FALSE, 0]), (2, 0xCA, [5, 4 | NOT, 3]), (3, 0x96, []), (2, 0xE8, [11, 10 | NOT, 9])]
MULTI, SINGLE = "sgfhe_circuit_create_lut_multi", "sgfhe_circuit_create_lut"


def test_abi_and_declaration(S):
    L = S.lib()
    assert L.sgfhe_abi_version() == 7 == S.ABI_VERSION              # functions are only added
    assert MULTI in S.EXPORTED_SYMBOLS and len(getattr(L, MULTI).argtypes) == len(getattr(L, SINGLE).argtypes) == 13


def test_a_family_plan_and_its_info(S):
    L = S.lib()
    rc, h = _create(L, MULTI, 3, GOOD, [12, 9 | NOT])
    assert rc == 0 and h.value
    # levels; bootstraps (the sibling takes no row); widest; slots: input 0, wire 3, 4, 5, then 9, 10, 11, then 12
    assert _info(L, h)[:3] == [3, 3, 1]
    L.sgfhe_circuit_destroy(h)
    # a dead sibling changes nothing: the plan of the arrays without it
    rc, h = _create(L, MULTI, 3, GOOD[:3], [6])
    rc2, h2 = _create(L, SINGLE, 3, GOOD[:2], [6])
    assert rc == 0 and rc2 == 0 and _info(L, h) == _info(L, h2) == [2, 2, 1, _info(L, h)[3]]
    L.sgfhe_circuit_destroy(h)
    L.sgfhe_circuit_destroy(h2)


def _edit(i, node):
    nodes = list(GOOD)
    nodes[i] = node
    return nodes


@pytest.mark.parametrize("what, nodes, outputs", [
    ("terms on a sibling", _edit(2, (3, 0x96, [FALSE])), [12]),
    ("three terms on a sibling", _edit(2, (3, 0x96, [5, 4, 3])), [12]),
    ("a sibling first", [(3, 0x96, [])] + GOOD[:2], [9]),
    ("a sibling behind a classic node", [GOOD[0], (0, 0, [3, 3]), (3, 0x96, [])], [6]),
    ("a sibling behind a sum node", [GOOD[0], (1, 0, [3, 3, 3]), (3, 0x96, [])], [6]),
    ("table 256", _edit(2, (3, 256, [])), [12]),
    ("kind 4", _edit(2, (4, 0x96, [])), [6]),
    ("a family of 257", [GOOD[0], GOOD[1]] + [(3, 0x96, [])] * 256, [6]),
    ("position 0 reads the sibling's scale-1 wire", _edit(3, (2, 0xE8, [10, 10, 9])), [12]),
    ("position 2 reads the sibling's scale-2 wire", _edit(3, (2, 0xE8, [11, 10, 11])), [12]),
    ("a classic node reads the sibling's scale-1 wire", _edit(3, (0, 0, [9, 10])), [12]),
    ("an output of scale 2", GOOD, [12, 11]),
])
def test_validation(S, what, nodes, outputs):
    L = S.lib()
    rc, h = _create(L, MULTI, 3, nodes, outputs)
    assert rc == INVALID and not h.value, what


def test_the_largest_family_is_accepted(S):
    L = S.lib()
    rc, h = _create(L, MULTI, 3, [GOOD[0], GOOD[1]] + [(3, t, []) for t in range(255)], [6 + 3 * 255])
    assert rc == 0 and _info(L, h)[:3] == [2, 2, 1]
    L.sgfhe_circuit_destroy(h)


def test_the_other_entries_still_refuse_kind_3(S):
    L = S.lib()
    rc, h = _create(L, SINGLE, 3, GOOD, [12])
    assert rc == INVALID and not h.value
    rc, h = _create(L, SINGLE, 3, GOOD[:2], [6])
    assert rc == 0
    L.sgfhe_circuit_destroy(h)
    # sgfhe_circuit_create_w has no node_table
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kind = np.array([1, 3], dtype=np.uint32)
    start = np.array([0, 1, 1], dtype=np.uint32)
    refs, sh, w = np.array([0], dtype=np.uint32), np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32)
    outs, osh = np.array([1], dtype=np.uint32), np.zeros(1, dtype=np.int32)
    h = ctypes.c_void_p(0xDEAD)
    assert L.sgfhe_circuit_create_w(1, vp(kind), vp(start), vp(refs), vp(sh), vp(w), 2, vp(outs), vp(osh), 1, 1,
                                    ctypes.byref(h)) == INVALID and not h.value


def _truth(k):
    return np.array([[(i >> j) & 1 for i in range(1 << k)] for j in range(k)], dtype=bool)


def test_lut_multi_schedule_info_and_plain_evaluation(S):
    c = S.Circuit(3)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    tables = [0xCA, 0x96, 0xE8, 0x00, 0x35]
    fam = c.lut_multi(tables, fx[2], ~fy[1], fz[0])
    later = c.lut(0x96, fam[1][2], fam[2][1], fam[4][0])
    c.output(later[0], fam[2][0], ~fam[4][0])
    assert [c.kind(g) for g in range(6, 12)] == ["lut"] + ["sibling"] * 4 + ["lut"]
    assert c.siblings(6) == [7, 8, 9, 10] and c.live_siblings(6) == [7, 8, 10]          # 0x00 is read by nothing
    assert c.schedule() == [[0, 1, 2], [3, 4, 5], [6], [11]]                            # the leader through its siblings
    assert c.node_levels()[6:12] == [3, 3, 3, 0, 3, 4]
    assert c.info() == dict(levels=4, nodes=8, widest=3, slots=c.info()["slots"])
    assert [c.scale(w) for w in fam[3]] == [0, 1, 2]
    bits = _truth(3)
    x0, x1, x2 = bits[0].astype(int), (~bits[1]).astype(int), bits[2].astype(int)
    f = lambda t, a, b, d: (t >> (a + 2 * b + 4 * d)) & 1
    s = x0 + 2 * x1 + 4 * x2
    want_later = f(0x96, (0x96 >> s) & 1, (0xE8 >> s) & 1, (0x35 >> s) & 1)
    got = c.evaluate_plain(bits)
    assert np.array_equal(got, np.array([want_later, (0xE8 >> s) & 1, 1 - ((0x35 >> s) & 1)], dtype=bool))
    with pytest.raises(ValueError):
        c.lut_multi([], fx[2], fy[1], fz[0])
    with pytest.raises(ValueError):
        c.lut_multi([0] * 257, fx[2], fy[1], fz[0])
    with pytest.raises(ValueError):
        c.lut_multi([256], fx[2], fy[1], fz[0])
    with pytest.raises(ValueError):
        c.gate(fam[1][1], rx)                     # a sibling's wire +1 has scale 1


def test_a_circuit_without_siblings_takes_the_entry_it_took(S, monkeypatch):
    c = S.Circuit(1)
    f = c.fan(c.inputs[0])
    c.output(c.lut_multi([0x96], f[2], f[1], f[0])[0][0])
    assert not c.has_sibling
    called = []

    class Spy:
        def __getattr__(self, name):
            if name == "sgfhe_circuit_create_lut_multi":
                called.append(name)
            return getattr(S.lib(), name)

    import sgfhe_jl_amd._lib as lib_mod
    monkeypatch.setattr(lib_mod, "lib", lambda spy=Spy(): spy)
    assert c.info()["nodes"] == 2 and not called
    d = S.Circuit(1)
    f = d.fan(d.inputs[0])
    d.output(d.lut_multi([0x96, 0x17], f[2], f[1], f[0])[1][0])
    assert d.info()["nodes"] == 2 and called


@pytest.mark.parametrize("k", [3, 4, 5, 6])
def test_shannon_against_brute_force(S, k):
    rng = np.random.default_rng(900 + k)
    full = (1 << (1 << k)) - 1
    tables = [int.from_bytes(rng.bytes((1 << k) // 8), "little") for _ in range(5)] + [0, full, 0xAA & full | 0xAA << 8 & full]
    want = np.array([[(t >> i) & 1 for i in range(1 << k)] for t in tables], dtype=bool)
    nodes = {}
    for family in (True, False):
        c = S.Circuit(k)
        outs = S.shannon(c, tables, c.inputs, refresh=True, family=family)
        assert len(outs) == len(tables) and all(c.scale(w) in (None, 0) for w in outs)
        c.output(*outs)
        assert np.array_equal(c.evaluate_plain(_truth(k)), want), (k, family)
        info = c.info()
        assert info["nodes"] == sum(len(level) for level in c.schedule())
        assert info["levels"] == 3 + (k - 3)
        nodes[family] = info["nodes"]
        # all cofactors of all functions: one family, so level 3 is one bootstrap
        assert len(c.schedule()[2]) == (1 if family else len({(t >> (8 * h)) & 0xFF for t in tables
                                                               for h in range(1 << (k - 3))} - {0, 0xFF}))
    assert nodes[True] < nodes[False]
    with pytest.raises(ValueError):
        S.shannon(S.Circuit(2), [0], S.Circuit(2).inputs)


def test_shannon_reads_wires_at_their_scale_only_where_needed(S):
    """Wires that already have the scale they are read at cost nothing: x0 at scale 2, x1 at scale 1, x2 at scale 0."""
    c = S.Circuit(3)
    f0, f1 = c.fan(c.inputs[0]), c.fan(c.inputs[1])
    before = c.n_gates
    (out,) = S.shannon(c, [0x96], [f0[2], f1[1], c.inputs[2]])
    assert c.n_gates == before + 1 and c.kind(before) == "lut"
    c.output(out)
    assert np.array_equal(c.evaluate_plain(_truth(3))[0], np.array([(0x96 >> i) & 1 for i in range(8)], dtype=bool))
    # a scale-1 wire read at scale 2 goes through one LUT node at its own position
    d = S.Circuit(3)
    g0, g1 = d.fan(d.inputs[0]), d.fan(d.inputs[1])
    (out,) = S.shannon(d, [0xE8], [g0[1], g1[1], d.inputs[2]])
    d.output(out)
    assert d.info()["nodes"] == 4
    assert np.array_equal(d.evaluate_plain(_truth(3))[0], np.array([(0xE8 >> i) & 1 for i in range(8)], dtype=bool))


def test_replay_levels_with_families_against_hand_composition(S):
    """boot_lut stands for the primitive as a function of (call, row index, table, row): the replay hands a sibling its
    leader's rows and indices with its own table, in the leader's call."""
    from sgfhe_jl_amd import circuit as C
    n, r, inst = 4, 64, 3
    c = S.Circuit(2)
    x, y = c.inputs
    fam = c.lut_multi([0xCA, 0x96, 0x35], S.Circuit.FALSE, S.Circuit.FALSE, x)       # sibling 0x35 is dead
    g = c.gate(x, ~y)
    top = c.lut(0xE8, fam[1][2], S.Circuit.FALSE, g[0])
    c.output(top[0], fam[1][0], fam[0][0])
    assert c.schedule() == [[0, 3], [4]]
    rng = np.random.default_rng(910)
    inputs = rng.integers(0, r, size=(2, inst, n + 1), dtype=np.uint64)
    seen = []

    def boot(call, a1, b1, a2, b2):
        return np.stack([np.concatenate([a1 + a2, (b1 + b2)[:, None]], axis=1) + np.uint64(k + 10 * call) for k in range(3)],
                        axis=1) & np.uint64(r - 1)

    def boot_lut(call, a, b, tables, idx):
        seen.append((call, list(tables), list(idx)))
        row = np.concatenate([a, b[:, None]], axis=1)
        t = np.asarray(tables, dtype=np.uint64)[:, None] + np.asarray(idx, dtype=np.uint64)[:, None]
        return np.stack([(row + t * np.uint64(k + 1) + np.uint64(call)) & np.uint64(r - 1) for k in range(3)], axis=1)

    got = C.replay_levels(c, inputs, r, boot, boot_lut)
    # call 0: rows 0..2 the leader (its own table), rows 3..5 the gate; then the live sibling at the leader's rows
    assert seen[0] == (0, [0xCA] * 3, [0, 1, 2]) and seen[1] == (0, [0x96] * 3, [0, 1, 2])
    assert seen[2] == (1, [0xE8] * 3, [0, 1, 2]) and len(seen) == 3
    mask = np.uint64(r - 1)
    idx = np.arange(inst, dtype=np.uint64)[:, None]
    lead = lambda t, k, call, row: (row + (np.uint64(t) + idx) * np.uint64(k + 1) + np.uint64(call)) & mask
    xr = inputs[0]
    sib2 = lead(0x96, 2, 0, xr)                               # wire +2 of the sibling
    not_y = C.lwe_not(inputs[1], r)
    g0 = (xr + not_y) & mask                                  # boot's row 0 at call 0, k = 0
    u = (sib2 + g0) & mask
    assert np.array_equal(got[0], lead(0xE8, 0, 1, u))
    assert np.array_equal(got[1], lead(0x96, 0, 0, xr)) and np.array_equal(got[2], lead(0xCA, 0, 0, xr))


def test_family_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_lut_multi_sanitized.cpp: random circuits with families, circuit_plain_bits against a
    per-instance evaluation, the model restated from the arrays, the call arithmetic over a call boundary, and the
    refused inputs without an allocation.  A child process of its own, a stand-alone program; the same program without
    the sanitizers compares as many bits."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_lut_multi_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_lut_multi_sanitized")
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
    exe2 = str(tmp_path / "circuit_lut_multi_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
