"""Data planes without a GPU (sgfhe_circuit_create_data, include/sgfhe_hip.h): the create entry's
validation through ctypes, case by case; sgfhe_circuit_create_lut_multi and sgfhe_circuit_create_lut still refuse kinds 4
and 5; sgfhe_circuit_info of a data plan against the plan with kind 4 read as 2 and kind 5 as 3; sgfhe_circuit_planes; the
ABI revision; Circuit.lut_data, Circuit.plane, evaluate_plain with data against brute force over all 256 table bytes;
circuit.lookup / lookup_data against direct indexing; replay_levels with data against a hand composition; and the planner
and circuit_plain_bits with planes under ASan / UBSan (tests/native/circuit_data_sanitized.cpp)."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT = 0x7FFFFFFF, 0x80000000
INVALID = -1
DATA, MULTI, SINGLE = "sgfhe_circuit_create_data", "sgfhe_circuit_create_lut_multi", "sgfhe_circuit_create_lut"


def _create(L, fn, n_inputs, nodes, outputs, planes=None, group=1):
    """nodes: [(kind, table or plane, [ref, ...])], unit weights, no shifts -> (rc, handle).  planes: n_planes of
    sgfhe_circuit_create_data (None for the other creators, which have no such argument)."""
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
    head = (n_inputs,) if planes is None else (n_inputs, planes)
    rc = getattr(L, fn)(*head, vp(kind), vp(start), vp(refs), vp(shifts), vp(weights), vp(table), len(nodes), vp(outs),
                        vp(oshift), len(outs), group, ctypes.byref(h))
    return rc, h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def _planes(L, h):
    p = ctypes.c_uint32(0xDEAD)
    assert L.sgfhe_circuit_planes(h, ctypes.byref(p)) == 0
    return p.value


# 3 inputs, 2 planes; node 0 = fan(input 0): wires 3, 4, 5 at scales 0, 1, 2; node 1 = data lut(5, ~4, 3) of plane 1: wires
# 6, 7, 8; node 2 its data sibling of plane 0: wires 9, 10, 11; node 3 its constant sibling: wires 12, 13, 14; node 4 =
# lut(11, ~10, 12): wires 15, 16, 17
GOOD = [(2, 0xF0, [FALSE, FALSE, 0]), (4, 1, [5, 4 | NOT, 3]), (5, 0, []), (3, 0x96, []), (2, 0xE8, [11, 10 | NOT, 12])]


def _as_constant(nodes):
    """kind 4 read as 2, kind 5 read as 3 (the plane number serves as the table)."""
    return [({4: 2, 5: 3}.get(k, k), t, r) for k, t, r in nodes]


def test_abi_and_declarations(S):
    L = S.lib()
    assert L.sgfhe_abi_version() == 7 == S.ABI_VERSION              # functions are only added
    for name in (DATA, "sgfhe_circuit_planes", "sgfhe_circuit_run_data", "sgfhe_circuit_run_ct_data",
                 "sgfhe_circuit_run_probe_data"):
        assert name in S.EXPORTED_SYMBOLS and getattr(L, name)
    assert len(getattr(L, DATA).argtypes) == len(getattr(L, MULTI).argtypes) + 1 == 14
    assert len(L.sgfhe_circuit_run_data.argtypes) == 6 and len(L.sgfhe_circuit_run_ct_data.argtypes) == 11
    assert len(L.sgfhe_circuit_run_probe_data.argtypes) == 9
    header = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    assert "#define SGFHE_CIRCUIT_MAX_PLANES 65536u" in header and "#define SGFHE_ABI_VERSION 7u" in header


def test_a_data_plan_its_info_and_its_planes(S):
    L = S.lib()
    for outputs in ([15, 9 | NOT], [6], [12], [15, 6, 9, 12 | NOT]):
        rc, h = _create(L, DATA, 3, GOOD, outputs, planes=2)
        rc2, h2 = _create(L, MULTI, 3, _as_constant(GOOD), outputs)
        assert rc == 0 and rc2 == 0 and h.value and h2.value
        assert _info(L, h) == _info(L, h2)
        assert _planes(L, h) == 2 and _planes(L, h2) == 0
        L.sgfhe_circuit_destroy(h)
        L.sgfhe_circuit_destroy(h2)
    rc, h = _create(L, DATA, 3, GOOD, [15, 9 | NOT], planes=2)
    assert _info(L, h)[:3] == [3, 3, 1]                              # the siblings take no row
    L.sgfhe_circuit_destroy(h)
    # a plane may be used by several nodes or by none; n_planes at the cap
    rc, h = _create(L, DATA, 3, [GOOD[0], (4, 65535, [5, 4, 3]), (5, 65535, []), (5, 7, [])], [9, 12], planes=65536)
    assert rc == 0 and _planes(L, h) == 65536
    L.sgfhe_circuit_destroy(h)
    # no planes and no data kinds: the plan of sgfhe_circuit_create_lut_multi
    const = _as_constant(GOOD)
    rc, h = _create(L, DATA, 3, const, [15, 9 | NOT], planes=0)
    rc2, h2 = _create(L, MULTI, 3, const, [15, 9 | NOT])
    assert rc == 0 and rc2 == 0 and _info(L, h) == _info(L, h2) and _planes(L, h) == 0
    L.sgfhe_circuit_destroy(h)
    L.sgfhe_circuit_destroy(h2)
    assert L.sgfhe_circuit_planes(None, ctypes.byref(ctypes.c_uint32())) == INVALID


def _edit(i, node):
    nodes = list(GOOD)
    nodes[i] = node
    return nodes


MIXED_257 = [GOOD[0], (4, 1, [5, 4, 3])] + [(5, i % 2, []) if i % 2 else (3, i & 0xFF, []) for i in range(256)]


@pytest.mark.parametrize("what, nodes, outputs, planes", [
    ("a node's plane is n_planes", _edit(1, (4, 2, [5, 4 | NOT, 3])), [15], 2),
    ("a sibling's plane is n_planes", _edit(2, (5, 2, [])), [15], 2),
    ("a plane with no planes at all", GOOD, [15], 0),
    ("n_planes above the cap", GOOD, [15], 65537),
    ("kind 6", _edit(2, (6, 0, [])), [6], 2),
    ("a data sibling first", [(5, 0, [])] + GOOD[:2], [9], 2),
    ("a data sibling behind a classic node", [GOOD[0], (0, 0, [3, 3]), (5, 0, [])], [6], 2),
    ("a data sibling behind a sum node", [GOOD[0], (1, 0, [3, 3, 3]), (5, 0, [])], [6], 2),
    ("terms on a data sibling", _edit(2, (5, 0, [FALSE])), [15], 2),
    ("three terms on a data sibling", _edit(2, (5, 0, [5, 4, 3])), [15], 2),
    ("two terms on a data node", _edit(1, (4, 1, [5, 4])), [15], 2),
    ("a family of 257 with mixed members", MIXED_257, [6], 2),
    ("position 0 reads the data sibling's scale-1 wire", _edit(4, (2, 0xE8, [10, 10, 12])), [15], 2),
    ("position 2 reads the data node's scale-2 wire", _edit(4, (2, 0xE8, [11, 10, 8])), [15], 2),
    ("a data node reads a scale-0 wire at position 0", _edit(1, (4, 1, [3, 4, 3])), [15], 2),
    ("a classic node reads the data sibling's scale-1 wire", _edit(4, (0, 0, [9, 10])), [15], 2),
    ("an output of scale 1 of a data node", GOOD, [15, 7], 2),
    ("an output of scale 2 of a data sibling", GOOD, [15, 11 | NOT], 2),
])
def test_validation(S, what, nodes, outputs, planes):
    L = S.lib()
    rc, h = _create(L, DATA, 3, nodes, outputs, planes=planes)
    assert rc == INVALID and not h.value, what


def test_the_largest_mixed_family_is_accepted(S):
    L = S.lib()
    rc, h = _create(L, DATA, 3, MIXED_257[:-1], [6 + 3 * 255], planes=2)
    assert rc == 0 and _info(L, h)[:3] == [2, 2, 1]
    L.sgfhe_circuit_destroy(h)


def test_the_other_entries_still_refuse_kinds_4_and_5(S):
    L = S.lib()
    rc, h = _create(L, DATA, 3, GOOD, [15], planes=2)                          # the arrays the others refuse
    assert rc == 0 and h.value
    L.sgfhe_circuit_destroy(h)
    for fn in (MULTI, SINGLE):
        rc, h = _create(L, fn, 3, GOOD, [15])
        assert rc == INVALID and not h.value
        rc, h = _create(L, fn, 3, [GOOD[0], (4, 1, [5, 4, 3])], [6])          # kind 4 alone
        assert rc == INVALID and not h.value
    rc, h = _create(L, MULTI, 3, [GOOD[0], (2, 1, [5, 4, 3]), (5, 0, [])], [9])   # kind 5 alone
    assert rc == INVALID and not h.value
    rc, h = _create(L, MULTI, 3, _as_constant(GOOD), [15])
    assert rc == 0
    L.sgfhe_circuit_destroy(h)


def _truth(k):
    return np.array([[(i >> j) & 1 for i in range(1 << k)] for j in range(k)], dtype=bool)


def test_lut_data_kinds_schedule_info_and_the_creator(S, monkeypatch):
    c = S.Circuit(3, planes=3)
    assert c.planes == 3
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    fam = c.lut_multi([S.Circuit.plane(2), 0x96, S.Circuit.plane(0), S.Circuit.plane(2), 0x35], fx[2], ~fy[1], fz[0])
    single = c.lut_data(1, fam[1][2], fam[2][1], fam[4][0])
    c.output(single[0], fam[2][0], ~fam[4][0])
    assert [c.kind(g) for g in range(6, 12)] == ["data", "sibling", "data_sibling", "data_sibling", "sibling", "data"]
    assert c.siblings(6) == [7, 8, 9, 10] and c.live_siblings(6) == [7, 8, 10]    # no de-duplication: 9 is plane 2 again
    assert c.schedule() == [[0, 1, 2], [3, 4, 5], [6], [11]]
    assert c.node_levels()[6:12] == [3, 3, 3, 0, 3, 4]
    assert [c.scale(w) for w in fam[2]] == [0, 1, 2] and [c.scale(w) for w in single] == [0, 1, 2]
    # the same circuit with constant tables: the same info
    d = S.Circuit(3)
    rx, ry, rz = (d.refresh(w) for w in d.inputs)
    fx, fy, fz = d.fan(rx), d.fan(ry), d.fan(rz)
    fam = d.lut_multi([2, 0x96, 0, 2, 0x35], fx[2], ~fy[1], fz[0])
    d.output(d.lut(1, fam[1][2], fam[2][1], fam[4][0])[0], fam[2][0], ~fam[4][0])
    called = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("sgfhe_circuit_create"):
                called.append(name)
            return getattr(S.lib(), name)

    import sgfhe_jl_amd._lib as lib_mod
    monkeypatch.setattr(lib_mod, "lib", lambda spy=Spy(): spy)
    assert c.info() == d.info() == dict(levels=4, nodes=8, widest=3, slots=c.info()["slots"])
    assert called == [DATA, MULTI]                                   # only a circuit with planes takes the new creator
    with pytest.raises(ValueError):
        c.lut_data(3, fx[2], fy[1], fz[0])                           # a plane the circuit does not have
    with pytest.raises(ValueError):
        c.lut_multi([0x96, S.Circuit.plane(3)], fx[2], fy[1], fz[0])
    with pytest.raises(ValueError):
        d.lut_data(0, fx[2], fy[1], fz[0])                           # a circuit without planes
    with pytest.raises(ValueError):
        S.Circuit(1, planes=65537)
    with pytest.raises(ValueError):
        c.gate(single[1], c.inputs[0])                               # a data node's wire +1 has scale 1


def test_evaluate_plain_over_every_table_byte_at_one_node(S):
    """One data node and a data sibling over the 8 input combinations x all 256 bytes: 2048 instances."""
    c = S.Circuit(3, planes=2)
    f = [c.fan(w) for w in c.inputs]
    fam = c.lut_multi([S.Circuit.plane(1), S.Circuit.plane(0)], f[0][2], ~f[1][1], f[2][0])
    c.output(fam[0][0], ~fam[1][0])
    bits = np.tile(_truth(3), (1, 256))                              # instance = 8 * byte + combination
    byte = np.repeat(np.arange(256, dtype=np.uint8), 8)
    data = np.stack([byte[::-1].copy(), byte])                       # plane 0: the bytes in reverse order
    s = bits[0].astype(int) + 2 * (~bits[1]).astype(int) + 4 * bits[2].astype(int)
    got = c.evaluate_plain(bits, data)
    assert np.array_equal(got[0], ((data[1] >> s) & 1).astype(bool))
    assert np.array_equal(got[1], ~((data[0] >> s) & 1).astype(bool))
    with pytest.raises(ValueError):
        c.evaluate_plain(bits)                                       # planes and no data
    with pytest.raises(ValueError):
        c.evaluate_plain(bits, data.astype(np.int64))                # the wrong dtype
    with pytest.raises(ValueError):
        c.evaluate_plain(bits, data[:, :-1])                         # the wrong shape
    with pytest.raises(ValueError):
        c.evaluate_plain(bits, data[:1])
    plain = S.Circuit(1)
    plain.output(plain.inputs[0])
    with pytest.raises(ValueError):
        plain.evaluate_plain(np.zeros((1, 4), dtype=bool), np.zeros((1, 4), dtype=np.uint8))


def test_the_table_is_read_at_the_nodes_own_instance(S):
    c = S.Circuit(1, group=4, planes=1)
    f = c.fan(c.inputs[0])
    c.output(c.lut_data(0, f[2].lane(1), ~f[1].lane(-1), f[0].lane(2))[0])
    rng = np.random.default_rng(931)
    bits = rng.integers(0, 2, size=(1, 16)).astype(bool)
    data = rng.integers(0, 256, size=(1, 16), dtype=np.uint8)
    from sgfhe_jl_amd.circuit import lane_shift
    x0 = lane_shift(bits[0], 1, 4).astype(int)
    x1 = (~lane_shift(bits[0], -1, 4)).astype(int)
    x2 = lane_shift(bits[0], 2, 4).astype(int)
    assert np.array_equal(c.evaluate_plain(bits, data)[0], ((data[0] >> (x0 + 2 * x1 + 4 * x2)) & 1).astype(bool))


@pytest.mark.parametrize("k", [3, 4, 6])
@pytest.mark.parametrize("count", [1, 4])
def test_lookup_against_direct_indexing(S, k, count):
    rng = np.random.default_rng(940 + 10 * k + count)
    inst, H, plane0 = 1 << k, 1 << (k - 3), 2
    inst *= 3                                                        # every index three times, under different tables
    tables = [[int.from_bytes(rng.bytes((1 << k) // 8), "little") for _ in range(inst)] for _ in range(count)]
    c = S.Circuit(k, planes=plane0 + count * H + 1)
    outs = S.lookup(c, c.inputs, count=count, plane0=plane0, refresh=True)
    assert len(outs) == count and all(c.scale(w) == 0 for w in outs)
    c.output(*outs)
    planes = S.lookup_data(tables, k)
    assert planes.dtype == np.uint8 and planes.shape == (count * H, inst)
    data = np.concatenate([rng.integers(0, 256, size=(plane0, inst), dtype=np.uint8), planes,
                           rng.integers(0, 256, size=(1, inst), dtype=np.uint8)])
    bits = np.tile(_truth(k), (1, 3))
    x = sum(bits[j].astype(int) << j for j in range(k))
    want = np.array([[(tables[f][t] >> int(x[t])) & 1 for t in range(inst)] for f in range(count)], dtype=bool)
    assert np.array_equal(c.evaluate_plain(bits, data), want)
    # k refreshes, two fans, one family of all count * 2^(k-3) cofactors, then count * (2^(k-3) - 1) muxes, unmerged
    info = c.info()
    assert info["nodes"] == k + 2 + 1 + count * (H - 1) and info["levels"] == 3 + (k - 3)
    assert len(c.schedule()[2]) == 1
    fam = c.schedule()[2][0]
    assert [c.gate_planes[g] for g in [fam] + c.siblings(fam)] == list(range(plane0, plane0 + count * H))


def test_lookup_of_twelve_wires_is_two_families(S):
    c = S.Circuit(12, planes=512)
    (out,) = S.lookup(c, c.inputs)
    c.output(out)
    level = c.schedule()[1]                                          # no refresh: the fans of x0 and x1, then the families
    assert len(level) == 2 and [c.kind(g) for g in level] == ["data", "data"]
    assert [len(c.siblings(g)) for g in level] == [255, 255]
    assert c.gate_planes[level[1]] == 256
    assert c.info()["nodes"] == 2 + 2 + 511 and c.info()["levels"] == 2 + 9
    rng = np.random.default_rng(951)
    inst = 5
    tables = [[int.from_bytes(rng.bytes(512), "little") for _ in range(inst)]]
    x = rng.integers(0, 4096, size=inst)
    bits = np.array([[(int(v) >> j) & 1 for v in x] for j in range(12)], dtype=bool)
    want = np.array([[(tables[0][t] >> int(x[t])) & 1 for t in range(inst)]], dtype=bool)
    assert np.array_equal(c.evaluate_plain(bits, S.lookup_data(tables, 12)), want)
    with pytest.raises(ValueError):
        S.lookup(S.Circuit(12, planes=511), S.Circuit(12).inputs)    # one plane short
    with pytest.raises(ValueError):
        S.lookup(S.Circuit(2, planes=4), S.Circuit(2).inputs)
    with pytest.raises(ValueError):
        S.lookup_data([[1 << 16]], 4)
    with pytest.raises(ValueError):
        S.lookup_data([[1, 2], [3]], 4)


def test_replay_levels_with_data_against_hand_composition(S):
    """boot_lut stands for the primitive as a function of (call, row index, table, row): the replay hands every row of a
    data node the byte of its plane at the row's instance, and a data sibling its leader's rows and indices with its own
    plane's bytes, in the leader's call."""
    from sgfhe_jl_amd import circuit as C
    n, r, inst = 4, 64, 3
    c = S.Circuit(2, planes=3)
    x, y = c.inputs
    fam = c.lut_multi([S.Circuit.plane(2), S.Circuit.plane(0), 0x35], S.Circuit.FALSE, S.Circuit.FALSE, x)   # 0x35 is dead
    g = c.gate(x, ~y)
    top = c.lut_data(1, fam[1][2], S.Circuit.FALSE, g[0])
    c.output(top[0], fam[1][0], fam[0][0])
    assert c.schedule() == [[0, 3], [4]]
    rng = np.random.default_rng(960)
    inputs = rng.integers(0, r, size=(2, inst, n + 1), dtype=np.uint64)
    data = np.array([[0x96, 0x17, 0xE8], [1, 2, 3], [0xCA, 0xAC, 0x53]], dtype=np.uint8)
    seen = []

    def boot(call, a1, b1, a2, b2):
        return np.stack([np.concatenate([a1 + a2, (b1 + b2)[:, None]], axis=1) + np.uint64(k + 10 * call) for k in range(3)],
                        axis=1) & np.uint64(r - 1)

    def boot_lut(call, a, b, tables, idx):
        seen.append((call, list(tables), list(idx)))
        row = np.concatenate([a, b[:, None]], axis=1)
        t = np.asarray(tables, dtype=np.uint64)[:, None] + np.asarray(idx, dtype=np.uint64)[:, None]
        return np.stack([(row + t * np.uint64(k + 1) + np.uint64(call)) & np.uint64(r - 1) for k in range(3)], axis=1)

    got = C.replay_levels(c, inputs, r, boot, boot_lut, data=data)
    assert seen[0] == (0, [0xCA, 0xAC, 0x53], [0, 1, 2]) and seen[1] == (0, [0x96, 0x17, 0xE8], [0, 1, 2])
    assert seen[2] == (1, [1, 2, 3], [0, 1, 2]) and len(seen) == 3
    mask = np.uint64(r - 1)
    idx = np.arange(inst, dtype=np.uint64)[:, None]
    lead = lambda t, k, call, row: (row + (t.astype(np.uint64)[:, None] + idx) * np.uint64(k + 1) + np.uint64(call)) & mask
    xr = inputs[0]
    sib2 = lead(data[0], 2, 0, xr)                            # wire +2 of the data sibling
    not_y = C.lwe_not(inputs[1], r)
    g0 = (xr + not_y) & mask                                  # boot's row 0 at call 0, k = 0
    u = (sib2 + g0) & mask
    assert np.array_equal(got[0], lead(data[1], 0, 1, u))
    assert np.array_equal(got[1], lead(data[0], 0, 0, xr)) and np.array_equal(got[2], lead(data[2], 0, 0, xr))
    with pytest.raises(ValueError):
        C.replay_levels(c, inputs, r, boot, boot_lut)
    with pytest.raises(ValueError):
        C.replay_levels(c, inputs, r, boot, boot_lut, data=data[:, :2])


def test_data_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_data_sanitized.cpp: random circuits with data families, circuit_plain_bits with planes against
    a per-instance evaluation, the plan against its constant twin, the call arithmetic over a call boundary, and the
    refused inputs without an allocation.  A child process of its own, a stand-alone program; the same program without
    the sanitizers compares as many bits."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_data_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_data_sanitized")
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
    exe2 = str(tmp_path / "circuit_data_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
