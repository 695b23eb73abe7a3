"""Lane masks without a GPU (sgfhe_circuit_create_masked, include/sgfhe_hip.h): the new symbols and
the ABI revision; every refusal of the create entry through ctypes, with *out NULL; a plan with n_masks = 0 against the
sgfhe_circuit_create_routed plan (its info here, its image word for word in the native program); sgfhe_circuit_masks;
evaluate_plain against a per-lane Python loop for every node kind; normalisation and de-duplication of `lanes=` and the
creator a circuit takes; replay_levels in the pair-major row order; lane_reduce, packed_equal and
bitonic_sort(masked=True) against all / any / parity, == and sorted() with their rows per group; the planner, the call
arithmetic and circuit_plain_bits with masks under ASan / UBSan (tests/native/circuit_masks_sanitized.cpp); and a masked
plan through the CPU build of the engine, scripted, one-shot and stepped, under ASan / UBSan and both fill bytes
(tests/native/circuit_masks_engine_cpu.cpp)."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import engine_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT = 0x7FFFFFFF, 0x80000000
INVALID = -1
MASKED, ROUTED = "sgfhe_circuit_create_masked", "sgfhe_circuit_create_routed"
UNTOUCHED = 0xDEAD


def _create(L, n_inputs, nodes, outputs, group=1, masks=None, node_mask=None, n_masks=None, null_masks=False, routed=False,
            term_shift=None):
    """nodes: [(kind, table, [ref, ...])], unit weights; masks: [[G entries], ...]; node_mask: index list or None (NULL)
    -> (rc, handle).  routed: through sgfhe_circuit_create_routed."""
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    u32 = lambda x: None if x is None else np.array(list(x) + [0], dtype=np.uint32)
    kind = u32([k for k, _, _ in nodes])
    table = u32([t for _, t, _ in nodes])
    start = np.cumsum([0] + [len(r) for _, _, r in nodes]).astype(np.uint32)
    refs = u32([x for _, _, r in nodes for x in r])
    shifts = np.array(list(term_shift if term_shift is not None else [0] * (len(refs) - 1)) + [0], dtype=np.int32)
    weights = np.ones(len(refs), dtype=np.int32)
    outs = u32(outputs)
    mt = np.array([x for t in (masks or []) for x in t] + [1], dtype=np.uint8)
    nm = u32(node_mask)
    h = ctypes.c_void_p(UNTOUCHED)
    head = (n_inputs, 0, vp(kind), vp(start), vp(refs), vp(shifts), vp(weights), vp(table), len(nodes), vp(outs), None,
            len(outputs), group, 0, None, None, None, 0, None, None, None, None)
    if routed:
        return L.sgfhe_circuit_create_routed(*head, ctypes.byref(h)), h
    count = len(masks or []) if n_masks is None else n_masks
    return L.sgfhe_circuit_create_masked(*head, count, None if null_masks else vp(mt), vp(nm), ctypes.byref(h)), h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def _masks(L, h):
    n, rows = ctypes.c_uint32(UNTOUCHED), ctypes.c_uint64(UNTOUCHED)
    assert L.sgfhe_circuit_masks(h, ctypes.byref(n), ctypes.byref(rows)) == 0
    return n.value, rows.value


# 2 inputs, group 4; node 0 = classic (input 0, input 1): wires 2, 3, 4; node 1 = classic (wire 2, input 0): wires 5, 6, 7
SMALL = [(0, 0, [0, 1]), (0, 0, [2, 0])]
TABLES = [[1, 0, 1, 0], [0, 0, 0, 1]]
# inputs 0 .. 2 fanned (nodes 0, 1, 2), node 3 the LUT leader on them, node 4 its sibling; wires 3 .. 17
FAMILY = [(2, 0xF0, [FALSE, FALSE, 0]), (2, 0xF0, [FALSE, FALSE, 1]), (2, 0xF0, [FALSE, FALSE, 2]),
          (2, 0x96, [5, 7, 9]), (3, 0xE8, [])]


def test_abi_and_declarations(S):
    L = S.lib()
    assert L.sgfhe_abi_version() == 7 == S.ABI_VERSION              # functions are only added
    for name in (MASKED, "sgfhe_circuit_masks"):
        assert name in S.EXPORTED_SYMBOLS and getattr(L, name)
    assert len(getattr(L, MASKED).argtypes) == len(getattr(L, ROUTED).argtypes) + 3
    header = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    assert "#define SGFHE_CIRCUIT_MAX_MASKS 65536u" in header and "int32_t sgfhe_circuit_create_masked(" in header
    from sgfhe_jl_amd import circuit as C
    assert C.MAX_MASKS == 65536


def test_a_masked_plan_its_info_and_its_rows(S):
    L = S.lib()
    rc, h = _create(L, 2, SMALL, [5, 4], group=4, masks=TABLES, node_mask=[1, 2])
    assert rc == 0 and h.value and _masks(L, h) == (2, 2 + 1)
    rc, z = _create(L, 2, SMALL, [5, 4], group=4, routed=True)
    assert rc == 0 and _masks(L, z) == (0, 2 * 4) and _info(L, h) == _info(L, z)       # info does not see masks
    # every other creator: 0 and bootstraps * group
    gates = np.array([[0, 1]], dtype=np.uint32)
    outs = np.array([2], dtype=np.uint32)
    c = ctypes.c_void_p()
    assert L.sgfhe_circuit_create(2, gates.ctypes.data_as(ctypes.c_void_p), 1, outs.ctypes.data_as(ctypes.c_void_p), 1,
                                  ctypes.byref(c)) == 0 and _masks(L, c) == (0, 1)
    n, rows = ctypes.c_uint32(), ctypes.c_uint64()
    assert L.sgfhe_circuit_masks(None, ctypes.byref(n), ctypes.byref(rows)) == INVALID
    assert L.sgfhe_circuit_masks(h, None, ctypes.byref(rows)) == INVALID and L.sgfhe_circuit_masks(h, ctypes.byref(n), None) == INVALID
    for x in (h, z, c):
        L.sgfhe_circuit_destroy(x)


def test_no_masks_is_the_routed_plan(S):
    """n_masks = 0 with NULL arrays and with an all-zero node_mask: the plan the sgfhe_circuit_create_routed entry makes
    (info and rows here; field for field and image word for word in tests/native/circuit_masks_sanitized.cpp)."""
    L = S.lib()
    rc, z = _create(L, 2, SMALL, [5, 4], group=4, routed=True, term_shift=[0, 1, -2, 0])
    assert rc == 0
    for kw in (dict(), dict(node_mask=[0, 0])):
        rc, h = _create(L, 2, SMALL, [5, 4], group=4, term_shift=[0, 1, -2, 0], **kw)
        assert rc == 0 and _info(L, h) == _info(L, z) and _masks(L, h) == _masks(L, z) == (0, 8)
        L.sgfhe_circuit_destroy(h)
    L.sgfhe_circuit_destroy(z)


REFUSALS = [
    ("an entry of 2", SMALL, dict(masks=[[1, 0, 2, 0]], node_mask=[1, 0])),
    ("an entry of 255 in a table nothing uses", SMALL, dict(masks=[[1, 0, 1, 0], [0, 255, 0, 1]])),
    ("a table with no lane set", SMALL, dict(masks=[[1, 0, 1, 0], [0, 0, 0, 0]], node_mask=[1, 0])),
    ("a mask index above n_masks", SMALL, dict(masks=TABLES, node_mask=[0, 3])),
    ("a mask index without any table", SMALL, dict(node_mask=[1, 0])),
    ("n_masks > 0 with NULL masks", SMALL, dict(masks=TABLES, null_masks=True)),
    ("n_masks above the maximum", SMALL, dict(masks=TABLES, n_masks=65537)),
    ("a mask on a sibling", FAMILY, dict(masks=TABLES, node_mask=[0, 0, 0, 0, 1])),
    ("a masked LUT node that leads a live sibling", FAMILY, dict(masks=TABLES, node_mask=[0, 0, 0, 2, 0])),
    ("what sgfhe_circuit_create_routed refuses: a shift outside the group", SMALL,
     dict(masks=TABLES, node_mask=[1, 0], term_shift=[0, 4, 0, 0])),
]


@pytest.mark.parametrize("what,nodes,kw", REFUSALS, ids=[w for w, _, _ in REFUSALS])
def test_validation(S, what, nodes, kw):
    L = S.lib()
    outputs = [5, 4] if nodes is SMALL else [12, 15]                 # (the family: the leader's and the sibling's wire +0)
    n_inputs = 2 if nodes is SMALL else 3
    rc, h = _create(L, n_inputs, nodes, outputs, group=4, **kw)
    assert rc == INVALID and h.value is None, what       # *out is NULL, nothing is left allocated (the native program counts)
    # and the same arrays with the offence taken out are accepted
    rc, h = _create(L, n_inputs, nodes, outputs, group=4, masks=TABLES, node_mask=[1, 0, 2, 0, 0] if nodes is FAMILY else [1, 2])
    assert rc == 0
    L.sgfhe_circuit_destroy(h)


def test_a_masked_leader_of_a_dead_sibling_and_null_out(S):
    L = S.lib()
    rc, h = _create(L, 3, FAMILY, [12], group=4, masks=TABLES, node_mask=[0, 0, 0, 2, 0])     # nothing reads the sibling
    assert rc == 0 and _masks(L, h) == (2, 4 + 4 + 4 + 1)
    L.sgfhe_circuit_destroy(h)
    z = np.zeros(8, dtype=np.uint32)
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert L.sgfhe_circuit_create_masked(1, 0, p, p, p, None, p, p, 0, p, None, 1, 1, 0, None, None, None, 0, None, None,
                                         None, None, 0, None, None, None) == INVALID


# ---- the Python model ------------------------------------------------------------------------------------------------

def _masks_of(G):
    """lane 0 only, the last lane only, all but one, alternating, none (every lane)"""
    return dict(first=[0], last=[G - 1], all_but_one=[t for t in range(G) if t != G // 2], alternating=list(range(0, G, 2)),
                none=None)


@pytest.mark.parametrize("G", [2, 8, 24])
def test_evaluate_plain_against_a_per_lane_loop(S, G):
    """Every mask on a classic node, a gate3, a sum node, a LUT node and a data LUT node, read plain, negated, shifted
    and routed by unmasked nodes and as outputs: against a loop over the instances."""
    rng = np.random.default_rng(200 + G)
    inst = 3 * G
    bits = rng.integers(0, 2, (3, inst)).astype(bool)
    data = rng.integers(0, 256, (1, inst)).astype(np.uint8)
    for name, lanes in _masks_of(G).items():
        c = S.Circuit(3, group=G, planes=1)
        x, y, z = c.inputs
        a, o, xo = c.gate(x, ~y, lanes=lanes)
        maj, _, x3 = c.gate3(x, y, z, lanes=lanes)
        hi, mid, low = c.sum_node([(2, x), (-1, y), (1, z)], lanes=lanes)
        fx, fy = c.fan(x, lanes=lanes), c.fan(y)
        f = c.lut(0x96, fx[2], fy[1], z, lanes=lanes)[0]
        d = c.lut_data(0, fx[2], fy[1], z, lanes=lanes)[0]
        rev = c.reverse(a)
        c.output(a, ~xo, maj, x3, mid, low, f, d, c.gate(~a, o.lane(1))[0], c.gate(rev, ~hi)[1], fx[0])
        on = np.array([lanes is None or (t % G) in lanes for t in range(inst)])
        X, Y, Z = bits
        s = (2 * X.astype(int) - Y + Z) % 4
        A, O, XO = (X & ~Y) & on, (X | ~Y) & on, (X ^ ~Y) & on
        FX = X & on                                              # the masked fan: FALSE on the off lanes
        idx = FX.astype(int) + 2 * Y + 4 * Z
        F, D = ((0x96 >> idx) & 1).astype(bool) & on, ((data[0].astype(int) >> idx) & 1).astype(bool) & on
        HI = (s >= 2) & on

        def shifted(v, d_):
            return np.array([v[t + d_] if 0 <= t % G + d_ < G else False for t in range(inst)])

        REV = np.array([A[t - t % G + G - 1 - t % G] for t in range(inst)])
        want = [A, ~XO, ((X & Y) | (Z & (X | Y))) & on, (X ^ Y ^ Z) & on, ((s == 1) | (s == 2)) & on, (s % 2 == 1) & on, F, D,
                ~A & shifted(O, 1), REV | ~HI, FX]
        got = c.evaluate_plain(bits, data=data)
        assert np.array_equal(got, np.array(want)), (G, name)
        n_lanes = G if lanes is None else len(lanes)
        assert c.rows_per_group() == 6 * n_lanes + 3 * G            # six masked nodes; fan(y) and the two readers are not
        assert ("rows_per_group" in c.info()) == (lanes is not None)
        assert _masks(c._L, c.handle())[0] == len(c.mask_tables) == (0 if lanes is None else 1)   # de-duplicated


def test_lanes_normalisation_and_the_creator_a_circuit_takes(S, monkeypatch):
    L = S.lib()
    calls = []
    real = L.sgfhe_circuit_create_masked
    monkeypatch.setattr(L, "sgfhe_circuit_create_masked", lambda *a: calls.append(a) or real(*a), raising=False)
    c = S.Circuit(2, group=4)
    x, y = c.inputs
    a = c.gate(x, y, lanes=range(4))[0]                               # every lane: no mask
    b = c.gate(a, y, lanes=[1, 1, 1, 1])[0]                           # ... as flags
    c.output(c.gate3(a, b, x, lanes=(3, 2, 1, 0))[0])
    c.handle()
    assert not calls and not c.gate_masks and not c.mask_tables and "rows_per_group" not in c.info()
    assert c.rows_per_group() == 12 and c.lanes_on(0) == [0, 1, 2, 3]
    c = S.Circuit(2, group=4, registers=1)
    x, y = c.inputs
    a = c.gate(x, y, lanes=[0, 2])[0]
    b = c.xor(a, y, lanes=[1, 0, 1, 0])                               # the same mask as flags
    r = c.refresh(b, lanes={3})
    s_, carry = c.full_adder(a, b, r, lanes=[2, 0, 2])                # an index twice is the index
    c.output(s_, c.fan(r, lanes=[0, 1, 2])[0])
    c.next_state(carry)
    c.handle()
    assert len(calls) == 1 and c.mask_tables == [(1, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 0)]
    assert c.gate_masks == {0: (1, 0, 1, 0), 1: (1, 0, 1, 0), 2: (0, 0, 0, 1), 3: (1, 0, 1, 0), 4: (1, 1, 1, 0)}
    args = calls[0]
    assert args[12] == 4 and args[13] == 1 and args[17] == 0 and args[22] == 3
    assert c.info()["rows_per_group"] == c.rows_per_group() == 2 + 2 + 1 + 2 + 3 and c.lanes_on(2) == [3]
    assert c.step_plan().gate_masks == c.gate_masks
    with pytest.raises(ValueError):
        c.gate(x, y, lanes=[])                                        # no lane at all
    with pytest.raises(ValueError):
        c.gate(x, y, lanes=[0, 0, 0, 0])
    with pytest.raises(ValueError):
        c.gate(x, y, lanes=[4])                                       # no lane of the group
    with pytest.raises(ValueError):
        c.gate(x, y, lanes=[-1])
    with pytest.raises(ValueError):
        S.Circuit(2).gate(*S.Circuit(2).inputs, lanes=[0])            # group 1 takes no mask
    n = len(c.gates)
    with pytest.raises(ValueError):
        c.sum_node([(3, x)], lanes=[0])                               # a refused node leaves nothing behind
    assert len(c.gates) == n and set(c.gate_masks) == {0, 1, 2, 3, 4}
    # a masked leader of a live sibling is the planner's to refuse
    d = S.Circuit(1, group=4)
    f = d.fan(d.inputs[0])
    fam = d.lut_multi([0x96, 0xE8], f[2], f[1], f[0])
    d.gate_masks[1] = (1, 0, 0, 0)
    d.output(fam[1][0])
    with pytest.raises(S.SgfheError):
        d.handle()


def test_replay_levels_runs_the_pairs_in_order(S):
    """replay_levels with a 'bootstrap' that returns its inputs: the rows of a masked level arrive pair-major (node, lane,
    group), a call boundary cuts them where the plan cuts them, and off lanes read as the trivial LWE -- TRUE when
    negated, at the codeword Dr."""
    from sgfhe_jl_amd import circuit as C
    r, n, G, inst = 1 << 10, 3, 4, 8
    rng = np.random.default_rng(5)
    inputs = rng.integers(0, r, (2, inst, n + 1)).astype(np.uint64)
    c = S.Circuit(2, group=G)
    x, y = c.inputs
    a = c.gate(x, y, lanes=[1, 3])
    b = c.gate(y, x)
    low = c.sum_node([(1, x), (1, y)], lanes=[2])[2]
    c.output(a[0], ~a[1], b[2], low, ~low.lane(1))
    seen = []

    def boot(call, a1, b1, a2, b2):
        x_ = np.concatenate([a1, b1[:, None]], axis=1)
        y_ = np.concatenate([a2, b2[:, None]], axis=1)
        seen.append((call, x_.copy(), y_.copy()))
        return np.stack([x_, y_, (x_ + y_) & np.uint64(r - 1)], axis=1)

    out = C.replay_levels(c, inputs, r, boot)
    order = [(0, t) for lane in (1, 3) for t in (lane, 4 + lane)] + [(1, t) for lane in range(4) for t in (lane, 4 + lane)] + \
        [(2, 2), (2, 6)]
    rk, ri = C.level_row_map(c, [0, 1, 2], inst)
    assert list(zip(rk.tolist(), ri.tolist())) == order and len(seen) == 1 and seen[0][0] == 0
    X = np.stack([inputs[(0, 1, 0)[k]][t] if k < 2 else (inputs[0][t] + inputs[1][t]) & np.uint64(r - 1) for k, t in order])
    assert np.array_equal(seen[0][1], X)
    on = np.zeros((inst, 1), dtype=bool)
    on[[1, 3, 5, 7]] = True
    true = np.array([0] * n + [r // 4], dtype=np.uint64)
    assert np.array_equal(out[0], inputs[0] * on) and np.array_equal(out[1], np.where(on, C.lwe_not(inputs[1], r), true))
    assert np.array_equal(out[2], (inputs[0] + inputs[1]) & np.uint64(r - 1))
    # LOW = U - 2 HI with HI = the row's first input = U: -U on lane 2, FALSE elsewhere; shifted, lane 1 reads lane 2
    U = (inputs[0] + inputs[1]) & np.uint64(r - 1)
    LOW = np.zeros_like(U)
    LOW[[2, 6]] = (np.uint64(r) - U[[2, 6]]) & np.uint64(r - 1)
    assert np.array_equal(out[3], LOW)
    want4 = np.tile(true, (inst, 1))
    want4[[1, 5]] = C.lwe_not(LOW[[2, 6]], r)
    assert np.array_equal(out[4], want4)
    # an unmasked circuit keeps rank * instances + instance
    d = S.Circuit(2, group=G)
    d.output(d.gate(*d.inputs)[0])
    rk, ri = C.level_row_map(d, [0, 5], 3)
    assert rk.tolist() == [0, 0, 0, 1, 1, 1] and ri.tolist() == [0, 1, 2, 0, 1, 2]


def test_lane_reduce_packed_equal_and_their_rows(S):
    from sgfhe_jl_amd.circuit import lane_reduce
    rng = np.random.default_rng(8)
    for G in (2, 8, 16):
        groups = 40
        v = rng.integers(0, 2, (1, groups * G)).astype(bool)
        v[0, :G] = True
        v[0, G:2 * G] = False
        words = v[0].reshape(groups, G)
        for which, fold in ((0, [all(w) for w in words]), (1, [any(w) for w in words]), (2, [sum(w) % 2 == 1 for w in words])):
            c = S.Circuit(1, group=G)
            c.output(lane_reduce(c, c.inputs[0], which, G))
            out = c.evaluate_plain(v)[0].reshape(groups, G)
            assert out[:, 0].tolist() == fold and not out[:, 1:].any(), (G, which)      # the result at lane 0, FALSE elsewhere
            assert c.info()["rows_per_group"] == G - 1 and c.info()["levels"] == G.bit_length() - 1
    c = S.Circuit(1, group=8)
    c.output(lane_reduce(c, c.inputs[0], 0))
    assert c.info()["rows_per_group"] == 7
    for bad in (dict(G=4), dict(which=3)):
        with pytest.raises(ValueError):
            lane_reduce(c, c.inputs[0], bad.get("which", 0), bad.get("G"))
    with pytest.raises(ValueError):
        lane_reduce(S.Circuit(1, group=6), S.Wire(0), 0)
    for width in (2, 8, 16):
        c = S.packed_equal(width)
        groups = 50
        xy = rng.integers(0, 2, (2, groups * width)).astype(bool)
        xy[1, :20 * width] = xy[0, :20 * width]                       # equal words
        xy[1, 18 * width] ^= True                                    # ... and words that differ in one bit: the first,
        xy[1, 20 * width - 1] ^= True                                 # the last
        out = c.evaluate_plain(xy)[0].reshape(groups, width)
        want = [list(a) == list(b) for a, b in zip(xy[0].reshape(groups, width), xy[1].reshape(groups, width))]
        assert out[:, 0].tolist() == want and sum(want) >= 18 and not out[:, 1:].any()
        assert c.info()["rows_per_group"] == 2 * width - 1 and c.info()["nodes"] == 1 + width.bit_length() - 1


def test_masked_bitonic_sort_against_sorted(S):
    width, G = 3, 8
    c, m = S.bitonic_sort(width, G), S.bitonic_sort(width, G, masked=True)
    assert "rows_per_group" not in c.info() and c.rows_per_group() == 336 and m.info()["rows_per_group"] == 264
    assert {k: v for k, v in m.info().items() if k != "rows_per_group"} == c.info()      # info does not see masks
    assert all(sum(t) == G // 2 for t in m.mask_tables) and len(m.gate_masks) == 6 * width
    assert S.bitonic_sort(4, 8, masked=True).rows_per_group() == 8 * (8 + 6 * 4) + 6 * 4 * 4
    rng = np.random.default_rng(9)
    groups = 40
    vals = rng.integers(0, 1 << width, groups * G)
    vals[:G] = 5
    vals[G:2 * G] = np.arange(G)[::-1] % (1 << width)
    vals[2 * G:3 * G] = np.arange(G) % 2
    bits = np.array([(vals >> i) & 1 for i in range(width)], dtype=bool)
    out = m.evaluate_plain(bits)
    got = sum(out[i].astype(int) << i for i in range(width))
    assert got.tolist() == [v for g in range(groups) for v in sorted(vals[g * G:(g + 1) * G].tolist())]
    assert np.array_equal(out, c.evaluate_plain(bits))


# ---- the native programs ---------------------------------------------------------------------------------------------

def test_masks_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_masks_sanitized.cpp: random masked circuits of every node kind against the plan without masks
    and against a scalar evaluation, the call arithmetic restated row by row (a call boundary inside a node's pairs and
    between two nodes), n_masks = 0 against the routed plan image for image, and the refused inputs.  A stand-alone
    program run as a child process, the sanitizers' runtimes linked into it; the same program without sanitizers counts
    the allocations of the refusals and compares as much."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_masks_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_masks_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                        "-I", inc, src, "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("sanitize" in b.stderr or "libasan" in b.stderr or "libubsan" in b.stderr) and \
            "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    tag, compared = r.stdout.split()
    assert tag == "ok" and int(compared) > 100000
    exe2 = str(tmp_path / "circuit_masks_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-DCOUNT_ALLOCATIONS", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe2],
                   check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout


def test_masked_runs_through_the_cpu_engine_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_masks_engine_cpu.cpp linked to csrc/engine.hip compiled against tests/native/hipcpu with the
    flags of tests/engine_cpu.py: masked plans through sgfhe_debug_circuit_script on a keyless ctx, one-shot and stepped,
    every call's staged rows and descriptors and the final wire table against integers computed in the program -- under
    both fill bytes of the stand-in's device memory, which is what a missing fill would hand back.  The stand-in's
    launch log says the row decode and the fill kernel ran."""
    if not (os.path.exists(engine_cpu.CLANG) or shutil.which(engine_cpu.CLANG)):
        pytest.skip("no ROCm clang++ (%s)" % engine_cpu.CLANG)
    exe = str(tmp_path / "circuit_masks_engine_cpu")
    cmd = engine_cpu.build_command(exe, engine_cpu.SAN_FLAGS)
    driver = os.path.join(ROOT, "tests", "native", "engine_cpu_driver.cpp")
    assert cmd.count(driver) == 1
    cmd[cmd.index(driver)] = os.path.join(ROOT, "tests", "native", "circuit_masks_engine_cpu.cpp")
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=engine_cpu.BUILD_TIMEOUT)
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "no such file" in b.stderr.lower()):
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-4000:]
    outs = []
    for fill in engine_cpu.FILLS:
        log = str(tmp_path / ("launches" + fill))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=engine_cpu.RUN_TIMEOUT,
                           env=engine_cpu.run_env(fill, log))
        assert r.returncode == 0, (fill, (r.stdout + r.stderr)[-4000:])
        outs.append(r.stdout)
        launches = {}
        with open(log) as fh:
            for line in fh:
                k, n, oob = line.split()
                launches[k] = int(n)
                assert int(oob) == 0, line
        assert launches["k_circ_mask_fill"] >= 10 and launches["k_circ_gather"] == launches["k_circ_scatter"] >= 12
        assert launches["k_circ_xor3"] >= 2 and launches["k_circ_next"] == 3
    tag, compared = outs[0].split()
    assert tag == "ok" and int(compared) > 1000000 and outs[1] == outs[0]
