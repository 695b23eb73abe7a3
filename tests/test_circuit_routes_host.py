"""Lane routes without a GPU (sgfhe_circuit_create_routed, include/sgfhe_hip.h): the new symbols
and the ABI revision; every refusal of the create entry through ctypes, with *out untouched; a plan with n_routes = 0
against the sgfhe_circuit_create_seq plan (its info here, its image word for word in the native program);
sgfhe_circuit_routes; evaluate_plain against a per-lane Python loop at G = 1, 2, 8 and 24 with identity, reversal, swap,
rotation, broadcast and all-fill tables and negated references; composition and normalisation of Wire.route and
Wire.lane, and the creator a circuit takes; replay_levels with a route; bitonic_sort against sorted(); and the planner
and circuit_plain_bits with routes under ASan / UBSan (tests/native/circuit_routes_sanitized.cpp)."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT = 0x7FFFFFFF, 0x80000000
INVALID = -1
ROUTED, SEQ = "sgfhe_circuit_create_routed", "sgfhe_circuit_create_seq"
UNTOUCHED = 0xDEAD


def _create(L, n_inputs, nodes, outputs, group=1, routes=None, term_route=None, out_route=None, next_route=None,
            regs=None, term_shift=None, out_shift=None, n_routes=None, seq=False, null_routes=False):
    """nodes: [(kind, table, [ref, ...])], unit weights; routes: [[G entries], ...]; term_route / out_route / next_route:
    index lists or None (NULL); regs: (next_ref, next_shift) -> (rc, handle).  seq: through sgfhe_circuit_create_seq."""
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    u32 = lambda x: None if x is None else np.array(list(x) + [0], dtype=np.uint32)
    i32 = lambda x: None if x is None else np.array(list(x) + [0], dtype=np.int32)
    kind = u32([k for k, _, _ in nodes])
    table = u32([t for _, t, _ in nodes])
    start = np.cumsum([0] + [len(r) for _, _, r in nodes]).astype(np.uint32)
    refs = u32([x for _, _, r in nodes for x in r])
    n_terms = len(refs) - 1
    shifts = i32(term_shift if term_shift is not None else [0] * n_terms)
    weights = np.ones(len(refs), dtype=np.int32)
    outs = u32(outputs)
    oshift = i32(out_shift if out_shift is not None else [0] * len(outputs))
    nref, nshift = regs if regs is not None else ([], [])
    keep = [u32(nref), i32(nshift), u32(term_route), u32(out_route), u32(next_route),
            i32([x for t in (routes or []) for x in t])]
    h = ctypes.c_void_p(UNTOUCHED)
    head = (n_inputs, 0, vp(kind), vp(start), vp(refs), vp(shifts), vp(weights), vp(table), len(nodes), vp(outs),
            vp(oshift), len(outputs), group, len(nref), vp(keep[0]), vp(keep[1]), None)
    if seq:
        return L.sgfhe_circuit_create_seq(*head, ctypes.byref(h)), h
    count = len(routes or []) if n_routes is None else n_routes
    return L.sgfhe_circuit_create_routed(*head, count, None if null_routes else vp(keep[5]), vp(keep[2]), vp(keep[3]),
                                         vp(keep[4]), ctypes.byref(h)), h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def _routes(L, h):
    r = ctypes.c_uint32(UNTOUCHED)
    assert L.sgfhe_circuit_routes(h, ctypes.byref(r)) == 0
    return r.value


# 2 inputs, group 4; node 0 = classic (input 0, input 1): wires 2, 3, 4; node 1 = classic (wire 2, input 0): wires 5, 6, 7
SMALL = [(0, 0, [0, 1]), (0, 0, [2, 0])]
TABLES = [[3, 2, 1, 0], [-1, 0, 0, 2]]


def test_abi_and_declarations(S):
    L = S.lib()
    assert L.sgfhe_abi_version() == 7 == S.ABI_VERSION              # functions are only added
    for name in (ROUTED, "sgfhe_circuit_routes"):
        assert name in S.EXPORTED_SYMBOLS and getattr(L, name)
    assert len(getattr(L, ROUTED).argtypes) == len(getattr(L, SEQ).argtypes) + 5
    header = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    assert "#define SGFHE_CIRCUIT_MAX_ROUTES 65536u" in header and "#define SGFHE_CIRCUIT_ROUTE_FALSE (-1)" in header
    from sgfhe_jl_amd import circuit as C
    assert C.MAX_ROUTES == 65536 and C.ROUTE_FALSE == -1


def test_a_routed_plan_its_info_and_its_routes(S):
    L = S.lib()
    rc, h = _create(L, 2, SMALL, [5, 4], group=4, routes=TABLES, term_route=[1, 0, 2, 0], out_route=[0, 1])
    assert rc == 0 and h.value and _routes(L, h) == 2
    rc, z = _create(L, 2, SMALL, [5, 4], group=4, seq=True)
    assert rc == 0 and _routes(L, z) == 0 and _info(L, h) == _info(L, z)       # info does not see routes
    g = ctypes.c_uint32()
    assert L.sgfhe_circuit_group(h, ctypes.byref(g)) == 0 and g.value == 4
    # every other creator: 0
    gates = np.array([[0, 1]], dtype=np.uint32)
    outs = np.array([2], dtype=np.uint32)
    c = ctypes.c_void_p()
    assert L.sgfhe_circuit_create(2, gates.ctypes.data_as(ctypes.c_void_p), 1, outs.ctypes.data_as(ctypes.c_void_p), 1,
                                  ctypes.byref(c)) == 0 and _routes(L, c) == 0
    assert L.sgfhe_circuit_routes(None, ctypes.byref(g)) == INVALID and L.sgfhe_circuit_routes(h, None) == INVALID
    for x in (h, z, c):
        L.sgfhe_circuit_destroy(x)


def test_no_routes_is_the_seq_plan(S):
    """n_routes = 0 with NULL arrays, with all-zero arrays, and tables nothing uses: the plan the sgfhe_circuit_create_seq
    entry makes (info here; field for field and image word for word in tests/native/circuit_routes_sanitized.cpp)."""
    L = S.lib()
    regs = ([5 | NOT], [1])
    rc, z = _create(L, 2, SMALL, [5, 4], group=4, regs=regs, out_shift=[-1, 2], seq=True)
    assert rc == 0
    for kw in (dict(), dict(term_route=[0] * 4, out_route=[0, 0], next_route=[0]), dict(routes=TABLES)):
        rc, h = _create(L, 2, SMALL, [5, 4], group=4, regs=regs, out_shift=[-1, 2], **kw)
        assert rc == 0 and _info(L, h) == _info(L, z) and _routes(L, h) == len(kw.get("routes", []))
        L.sgfhe_circuit_destroy(h)
    L.sgfhe_circuit_destroy(z)


REFUSALS = [
    ("an entry at G", dict(routes=[[3, 2, 4, 0]], term_route=[1, 0, 0, 0])),
    ("an entry below the fill", dict(routes=[[3, -2, 1, 0]], term_route=[1, 0, 0, 0])),
    ("an entry outside [-1, G) in a table nothing uses", dict(routes=[[0, 1, 2, 3], [0, 0, 0, 7]])),
    ("a term's route index above n_routes", dict(routes=TABLES, term_route=[3, 0, 0, 0])),
    ("an output's route index above n_routes", dict(routes=TABLES, out_route=[0, 3])),
    ("a next state's route index above n_routes", dict(routes=TABLES, regs=([5], [0]), next_route=[3])),
    ("a route index without any table", dict(term_route=[0, 0, 1, 0])),
    ("a term's route beside a shift", dict(routes=TABLES, term_route=[1, 0, 0, 0], term_shift=[1, 0, 0, 0])),
    ("an output's route beside a shift", dict(routes=TABLES, out_route=[0, 2], out_shift=[0, -3])),
    ("a next state's route beside a shift", dict(routes=TABLES, regs=([5], [2]), next_route=[1])),
    ("n_routes > 0 with NULL routes", dict(routes=TABLES, null_routes=True)),
    ("n_routes above the maximum", dict(routes=TABLES, n_routes=65537)),
    ("what sgfhe_circuit_create_seq refuses: a shift outside the group", dict(routes=TABLES, term_shift=[0, 4, 0, 0])),
]


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_validation(S, what, kw):
    L = S.lib()
    rc, h = _create(L, 2, SMALL, [5, 4], group=4, **kw)
    assert rc == INVALID and h.value is None, what       # *out is NULL, nothing was allocated (the native program counts)
    # and the same arrays with the offence taken out are accepted
    rc, h = _create(L, 2, SMALL, [5, 4], group=4, routes=TABLES, term_route=[1, 0, 2, 0], out_route=[2, 1])
    assert rc == 0
    L.sgfhe_circuit_destroy(h)


def test_null_out(S):
    L = S.lib()
    z = np.zeros(8, dtype=np.uint32)
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert L.sgfhe_circuit_create_routed(1, 0, p, p, p, None, p, p, 0, p, None, 1, 1, 0, None, None, None, 0, None, None,
                                         None, None, None) == INVALID


# ---- the Python model ------------------------------------------------------------------------------------------------

def _tables(G, rng):
    """identity, reversal, swap, rotation, broadcast, all fill, and a random table with fills"""
    ident = list(range(G))
    return dict(identity=ident, reversal=ident[::-1], swap=[t ^ 1 if (t ^ 1) < G else -1 for t in ident],
                rotation=[(t + 3) % G for t in ident], broadcast=[G - 1] * G, fill=[-1] * G,
                random=[int(x) for x in rng.integers(-1, G, G)])


def _loop(bits, table, G, negate):
    """The reference (w, NOT, route) one lane at a time: instance t of lane l reads instance t - l + table[l]."""
    out = np.zeros(len(bits), dtype=bool)
    for t in range(len(bits)):
        lane = t % G
        v = bool(bits[t - lane + table[lane]]) if table[lane] >= 0 else False
        out[t] = (not v) if negate else v
    return out


@pytest.mark.parametrize("G", [1, 2, 8, 24])
def test_evaluate_plain_against_a_per_lane_loop(S, G):
    """Every table as a term of a classic node, of a gate3, of a sum node and of a LUT node, as an output and negated:
    against the loop.  The circuit takes the routed creator exactly when a route survives normalisation."""
    rng = np.random.default_rng(100 + G)
    inst = 3 * G
    bits = rng.integers(0, 2, (3, inst)).astype(bool)
    for name, table in _tables(G, rng).items():
        c = S.Circuit(3, group=G)
        x, y, z = c.inputs
        xr, yr = x.route(table), (~y).route(table)
        a, o, xo = c.gate(xr, yr)
        maj, _, x3 = c.gate3(xr, z, yr)
        hi, mid, low = c.sum_node([(2, xr), (-1, yr), (1, z)])
        f = c.lut(0x96, c.fan(xr)[2], c.fan(yr)[1], z.route(table))[0]
        c.output(a, xo, maj, x3, mid, low, f, xr, ~(x.route(table)), a.route(table), (~hi).route(table))
        X, Y, Z = _loop(bits[0], table, G, False), _loop(bits[1], table, G, True), _loop(bits[2], table, G, False)
        s = (2 * X.astype(int) - Y + bits[2]) % 4
        A, HI = X & Y, s >= 2
        want = [A, X ^ Y, (X & bits[2]) | (Y & (X | bits[2])), X ^ Y ^ bits[2], (s == 1) | (s == 2), s % 2 == 1,
                X ^ Y ^ Z, X, ~X, _loop(A, table, G, False), _loop(HI, table, G, True)]
        got = c.evaluate_plain(bits)
        assert np.array_equal(got, np.array(want)), (G, name)
        assert bool(c.route_tables) == (S.Wire(0).route(table).table is not None), (G, name)
        assert c.info()["nodes"] == 6
        n = ctypes.c_uint32()
        assert c._L.sgfhe_circuit_routes(c.handle(), ctypes.byref(n)) == 0 and n.value == len(c.route_tables)
        assert len(c.route_tables) <= 1                       # de-duplicated: one table however many references


def test_route_composition_and_normalisation(S):
    from sgfhe_jl_amd.circuit import shift_table, normal_route
    w = S.Wire(5)
    G = 6
    ident = list(range(G))
    assert w.route(ident) == w and w.route(ident).table is None and (~w).route(ident) == ~w
    for d in range(-G + 1, G):                                   # a pure shift with FALSE fill is the shift
        assert w.route(shift_table(d, G)) == w.lane(d) and w.route(shift_table(d, G)).table is None
        assert normal_route(shift_table(d, G)) == (d, None)
    rev = ident[::-1]
    assert w.route(rev).table == tuple(rev) and w.route(rev).shift == 0
    assert w.route(rev).route(rev) == w                          # an involution composes to nothing
    A, B = [3, 3, -1, 0, 5, 1], [2, 0, 5, -1, 4, 4]
    assert w.route(A).route(B).table == tuple(-1 if b < 0 else A[b] for b in B) == (-1, 3, 1, -1, 5, 5)   # w at A[B[t]]
    assert (~w).route(A).negated and (~w).route(A) == ~(w.route(A)) and w.route(A).id == 5
    # a shift first, a shift afterwards: fills propagate
    assert w.lane(2).route(rev).table == tuple(-1 if not 0 <= t + 2 < G else t + 2 for t in rev)
    assert w.route(rev).lane(2).table == tuple(rev[t + 2] if t + 2 < G else -1 for t in ident)
    assert w.route(rev).lane(0) == w.route(rev)
    # rotations compose to a rotation, and back to nothing
    c = S.Circuit(1, group=G)
    assert c.rot(c.rot(w, 2), 3) == c.rot(w, 5) and c.rot(c.rot(w, 2), 4) == w
    assert c.swap(w, 3).table == (3, 2, 1, 0, -1, -1)               # 4 ^ 3 = 7 and 5 ^ 3 = 6 are no lanes of the group
    assert c.swap(c.swap(w, 3), 3).table == (0, 1, 2, 3, -1, -1)    # ... and a fill stays a fill
    assert c.bcast(w, 4).table == (4,) * G and c.bcast(w, 4).route(rev) == c.bcast(w, 4)
    assert c.reverse(w).table == tuple(rev)
    assert c.rot(w, 0) == w and S.Circuit(1, group=1).rot(w, 5) == w and S.Circuit(1, group=1).reverse(w) == w
    assert w.route([-1]).table == (-1,)                          # G = 1: all fill is a route
    with pytest.raises(ValueError):
        w.route([0, 1, 6, 3, 4, 5])
    with pytest.raises(ValueError):
        w.route([0, -2, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        w.route(rev).route([0, 1])                               # another group size
    with pytest.raises(ValueError):
        c.gate(w.route([1, 0]), w)                               # a table that is not the circuit's group
    with pytest.raises(ValueError):
        c.bcast(w, G)
    assert w.route(rev) != w.route(A) and len({w.route(rev), w.route(list(rev)), w}) == 2
    assert "route" in repr(w.route(rev))


def test_the_creator_a_circuit_takes(S, monkeypatch):
    """sgfhe_circuit_create_routed only when a route survives normalisation; the arrays it is given."""
    L = S.lib()
    calls = []
    real = L.sgfhe_circuit_create_routed
    monkeypatch.setattr(L, "sgfhe_circuit_create_routed", lambda *a: calls.append(a) or real(*a), raising=False)
    c = S.Circuit(2, group=4)
    x, y = c.inputs
    c.output(c.gate(x.route([1, 2, 3, -1]), c.rot(y, 4))[0].route([0, 1, 2, 3]))
    c.handle()
    assert not calls and not c.route_tables and c.gate_shifts == [(1, 0)] and c.output_shifts == [0]
    c = S.Circuit(2, group=4, registers=1)
    x, y = c.inputs
    a = c.gate(c.rot(x, 1), c.reverse(y))[0]
    c.output(c.rot(a, 1), a.lane(-1), ~c.reverse(a))
    c.next_state(c.rot(x, 1))
    c.handle()
    assert len(calls) == 1 and c.route_tables == [(1, 2, 3, 0), (3, 2, 1, 0)]
    args = calls[0]
    assert args[12] == 4 and args[13] == 1 and args[17] == 2
    n = ctypes.c_uint32()
    assert L.sgfhe_circuit_routes(c.handle(), ctypes.byref(n)) == 0 and n.value == 2
    assert c.step_plan().output_shifts == [(1, 2, 3, 0), -1, (3, 2, 1, 0), (1, 2, 3, 0)]
    # one step in clear: the register is rotated, the outputs are taken before
    bits = np.array([[1, 0, 0, 1, 0, 1, 1, 1], [1, 1, 0, 0, 1, 0, 1, 0]], dtype=bool)
    outs, state = c.evaluate_plain_steps(bits[:1], bits[None, 1:])
    rot = lambda v: np.concatenate([np.roll(v[:4], -1), np.roll(v[4:], -1)])
    rev = lambda v: np.concatenate([v[:4][::-1], v[4:][::-1]])
    A = rot(bits[0]) & rev(bits[1])
    assert np.array_equal(state[0], rot(bits[0])) and np.array_equal(outs[0, 0], rot(A)) and np.array_equal(outs[0, 2], ~rev(A))


def test_replay_levels_applies_routes(S):
    """replay_levels with an identity-on-XOR 'bootstrap': a routed term, a routed negated output at the codeword Dr, and
    a routed next state against numpy; fills are the trivial LWE, TRUE when negated."""
    from sgfhe_jl_amd import circuit as C
    r, n, G, inst = 1 << 10, 4, 4, 8
    rng = np.random.default_rng(3)
    inputs = rng.integers(0, r, (2, inst, n + 1)).astype(np.uint64)
    table = (2, -1, 0, 0)
    c = S.Circuit(2, group=G, registers=1)
    x, y = c.inputs
    g = c.gate(x.route(table), y)
    c.output((~g[2]).route(table), x.route(table))
    c.next_state((~y).route(table))

    def boot(call, a1, b1, a2, b2):            # "AND" = first input, "OR" = second, "XOR" = their sum: enough to see the routing
        x_ = np.concatenate([a1, b1[:, None]], axis=1)
        y_ = np.concatenate([a2, b2[:, None]], axis=1)
        return np.stack([x_, y_, (x_ + y_) & np.uint64(r - 1)], axis=1)

    def routed(v):
        out = np.zeros_like(v)
        for t in range(inst):
            if table[t % G] >= 0:
                out[t] = v[t - t % G + table[t % G]]
        return out

    out, nxt, calls = C.replay_levels(c, inputs, r, boot, _next=True)
    xor = (routed(inputs[0]) + inputs[1]) & np.uint64(r - 1)
    assert calls == 1 and np.array_equal(out[1], routed(inputs[0]))
    assert np.array_equal(out[0], C.lwe_not(routed(xor), r)) and np.array_equal(nxt[0], C.lwe_not(routed(inputs[1]), r))
    assert np.array_equal(out[0][1], [0] * n + [r // 4])         # a fill under NOT: the trivial TRUE


@pytest.mark.parametrize("width,G", [(3, 8), (4, 4)])
def test_bitonic_sort_against_sorted(S, width, G):
    from sgfhe_jl_amd.circuit import bitonic_stages
    c = S.bitonic_sort(width, G)
    k = G.bit_length() - 1
    stages = k * (k + 1) // 2
    assert len(bitonic_stages(G)) == stages
    assert c.info()["nodes"] == 2 * width + 2 * width * stages and c.info()["levels"] == 2 + (width + 1) * stages
    bare = S.bitonic_sort(width, G, refresh_inputs=False).info()
    assert bare["nodes"] == width + 2 * width * stages and bare["levels"] == 1 + (width + 1) * stages
    assert c.n_inputs == c.n_outputs == width and c.group == G and not c.planes and not c.n_regs
    assert all(set(t) <= set(range(G)) for t in c.route_tables)          # permutations and decisions only: no fill
    rng = np.random.default_rng(width * 100 + G)
    groups = 40
    vals = rng.integers(0, 1 << width, groups * G)
    vals[:G] = 5                                                        # all equal
    vals[G:2 * G] = np.arange(G)[::-1] % (1 << width)                   # descending
    vals[2 * G:3 * G] = np.arange(G) % 2                                # many ties
    bits = np.array([(vals >> i) & 1 for i in range(width)], dtype=bool)
    out = c.evaluate_plain(bits)
    got = sum(out[i].astype(int) << i for i in range(width))
    want = [v for g in range(groups) for v in sorted(vals[g * G:(g + 1) * G].tolist())]
    assert got.tolist() == want


def test_bitonic_sort_arguments(S):
    with pytest.raises(ValueError):
        S.bitonic_sort(3, 6)
    with pytest.raises(ValueError):
        S.bitonic_sort(0, 4)
    one = S.bitonic_sort(2, 1)                                          # one element: the refreshes and fans alone
    assert one.info()["nodes"] == 4 and not one.route_tables


def test_routes_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_routes_sanitized.cpp: random routed circuits of every node kind against the plan without
    routes and against a scalar evaluation, n_routes = 0 against the sequential plan image for image, and the refused
    inputs.  A stand-alone program run as a child process, the sanitizers' runtimes linked into it; the same program
    without sanitizers counts the allocations of the refusals and compares as much."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_routes_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_routes_sanitized")
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
    exe2 = str(tmp_path / "circuit_routes_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-DCOUNT_ALLOCATIONS", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe2],
                   check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
