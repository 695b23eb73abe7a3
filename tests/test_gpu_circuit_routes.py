"""Lane routes on the device (sgfhe_circuit_create_routed).  A route is a public per-lane table in
place of a lane shift, so: tables that spell the shifts {0, +-1, +-7}, given raw through the C entry, against the
sgfhe_circuit_create_lanes plan, byte for byte in both flatten modes; a random circuit of classic, sum, LUT and data nodes
with random tables (fills, NOT at every LUT position) against circuit.replay_levels on the two oracles; a call boundary
inside a group of 48 with a swap and a rotation across it; a rotate-by-one register with no bootstrap at all; the
ciphertext form under all three flag sets, where a routed output is refreshed or lifted and never direct; the probe's
records; the argument errors; bitonic_sort(3, 8); one routed plan at Params(1024).  Every comparison of ciphertext words
is for equality."""

import ctypes
import os
import sys

import numpy as np
import pytest

import lut_ref as LR
import noise_ref as NR
import pack_lift_ref as PL

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(5, 37))
SENTINEL = 0xA5A5A5A5A5A5A5A5
INVALID = -1
DIRECT, LIFT = 1, 2


def _setup64(S, oc, seed, engines=1):
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    lo = LR.low_oracle(oc, params)
    sk = o.private_key(seed)
    bkey = o.bootstrap_key(sk, seed + 1)
    engs = []
    for _ in range(engines):
        e = S.Engine(params)
        e.upload_key(bkey)
        engs.append(e)
    return params, o, lo, sk, bkey, engs


def _inputs(params, sk, bits, seed):
    """bits [n_inputs][instances] -> LWEs with |e| <= Dr/16, made from the secret key."""
    rng = np.random.default_rng(seed)
    flat = np.asarray(bits).reshape(-1)
    e = rng.integers(-(params.r // 64), params.r // 64 + 1, size=flat.size)
    return NR.handmade_zr(params, sk, rng, e, flat).reshape(np.asarray(bits).shape + (params.n + 1,))


def _decrypt0(params, sk, lwe):
    return LR.decrypt_scaled(params, sk, lwe, 0).reshape(lwe.shape[:-1]).astype(bool)


def _decrypt_ct(S, params, sk, w, v):
    return np.stack([np.concatenate([S.host.decrypt_rlwe(params, sk, w[o, t], v[o, t]) for t in range(w.shape[1])])
                     for o in range(w.shape[0])])


def _set_mode(engines, key):
    for e in engines:
        e.set_random_flatten(key is not None, key or 0)      # (the call counter starts again at 0)


def _second_ctx(ref):
    return (lambda call, *lwe: ref.bootstrap_batch(*lwe), lambda call, a, b, t, idx: ref.bootstrap_lut_batch(a, b, t))


def _shift_table(d, G):
    return [t + d if 0 <= t + d < G else -1 for t in range(G)]


# ---- shift equivalence --------------------------------------------------------------------------------------------

def test_tables_that_spell_shifts_give_the_bytes_of_the_lanes_plan(S, oc):
    """G = 8, 24 instances, 10 classic nodes whose every reference is shifted by one of {0, +-1, +-7}, shifted and negated
    outputs: the sgfhe_circuit_create_lanes plan against the sgfhe_circuit_create_routed plan of the same arrays with
    every shift 0 and the table of that shift in its place -- the identity table for shift 0 --, given raw so that nothing
    normalises them away.  The same bytes in both flatten modes; no oracle is needed."""
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 301)
    L = S.lib()
    G, inst, shifts = 8, 24, [0, 1, -1, 7, -7]
    rng = np.random.default_rng(302)
    c = S.Circuit(4, group=G)
    wires = list(c.inputs)
    for g in range(10):
        x, y = (wires[len(wires) - 1 - int(rng.integers(min(9, len(wires))))].lane(shifts[(g + k) % 5]) for k in (0, 2))
        wires.extend(c.gate(~x if g & 1 else x, ~y if g & 2 else y))
    outs = [wires[4 + 3 * g + int(rng.integers(3))].lane(shifts[g % 5]) for g in range(10)]
    outs[1], outs[4] = ~outs[1], ~outs[4]
    c.output(*(outs + [c.inputs[0].lane(7), ~c.inputs[1].lane(-7), c.inputs[2]]))
    assert c.info()["nodes"] == 10 and {d for pair in c.gate_shifts for d in pair} == set(shifts)
    # the routed plan, raw
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    index = {d: k + 1 for k, d in enumerate(shifts)}
    routes = np.array([_shift_table(d, G) for d in shifts], dtype=np.int32)
    kind = np.zeros(10, dtype=np.uint32)
    start = (2 * np.arange(11)).astype(np.uint32)
    tr = np.array(c.gates, dtype=np.uint32).reshape(-1)
    tw = np.ones(20, dtype=np.int32)
    tt = np.array([index[d] for pair in c.gate_shifts for d in pair], dtype=np.uint32)
    ov = np.array(c.outputs, dtype=np.uint32)
    ot = np.array([index[d] for d in c.output_shifts], dtype=np.uint32)
    h = ctypes.c_void_p()
    assert L.sgfhe_circuit_create_routed(4, 0, vp(kind), vp(start), vp(tr), None, vp(tw), vp(kind), 10, vp(ov), None, len(ov),
                                         G, 0, None, None, None, len(shifts), vp(routes), vp(tt), vp(ot), None,
                                         ctypes.byref(h)) == 0
    cnt = ctypes.c_uint32()
    assert L.sgfhe_circuit_routes(h, ctypes.byref(cnt)) == 0 and cnt.value == 5
    assert L.sgfhe_circuit_routes(c.handle(), ctypes.byref(cnt)) == 0 and cnt.value == 0
    bits = rng.integers(0, 2, size=(4, inst)).astype(bool)
    inputs = np.ascontiguousarray(_inputs(params, sk, bits, 303))
    try:
        for key in (None, KEY32):
            _set_mode([eng], key)
            want = eng.circuit_run(c, inputs)
            _set_mode([eng], key)
            got = np.full(want.shape, SENTINEL, dtype=np.uint64)
            assert L.sgfhe_circuit_run(eng._h, h, inst, vp(inputs), vp(got)) == 0
            assert got.tobytes() == want.tobytes(), "randomised" if key else "deterministic"
        assert np.array_equal(_decrypt0(params, sk, got), c.evaluate_plain(bits))
    finally:
        L.sgfhe_circuit_destroy(h)
        eng.close()


# ---- random routes ---------------------------------------------------------------------------------------------------

def _random_routed_circuit(S, seed=311):
    """G = 8, 4 inputs, one plane.  Every input is refreshed through a routed term; classic nodes, a gate3 and a sum node
    of weights (2, -1, 1, -2) read bootstrapped wires through random tables with fills; a LUT node and a data LUT node read
    fanned wires with a route and a NOT at every position; routed, negated and constant outputs."""
    rng = np.random.default_rng(seed)
    G = 8
    forms = [lambda: [int(x) for x in rng.integers(-1, G, G)], lambda: [int(x) for x in rng.permutation(G)],
             lambda: [int(rng.integers(G))] * G, lambda: [(t + int(rng.integers(1, G))) % G for t in range(G)],
             lambda: [t ^ 4 for t in range(G)], lambda: [-1] * G]
    table = lambda: forms[int(rng.integers(len(forms)))]()
    c = S.Circuit(4, group=G, planes=1)
    fresh = [c.refresh(w.route(table())) for w in c.inputs]
    boot = list(fresh)
    pick = lambda: boot[int(rng.integers(len(boot)))]
    neg = lambda w: ~w if rng.integers(2) else w
    for g in range(5):
        boot.extend(c.gate(neg(pick()).route(table()), neg(pick()).lane(int(rng.integers(-7, 8))))[:2])
    boot.append(c.gate3(pick().route(table()), ~pick().route(table()), pick())[0])
    hi, mid, low = c.sum_node([(2, pick().route(table())), (-1, neg(pick()).route(table())), (1, pick()),
                               (-2, S.Circuit.TRUE.route(table()))])
    boot += [hi, mid]
    fans = [c.fan(pick().route(table())) for _ in range(4)]
    f = c.lut(0x6B, (~fans[0][2]).route(table()), (~fans[1][1]).route(table()), (~pick()).route(table()))
    d = c.lut_data(0, fans[2][2].route(table()), (~fans[3][1]).route(table()), f[0].route(table()))
    e = c.lut(0xD4, (~d[2]).route(table()), f[1].route([-1] * G), (~d[0]).route(table()))
    c.output(f[0].route(table()), ~d[0].route(table()), e[0], (~e[0]).route(table()), low.route(table()), ~hi.route(table()),
             boot[5].route(table()), c.inputs[0].route(table()), ~c.inputs[1].route([-1] * G), S.Circuit.TRUE.route(table()),
             fresh[2])
    assert len(c.route_tables) > 12 and {"classic", "gate3", "sum", "lut", "data"} <= {c.kind(g) for g in range(c.n_gates)}
    return c


def test_random_routes_against_the_oracles_both_modes(S, oc):
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 312)
    try:
        c = _random_routed_circuit(S)
        cnt = ctypes.c_uint32()
        assert S.lib().sgfhe_circuit_routes(c.handle(), ctypes.byref(cnt)) == 0 and cnt.value == len(c.route_tables)
        inst = 16
        rng = np.random.default_rng(313)
        bits = rng.integers(0, 2, size=(4, inst)).astype(bool)
        data = rng.integers(0, 256, size=(1, inst), dtype=np.uint8)
        inputs = _inputs(params, sk, bits, 314)
        plain = c.evaluate_plain(bits, data)
        assert 0 < plain.sum() < plain.size
        runs = []
        for key in (None, KEY32):
            boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, key)
            want = C.replay_levels(c, inputs, params.r, boot, boot_lut, data=data)
            _set_mode([eng], key)
            got = eng.circuit_run(c, inputs, data=data)
            assert np.array_equal(got, want), "randomised" if key else "deterministic"
            assert np.array_equal(_decrypt0(params, sk, got), plain)
            runs.append(got)
        assert not np.array_equal(runs[0], runs[1])
    finally:
        eng.set_random_flatten(False)
        eng.close()


# ---- a call boundary inside a group ---------------------------------------------------------------------------------

def test_call_boundary_inside_a_group_with_routes_across_it(S, oc):
    """G = 48 over 2736 = 57 * 48 instances, as tests/test_gpu_circuit_lanes.py forces it: level 1 has 3 nodes = 8208
    rows, so call 0 ends at row 8192 = node 2, instance 2720 = lane 32 of the last group, and call 1 holds its other 16
    lanes.  Level 2 reads node 2's wires through swap(32) -- lanes 0 .. 15 read lanes 32 .. 47, the rows of the other
    call, and the reverse -- and through a rotation by 17, and node 0's reversed; randomised, against replay_levels
    through bootstrap_batch on a clone."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 321)
    ref = eng.clone()
    try:
        G, inst = 48, 2736
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        n0, n1, n2 = c.gate(x, y), c.gate(~x, y), c.gate(x, ~c.rot(y, 5))
        top = c.gate(c.swap(n2[2], 32), ~c.rot(n2[1], 17))
        c.output(top[0], top[2], c.reverse(n0[0]), ~c.swap(n2[0], 32), n1[1])
        info = c.info()
        assert (info["levels"], info["nodes"], info["widest"]) == (2, 4, 3)
        assert 3 * inst == 8208 and (C.CALL_ROWS - 2 * inst) % G == 32
        assert c.swap(n2[2], 32).table[:16] == tuple(range(32, 48)) and c.swap(n2[2], 32).table[32:] == tuple(range(16))
        bits = np.random.default_rng(322).integers(0, 2, size=(2, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 323)
        _set_mode([eng, ref], KEY32)
        got = eng.circuit_run(c, inputs)
        calls = []

        def boot(call, a1, b1, a2, b2):
            calls.append(len(b1))
            return ref.bootstrap_batch(a1, b1, a2, b2)
        want = C.replay_levels(c, inputs, params.r, boot)
        assert calls == [8192, 16, inst]
        assert np.array_equal(got, want)
        assert np.array_equal(_decrypt0(params, sk, got), c.evaluate_plain(bits))
    finally:
        ref.close()
        eng.close()


# ---- pure feedback ---------------------------------------------------------------------------------------------------

def test_a_rotating_register_without_any_bootstrap(S, oc):
    """Circuit(1, group=8, registers=1) with no node: the register takes itself rotated by one lane, the output shows it
    before the feedback.  After s steps the state is the input rotated by s lanes inside every group -- the very words:
    nothing is bootstrapped --, after G steps the input; a negated rotation flips every word's sign each step."""
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 331)
    try:
        G, inst, n, r = 8, 24, params.n, params.r
        rng = np.random.default_rng(332)
        state = rng.integers(0, r, size=(1, inst, n + 1), dtype=np.uint64)
        c = S.Circuit(1, group=G, registers=1)
        c.output(c.registers[0])
        c.next_state(c.rot(c.registers[0], 1))
        assert c.info()["nodes"] == 0 and c.route_tables == [tuple((t + 1) % G for t in range(G))]
        rot = lambda v, s: np.roll(v.reshape(inst // G, G, n + 1), -s, axis=1).reshape(inst, n + 1)
        stream = np.zeros((G, 0, inst, n + 1), dtype=np.uint64)
        out, last = eng.circuit_run_steps(c, state, stream)
        assert out.shape == (G, 1, inst, n + 1) and np.array_equal(last, state)
        for s in range(G):
            assert np.array_equal(out[s, 0], rot(state[0], s)), s
        out3, last3 = eng.circuit_run_steps(c, state, stream[:3])
        assert np.array_equal(last3[0], rot(state[0], 3)) and not np.array_equal(last3, state)
        # negated, and a table with a fill: lane 6 takes TRUE (NOT of the fill), lane 7 NOT of lane 0, the others NOT of
        # the lane above
        from sgfhe_jl_amd.circuit import lwe_not
        c2 = S.Circuit(1, group=G, registers=1)
        c2.output(c2.registers[0])
        c2.next_state(~c2.registers[0].route([1, 2, 3, 4, 5, 6, 7, -1]).route([0, 1, 2, 3, 4, 5, 6, 6]))
        assert c2.route_tables == [(1, 2, 3, 4, 5, 6, 7, 7)]
        c3 = S.Circuit(1, group=G, registers=1)
        c3.output(c3.registers[0])
        c3.next_state(~c3.registers[0].route([1, 2, 3, 4, 5, 6, -1, 0]))
        _, st = eng.circuit_run_steps(c3, state, stream[:1])
        src = state[0].reshape(inst // G, G, n + 1)
        want = np.zeros_like(src)
        want[:, :6], want[:, 7] = src[:, 1:7], src[:, 0]
        assert np.array_equal(st[0], lwe_not(want.reshape(inst, n + 1), r))
    finally:
        eng.close()


# ---- the ciphertext form ---------------------------------------------------------------------------------------------

def test_routed_outputs_are_refreshed_or_lifted_never_direct(S, oc):
    """Circuit(2, group=8) at n = 64, one block: a gate wire as it is (direct under PACK_DIRECT), the same wire under the
    IDENTITY table forced past the normalisation (routed all the same: refreshed, or lifted), a rotated, a reversed negated
    and a swapped negated input.  Flags 0, DIRECT and DIRECT | LIFT against replay_ct / replay_ct_direct on a second ctx,
    randomised; the calls each composition makes are the expected ones, and both ctxs have then consumed the same call
    numbers."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _setup64(S, oc, 341, engines=2)
    try:
        n, G = params.n, 8
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        g = c.gate(x, y)
        c.output(g[0], g[0], c.rot(g[2], 1), ~c.reverse(g[1]), c.swap(~x, 4), g[1].route([-1, 0, 0, 3, 3, 5, 7, -1]))
        c.output_shifts[1] = tuple(range(G))
        c._invalidate()
        assert c.route_tables[0] == tuple(range(G)) and len(c.route_tables) == 5
        bits = np.random.default_rng(342).integers(0, 2, size=(2, 1, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, bits, 343)
        plain = c.evaluate_plain(bits.reshape(2, -1))
        assert np.array_equal(plain[0], plain[1])
        seen = []

        def boot(raw):
            def f(call, a1, b1, a2, b2):
                seen.append(("boot", call, len(b1)))
                return ref.bootstrap_batch(a1, b1, a2, b2, raw=raw)
            return f

        def pack(call, pa, pb):
            seen.append(("pack", call, len(pa)))
            return ref.pack_encrypted_bits(pa, pb)

        def tail(call, group):
            seen.append(("tail", call, len(group)))
            return ref.pack_lwe_modq(group)

        probe_rows = _inputs(params, sk, bits.reshape(2, -1)[:, :3], 344)
        results = {}
        for flags in (0, DIRECT, DIRECT | LIFT):
            direct, lift = bool(flags & DIRECT), bool(flags & LIFT)
            _set_mode([eng, ref], KEY32)
            del seen[:]
            (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=direct, lift=lift)
            if not direct:
                (rw, rv), rlwe = C.replay_ct(c, a, b, params, boot(False), pack)
                assert seen == [("boot", 0, n), ("pack", 1, 6)]
            else:
                (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, boot(True), tail, lift=lift)
                # output 0 alone is direct: five ciphertexts are refreshed as one call of 5 n rows, or lifted without a call
                assert seen == ([("boot", 0, n), ("tail", 1, 6)] if lift else [("boot", 0, n), ("boot", 1, 5 * n), ("tail", 2, 6)])
            assert np.array_equal(lwe, rlwe), flags
            assert np.array_equal(w, rw) and np.array_equal(v, rv), flags
            assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain), flags
            # the same call numbers consumed: the next call draws alike on both
            x3, y3 = probe_rows[0], probe_rows[1]
            assert np.array_equal(eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n]),
                                  ref.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])), flags
            results[flags] = (w, v)
        # output 1 is refreshed under DIRECT and lifted under DIRECT | LIFT: other words
        assert not np.array_equal(results[DIRECT][0][1], results[DIRECT | LIFT][0][1])
    finally:
        eng.close()
        ref.close()


# ---- the probe -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_probe_of_a_routed_circuit(S, oc, mode):
    """The records of every wire against tests/noise_ref.py on the LWEs of the same nodes with every wire an output: only
    the bit table applies the routes, so a wrong table would show as wrong bits."""
    key = KEY32 if mode == "randomised" else None
    params, o, lo, sk, bkey, (A, B) = _setup64(S, oc, 351, engines=2)
    try:
        G, inst = 8, 24
        rng = np.random.default_rng(352)
        c = S.Circuit(3, group=G)
        wires = list(c.inputs)
        tables = [[int(t) for t in rng.integers(-1, G, G)] for _ in range(3)] + [[t ^ 2 for t in range(G)], [G - 1 - t for t in range(G)]]
        for g in range(7):
            x, y = (wires[int(rng.integers(len(wires)))].route(tables[(g + k) % 5]) for k in (0, 3))
            wires.extend(c.gate(~x if g & 1 else x, y.lane(1) if g == 3 else (~y if g & 2 else y)))
        c.output(*[wires[3 + 3 * g].route(tables[g % 5]) for g in range(7)])
        assert c.info()["nodes"] == 7
        d = S.Circuit(3, group=G)
        d.gates, d.gate_shifts = list(c.gates), list(c.gate_shifts)
        d.output(*[S.Wire(w) for w in range(3 + 3 * 7)])
        assert d.schedule() == c.schedule()
        bits = rng.integers(0, 2, size=(3, inst)).astype(np.uint8)
        inputs = _inputs(params, sk, bits, 353)
        _set_mode([A, B], key)
        out, stats = A.circuit_probe(c, inputs, sk, bits)
        assert np.array_equal(out, B.circuit_run(c, inputs))
        _set_mode([B], key)
        lwes = B.circuit_run(d, inputs)
        plain = d.evaluate_plain(bits)
        assert len(stats) == 3 + 3 * 7 == len(lwes)
        for w, (rows, exp) in enumerate(zip(lwes, plain)):
            assert stats[w] == S.NoiseStats(*NR.record_zr(params, sk, rows, exp)), w
            assert stats[w].rows == inst and stats[w].wrong == 0, w
    finally:
        A.close()
        B.close()


# ---- errors ----------------------------------------------------------------------------------------------------------

def test_routes_errors_leave_the_outputs_untouched(S, oc):
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 361)
    try:
        n, m, G = params.n, params.m, 8
        L = S.lib()
        ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        c.output(c.gate(c.rot(x, 3), ~c.reverse(y))[0], c.swap(x, 1))
        bits = np.random.default_rng(362).integers(0, 2, size=(2, 24)).astype(bool)
        inputs = np.ascontiguousarray(_inputs(params, sk, bits, 363))
        # instances = 20 with G = 8
        short = np.ascontiguousarray(inputs[:, :20])
        out = np.full((2, 20, n + 1), SENTINEL, dtype=np.uint64)
        assert L.sgfhe_circuit_run(eng._h, c.handle(), 20, ptr(short), ptr(out)) == INVALID
        stats = np.full((2 + 3, 8), SENTINEL, dtype=np.uint64)
        sk64 = np.ascontiguousarray(sk, dtype=np.uint64)
        b8 = np.ascontiguousarray(bits[:, :20].astype(np.uint8))
        assert L.sgfhe_circuit_run_probe(eng._h, c.handle(), 20, ptr(short), ptr(out), ptr(sk64), ptr(b8), ptr(stats)) == INVALID
        assert np.all(out == SENTINEL) and np.all(stats == SENTINEL)
        # a routed plan with a register goes through the _steps entries only
        s = S.Circuit(2, group=G, registers=1)
        s.output(s.gate(*s.inputs)[0])
        s.next_state(s.rot(s.inputs[1], 1))
        full = np.full((1, 24, n + 1), SENTINEL, dtype=np.uint64)
        assert L.sgfhe_circuit_run(eng._h, s.handle(), 24, ptr(inputs), ptr(full)) == INVALID and np.all(full == SENTINEL)
        # the ciphertext form with G = 48 at n = 64: a group would straddle two ciphertexts
        c48 = S.Circuit(1, group=48)
        c48.output(c48.gate(c48.inputs[0], c48.reverse(c48.inputs[0]))[0])
        cb = np.random.default_rng(364).integers(0, 2, size=(1, 3, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, cb, 365)
        ow = np.full((1, 3, m), SENTINEL, dtype=np.uint64)
        ov, ol = ow.copy(), np.full((1, 3 * n, n + 1), SENTINEL, dtype=np.uint64)
        for flags in (0, DIRECT, DIRECT | LIFT):
            assert L.sgfhe_circuit_run_ct_ex(eng._h, c48.handle(), 3, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol), flags) == INVALID
        assert np.all(ow == SENTINEL) and np.all(ov == SENTINEL) and np.all(ol == SENTINEL)
        # a refused plan leaves *out NULL
        z = np.zeros(4, dtype=np.uint32)
        bad = np.array([0, 1, 2, 3, 4, 5, 6, 8], dtype=np.int32)
        one = np.ones(1, dtype=np.uint32)
        h = ctypes.c_void_p(0xDEAD)
        assert L.sgfhe_circuit_create_routed(1, 0, None, ptr(z), None, None, None, None, 0, ptr(z), None, 1, G, 0, None, None,
                                             None, 1, ptr(bad), None, ptr(one), None, ctypes.byref(h)) == INVALID
        assert h.value is None
        # correct runs on the same ctx afterwards
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(_decrypt0(params, sk, got), c.evaluate_plain(bits))
        lwe48 = _inputs(params, sk, cb.reshape(1, -1)[:, :96], 366)
        assert np.array_equal(_decrypt0(params, sk, eng.circuit_run(c48, lwe48)), c48.evaluate_plain(cb.reshape(1, -1)[:, :96]))
    finally:
        eng.close()


# ---- the sort --------------------------------------------------------------------------------------------------------

def test_bitonic_sort_decrypts_sorted_and_equals_the_replay(S, oc):
    """bitonic_sort(3, 8) over two groups: 42 nodes in 26 levels, every lane exchange a route.  Word for word
    replay_levels on a second ctx's primitives; the outputs decrypt to sorted()."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 371)
    ref = eng.clone()
    try:
        width, G, inst = 3, 8, 16
        c = S.bitonic_sort(width, G)
        assert c.info()["nodes"] == 42 and c.info()["levels"] == 26
        vals = np.array([5, 1, 7, 0, 3, 3, 6, 2, 4, 4, 4, 0, 7, 7, 1, 0])
        bits = np.array([(vals >> i) & 1 for i in range(width)], dtype=bool)
        inputs = _inputs(params, sk, bits, 372)
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(got, C.replay_levels(c, inputs, params.r, *_second_ctx(ref)))
        dec = _decrypt0(params, sk, got)
        assert np.array_equal(dec, c.evaluate_plain(bits))
        nums = sum(dec[i].astype(int) << i for i in range(width))
        assert nums.tolist() == sorted(vals[:8].tolist()) + sorted(vals[8:].tolist())
    finally:
        ref.close()
        eng.close()


# ---- the full-size ring ----------------------------------------------------------------------------------------------

def test_a_routed_plan_at_p1024_on_a_clone(S, oc, gpu_keys):
    """Params(1024), G = 8, one group: one level of one node = 8 rows, every term and every output routed.  On a clone of
    the session's engine, against replay_levels through bootstrap_batch on a second clone."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, shared = gpu_keys.engine(1024)
    eng, ref = shared.clone(), shared.clone()
    try:
        G = 8
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        g = c.gate(c.rot(x, 3), ~c.swap(y, 5))
        c.output(c.reverse(g[0]), ~c.bcast(g[2], 6), g[1].route([-1, 0, 1, 2, 7, 7, 3, -1]))
        bits = np.random.default_rng(381).integers(0, 2, size=(2, G)).astype(bool)
        inputs = _inputs(params, sk, bits, 382)
        got = eng.circuit_run(c, inputs)
        want = C.replay_levels(c, inputs, params.r, lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2))
        assert got.shape == (3, G, params.n + 1) and np.array_equal(got, want)
        assert np.array_equal(_decrypt0(params, sk, got), c.evaluate_plain(bits))
    finally:
        ref.close()
        eng.close()


def test_example_encrypted_sort_runs(S):
    """examples/encrypted_sort.py: encrypt -> one evaluate_circuit / evaluate_circuit_ct call -> decrypt, at Params(64):
    two groups of eight 3-bit numbers in the LWE form, one block of eight groups in the ciphertext form."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import encrypted_sort
    encrypted_sort.main(64, 3, 8, 2)
    encrypted_sort.main(64, 2, 8, 1, ct=True)
