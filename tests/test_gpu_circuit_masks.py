"""Lane masks on the device (sgfhe_circuit_create_masked).  A masked node takes a row only on the
lanes that are set, and all its wires are the constant FALSE on the others, so: a random circuit of classic, sum, LUT and
data LUT nodes under five masks, read through NOTs, shifts and routes, against circuit.replay_levels on the two oracles
in both flatten modes; the off lanes as exact trivial LWEs -- zero rows, and under NOT (0, Dr), (0, Dr/2), (0, Dr/4) --
in a slot that held a full-lane wire before; a scripted run on a keyless ctx, every staged row, descriptor and output
against Python integers; a level of 10000 rows whose call boundary falls inside a node's pairs; the ciphertext form under
the three flag sets; a stepped run whose register a masked node feeds; the device-resident entry; the probe's refusal;
bitonic_sort(masked=True), lane_reduce and packed_equal decrypted; one masked plan at Params(1024).  Every comparison of
ciphertext words is for equality."""

import ctypes
import os
import sys

import numpy as np
import pytest

import lut_ref as LR
import noise_ref as NR
import pack_lift_ref as PL

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(9, 41))
SENTINEL = 0xA5A5A5A5A5A5A5A5
UNSUPPORTED = -2
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
    return np.ascontiguousarray(NR.handmade_zr(params, sk, rng, e, flat).reshape(np.asarray(bits).shape + (params.n + 1,)))


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


def _on(lanes, G, inst):
    return np.array([lanes is None or (t % G) in lanes for t in range(inst)])


MASKS8 = [[0], [7], [0, 1, 2, 4, 5, 6, 7], [0, 2, 4, 6], None]     # lane 0 only, lane 7 only, all but one, alternating, none


# ---- a random circuit under every mask ------------------------------------------------------------------------------

def _random_masked_circuit(S, seed=411):
    """G = 8, 4 inputs, one plane.  Every input is refreshed under one of the masks; classic nodes, a gate3 and a sum node
    read bootstrapped wires -- masked ones among them -- plain, negated, shifted and routed, each under the next mask; LUT
    and data LUT nodes read fanned wires with a NOT at every position; outputs name masked wires plain, negated, shifted
    and routed."""
    rng = np.random.default_rng(seed)
    G = 8
    mask = lambda k: MASKS8[k % 5]
    table = lambda: [int(x) for x in rng.integers(-1, G, G)]
    c = S.Circuit(4, group=G, planes=1)
    fresh = [c.refresh(w, lanes=mask(i)) for i, w in enumerate(c.inputs)]
    boot = list(fresh)
    pick = lambda: boot[int(rng.integers(len(boot)))]
    neg = lambda w: ~w if rng.integers(2) else w
    for g in range(5):
        boot.extend(c.gate(neg(pick()).route(table()), neg(pick()).lane(int(rng.integers(-7, 8))), lanes=mask(g + 1))[:2])
    boot.append(c.gate3(pick().lane(1), ~pick(), pick().route(table()), lanes=mask(2))[0])
    hi, mid, low = c.sum_node([(2, pick().lane(-2)), (-1, neg(pick())), (1, pick()), (-2, S.Circuit.TRUE)], lanes=mask(3))
    boot += [hi, mid]
    fans = [c.fan(neg(pick()).lane(int(rng.integers(-2, 3))), lanes=mask(k)) for k in range(4)]
    f = c.lut(0x6B, ~fans[0][2], (~fans[1][1]).lane(1), ~pick(), lanes=mask(1))
    d = c.lut_data(0, fans[2][2].route(table()), ~fans[3][1], f[0].lane(-1), lanes=mask(2))
    e = c.lut(0xD4, ~d[2], f[1].lane(3), ~d[0], lanes=mask(0))
    c.output(f[0], ~d[0], e[0].lane(-1), (~e[0]).route(table()), low, ~hi.lane(2), boot[5], ~boot[7].route(table()), fresh[0],
             ~fresh[1], fresh[2].lane(1), mid)
    assert len(c.mask_tables) == 4 and {"classic", "gate3", "sum", "lut", "data"} <= {c.kind(g) for g in range(c.n_gates)}
    return c


def test_random_masks_against_the_oracles_both_modes(S, oc):
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 412)
    try:
        c = _random_masked_circuit(S)
        info = c.info()
        assert info["rows_per_group"] == sum(len(c.lanes_on(g)) for lv in c.schedule() for g in lv) < info["nodes"] * 8
        inst = 24
        rng = np.random.default_rng(413)
        bits = rng.integers(0, 2, size=(4, inst)).astype(bool)
        data = rng.integers(0, 256, size=(1, inst), dtype=np.uint8)
        inputs = _inputs(params, sk, bits, 414)
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


# ---- the off lanes ---------------------------------------------------------------------------------------------------

def test_off_lanes_are_trivial_lwes_in_a_reused_slot(S, oc):
    """Circuit(3, group=8, registers=2) with registers of scales 1 and 2: refresh, fan, then a LUT node M on lanes {0, 3}.
    M's wire +0 takes the slot the refreshed wire held on every lane -- a bootstrap's output rows, none of them zero --
    which nothing reads after the fan (info: 6 slots where 8 wires are written).  Outputs M
    and ~M, next states ~M at Dr/2 and ~M at Dr/4: on the off lanes the rows are all zero, and (0, Dr), (0, Dr/2),
    (0, Dr/4) under NOT; on the others they are what replay_steps gives."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 421)
    ref = eng.clone()
    try:
        G, inst, n, r = 8, 16, params.n, params.r
        c = S.Circuit(3, group=G, registers=2, reg_scales=[1, 2])
        x = c.stream_inputs[0]
        a = c.refresh(x)
        f = c.fan(a)
        m = c.lut(0x96, f[2], ~f[1], f[0], lanes=[0, 3])
        c.output(m[0], ~m[0])
        c.next_state(~m[1], ~m[2])
        info = c.info()
        assert (info["levels"], info["nodes"], info["slots"], info["rows_per_group"]) == (3, 3, 6, 8 + 8 + 2)
        bits = np.random.default_rng(422).integers(0, 2, size=(1, 1, inst)).astype(bool)
        bits[0, 0, :4] = True                                        # (f(1, 0, 1) = 0 and f(0, 1, 0) = 1: both values occur)
        stream = _inputs(params, sk, bits, 423)
        out, state = eng.circuit_run_steps(c, None, stream)
        want_out, want_state = C.replay_steps(c, None, stream, r, *_second_ctx(ref))
        assert np.array_equal(out, want_out) and np.array_equal(state, want_state)
        off = ~_on([0, 3], G, inst)
        word = lambda b: np.array([0] * n + [b], dtype=np.uint64)
        assert not out[0, 0][off].any() and out[0, 0][~off].any()
        assert np.array_equal(out[0, 1][off], np.tile(word(r // 4), (off.sum(), 1)))
        assert np.array_equal(state[0][off], np.tile(word(r // 8), (off.sum(), 1)))
        assert np.array_equal(state[1][off], np.tile(word(r // 16), (off.sum(), 1)))
        dec = _decrypt0(params, sk, out[0])
        assert np.array_equal(dec, c.evaluate_plain(np.concatenate([np.zeros((2, inst), bool), bits[0]])))
    finally:
        ref.close()
        eng.close()


# ---- the scripted run ------------------------------------------------------------------------------------------------

def test_scripted_run_stages_the_pairs_and_fills_the_rest(S):
    """debug_circuit_script on a ctx without a key: G = 4, 8 instances, a masked classic node, a masked sum node, a masked
    LUT node beside an unmasked classic node, read through NOTs and shifts.  The script holds one row per (node, lane that
    is on, group) and no other -- every scripted word is non-zero, so a zero output row is a row no script row reached --
    and replay_levels with a 'bootstrap' that hands the same script out says what every call must have staged."""
    from sgfhe_jl_amd import circuit as C
    params = S.Params(64)
    eng = S.Engine(params)
    try:
        G, inst, n, r = 4, 8, params.n, params.r
        rng = np.random.default_rng(431)
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        a = c.gate(x, ~y.lane(1), lanes=[0, 2])
        hi, mid, low = c.sum_node([(2, x), (-1, y), (1, S.Circuit.TRUE)], lanes=[3])
        b = c.gate(a[0].lane(1), ~low.lane(-1))
        fa = c.fan(~a[1], lanes=[1, 2, 3])
        f = c.lut(0xE8, ~fa[2], fa[1].lane(-1), b[1], lanes=[0, 1, 2])
        c.output(a[0], ~a[2], hi, low, ~low, b[0], b[2], fa[0], f[0], ~f[0].lane(1))
        assert c.info()["rows_per_group"] == 2 + 1 + 4 + 3 + 3
        calls = eng.debug_circuit_script_calls(c, inst)
        assert calls == [(2 * (2 + 1), False), (2 * (4 + 3), False), (2 * 3, False)]
        results = [rng.integers(1, r, size=(rows, 3, n + 1), dtype=np.uint64) for rows, _ in calls]
        inputs = rng.integers(0, r, size=(2, inst, n + 1), dtype=np.uint64)
        staged = {}

        def boot(call, a1, b1, a2, b2):
            staged[call] = np.stack([np.concatenate([a1, b1[:, None]], axis=1), np.concatenate([a2, b2[:, None]], axis=1)], axis=1)
            return results[call]

        def boot_lut(call, a_, b_, tables, idx):
            rows = staged.setdefault(call, np.zeros((len(results[call]), 2, n + 1), dtype=np.uint64))
            rows[idx, 0] = np.concatenate([a_, b_[:, None]], axis=1)
            lut_words[call][idx] = 0x100 | tables.astype(np.uint32)
            return results[call][idx]

        lut_words = [np.zeros(rows, dtype=np.uint32) for rows, _ in calls]
        want = C.replay_levels(c, inputs, r, boot, boot_lut)
        got = eng.debug_circuit_script(c, results, inputs)
        for k in range(len(calls)):
            assert np.array_equal(got["staged"][k], staged[k]), k
            assert np.array_equal(got["lut"][k], lut_words[k]), k
        assert np.array_equal(got["out"], want)
        # by hand: call 0 is node `a` at lanes 0, 2 then the sum node at lane 3, each over the two groups
        for j, t in enumerate((0, 4, 2, 6)):
            assert np.array_equal(got["staged"][0][j, 0], inputs[0, t]) and \
                np.array_equal(got["staged"][0][j, 1], C.lwe_not(inputs[1, t + 1], r))
            assert np.array_equal(got["out"][0, t], results[0][j, 0])                         # a[0] where it is on
        one = np.array([0] * n + [r // 4], dtype=np.uint64)
        for j, t in enumerate((3, 7)):
            u = (2 * inputs[0, t] + np.uint64(r) - inputs[1, t] + one) & np.uint64(r - 1)
            assert np.array_equal(got["staged"][0][4 + j, 0], u) and not got["staged"][0][4 + j, 1].any()
            assert np.array_equal(got["out"][3, t], (u - 2 * results[0][4 + j, 0]) & np.uint64(r - 1))     # LOW = U - 2 HI
        off_a, off_s = ~_on([0, 2], G, inst), ~_on([3], G, inst)
        assert not got["out"][0][off_a].any() and not got["out"][2][off_s].any() and not got["out"][3][off_s].any()
        assert np.array_equal(got["out"][1][off_a], np.tile(one, (4, 1))) and np.array_equal(got["out"][4][off_s], np.tile(one, (6, 1)))
        assert not got["out"][7][~_on([1, 2, 3], G, inst)].any() and not got["out"][8][~_on([0, 1, 2], G, inst)].any()
        assert got["out"][0][~off_a].all() and got["out"][5].all() and got["out"][6].all()     # scripted words, none zero
    finally:
        eng.close()


# ---- a call boundary inside a node's pairs --------------------------------------------------------------------------

def test_call_boundary_inside_a_nodes_pairs(S, oc):
    """G = 8 over 3200 instances, one level of five nodes with 8, 3, 5, 8, 1 lanes set: 25 pairs of 400 groups = 10000 rows,
    so call 0 ends at row 8192 inside pair 20, the fourth node at lane 4.  Deterministic: against replay_levels through a
    second ctx's bootstrap_batch.  Randomised: against the same with both ctxs on one draw stream -- a row draws at its
    index within its call -- and rows 0, 8191, 8192 and 9999 against the oracle at (call, index) = (0, 0), (0, 8191),
    (1, 0), (1, 1807)."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 441)
    ref = eng.clone()
    try:
        G, inst, n = 8, 3200, params.n
        lanes = [None, [1, 4, 6], [0, 2, 3, 5, 7], None, [5]]
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        nodes = [c.gate(x if g & 1 else ~x, y.lane(g - 2), lanes=lanes[g]) for g in range(5)]
        c.output(*[w for nd in nodes for w in (nd[0], ~nd[2])])
        info = c.info()
        assert (info["levels"], info["nodes"], info["rows_per_group"]) == (1, 5, 25)
        rk, ri = C.level_row_map(c, [0, 1, 2, 3, 4], inst)
        assert len(rk) == 10000 and (rk[8191], ri[8191], rk[8192], ri[8192]) == (3, 191 * 8 + 4, 3, 192 * 8 + 4)
        bits = np.random.default_rng(442).integers(0, 2, size=(2, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 443)
        plain = c.evaluate_plain(bits)
        for key in (None, KEY32):
            _set_mode([eng, ref], key)
            got = eng.circuit_run(c, inputs)
            calls = []

            def boot(call, a1, b1, a2, b2):
                calls.append((call, np.concatenate([a1, b1[:, None]], axis=1), np.concatenate([a2, b2[:, None]], axis=1)))
                return ref.bootstrap_batch(a1, b1, a2, b2)
            want = C.replay_levels(c, inputs, params.r, boot)
            assert [len(u) for _, u, _ in calls] == [8192, 1808]
            assert np.array_equal(got, want), "randomised" if key else "deterministic"
            assert np.array_equal(_decrypt0(params, sk, got), plain)
        # the randomised run's rows at both sides of the boundary, from the oracle
        khat = o.key_transform(bkey)
        for R in (0, 8191, 8192, 9999):
            call, idx = divmod(R, C.CALL_ROWS)
            u, v = calls[call][1][idx:idx + 1], calls[call][2][idx:idx + 1]
            row = o.bootstrap_batch(khat, u[:, :n], u[:, n], v[:, :n], v[:, n], opt=True,
                                    rnd=(KEY32, call, np.array([idx], dtype=np.uint32)))[0]
            k, t = int(rk[R]), int(ri[R])
            assert np.array_equal(got[2 * k, t], row[0]) and np.array_equal(got[2 * k + 1, t], C.lwe_not(row[2], params.r)), R
    finally:
        eng.set_random_flatten(False)
        ref.close()
        eng.close()


# ---- the ciphertext form ---------------------------------------------------------------------------------------------

def test_masked_outputs_are_refreshed_or_lifted_never_direct(S, oc):
    """Circuit(2, group=8) at n = 64, one block: an unmasked node g and a node m on lanes {0, 3, 5} in one level call of
    64 + 24 rows.  Outputs g AND (direct under PACK_DIRECT), m AND and ~m OR (masked: refreshed, or lifted), g XOR
    (direct).  Flags 0, DIRECT and DIRECT | LIFT against replay_ct / replay_ct_direct on a second ctx, randomised; the calls
    each composition makes are the expected ones; everything decrypts."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _setup64(S, oc, 451, engines=2)
    try:
        n, G = params.n, 8
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        g = c.gate(x, y)
        m = c.gate(x, ~y.lane(1), lanes=[0, 3, 5])
        c.output(g[0], m[0], ~m[1], g[2])
        rows = (8 + 3) * (n // G)
        assert c.info()["rows_per_group"] == 11
        bits = np.random.default_rng(452).integers(0, 2, size=(2, 1, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, bits, 453)
        plain = c.evaluate_plain(bits.reshape(2, -1))
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

        results = {}
        for flags in (0, DIRECT, DIRECT | LIFT):
            direct, lift = bool(flags & DIRECT), bool(flags & LIFT)
            _set_mode([eng, ref], KEY32)
            del seen[:]
            (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=direct, lift=lift)
            if not direct:
                (rw, rv), rlwe = C.replay_ct(c, a, b, params, boot(False), pack)
                assert seen == [("boot", 0, rows), ("pack", 1, 4)]
            else:
                (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, boot(True), tail, lift=lift)
                # outputs 0 and 3 are direct: the two masked ones are refreshed as one call of 2 n rows, or lifted
                assert seen == ([("boot", 0, rows), ("tail", 1, 4)] if lift else
                                [("boot", 0, rows), ("boot", 1, 2 * n), ("tail", 2, 4)])
            assert np.array_equal(lwe, rlwe), flags
            assert np.array_equal(w, rw) and np.array_equal(v, rv), flags
            assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain), flags
            results[flags] = (w, v)
        assert not np.array_equal(results[DIRECT][0][1], results[DIRECT | LIFT][0][1])      # refreshed against lifted
        assert eng.debug_circuit_script_calls(c, 1, ct=True, pack=True, direct=True) == [(rows, True), (2 * n, True)]
    finally:
        eng.close()
        ref.close()


# ---- a stepped run ---------------------------------------------------------------------------------------------------

def test_a_register_fed_by_a_masked_node_over_three_steps(S, oc):
    """Circuit(2, group=4, registers=1): the register is fed by MAJ of a gate3 on lanes {0, 2} that reads the register
    itself plain and shifted, so from the second step on the node reads its own FALSE off lanes.  3 steps, randomised,
    against replay_steps on a clone: the calls' rows, the outputs of every step, the last state."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 461)
    ref = eng.clone()
    try:
        G, inst, steps = 4, 12, 3
        c = S.Circuit(2, group=G, registers=1)
        reg, x = c.inputs
        maj, _, x3 = c.gate3(x, ~reg, reg.lane(1), lanes=[0, 2])
        top = c.gate(maj.lane(-1), ~x)
        c.output(x3, ~maj, top[1])
        c.next_state(maj)
        assert c.info()["rows_per_group"] == 2 + 4
        rng = np.random.default_rng(462)
        sbits = rng.integers(0, 2, size=(steps, 1, inst)).astype(bool)
        state0 = _inputs(params, sk, rng.integers(0, 2, size=(1, inst)).astype(bool), 463)
        stream = _inputs(params, sk, sbits, 464)
        _set_mode([eng, ref], KEY32)
        out, state = eng.circuit_run_steps(c, state0, stream)
        seen = []

        def boot(call, a1, b1, a2, b2):
            seen.append((call, len(b1)))
            return ref.bootstrap_batch(a1, b1, a2, b2)
        want_out, want_state = C.replay_steps(c, state0, stream, params.r, boot)
        assert seen == [(2 * s + L, rows) for s in range(steps) for L, rows in ((0, 2 * 3), (1, 4 * 3))]
        assert np.array_equal(out, want_out) and np.array_equal(state, want_state)
        assert not state[0][~_on([0, 2], G, inst)].any()
    finally:
        eng.set_random_flatten(False)
        ref.close()
        eng.close()


# ---- the device-resident entry ---------------------------------------------------------------------------------------

def test_device_resident_run_gives_the_bytes_of_the_host_form(S, oc):
    import torch
    params, o, lo, sk, bkey, (eng, ref) = _setup64(S, oc, 471, engines=2)
    try:
        c = _random_masked_circuit(S, seed=472)
        inst = 16
        rng = np.random.default_rng(473)
        bits = rng.integers(0, 2, size=(4, inst)).astype(bool)
        data = rng.integers(0, 256, size=(1, inst), dtype=np.uint8)
        inputs = _inputs(params, sk, bits, 474)
        _set_mode([eng, ref], KEY32)
        want = ref.circuit_run(c, inputs, data=data)
        tx = torch.from_numpy(inputs.view(np.int64)).cuda()
        td = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        out = eng.circuit_run_device(c, tx, data=td)
        eng.sync()
        got = out.view(torch.int64).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want)
        assert np.array_equal(_decrypt0(params, sk, got), c.evaluate_plain(bits, data))
    finally:
        eng.set_random_flatten(False)
        eng.close()
        ref.close()


# ---- the probe -------------------------------------------------------------------------------------------------------

def test_probe_entries_refuse_a_masked_plan(S, oc):
    """SGFHE_ERR_UNSUPPORTED with a message, outputs and records untouched, and no call number taken: the next randomised
    call draws as call 0 does on a second ctx."""
    params, o, lo, sk, bkey, (eng, ref) = _setup64(S, oc, 481, engines=2)
    try:
        n, G, inst = params.n, 4, 8
        L = S.lib()
        ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        c = S.Circuit(2, group=G, planes=1)
        x, y = c.inputs
        fx = c.fan(c.refresh(x))
        c.output(c.gate(x, y, lanes=[1])[0], c.lut_data(0, fx[2], fx[1], fx[0])[0])
        bits = np.random.default_rng(482).integers(0, 2, size=(2, inst)).astype(np.uint8)
        inputs = _inputs(params, sk, bits, 483)
        data = np.zeros((1, inst), dtype=np.uint8)
        sk64 = np.ascontiguousarray(sk, dtype=np.uint64)
        _set_mode([eng, ref], KEY32)
        out = np.full((2, inst, n + 1), SENTINEL, dtype=np.uint64)
        stats = np.full((2 + 3 * c.n_gates, 8), SENTINEL, dtype=np.uint64)
        rc = L.sgfhe_circuit_run_probe_data(eng._h, c.handle(), inst, ptr(inputs), ptr(data), ptr(out), ptr(sk64), ptr(bits),
                                            ptr(stats))
        assert rc == UNSUPPORTED and b"lane masks" in L.sgfhe_last_error_string(eng._h)
        d = S.Circuit(2, group=G)
        d.output(d.gate(*d.inputs, lanes=[1])[0])
        rc = L.sgfhe_circuit_run_probe(eng._h, d.handle(), inst, ptr(inputs), ptr(out), ptr(sk64), ptr(bits), ptr(stats))
        assert rc == UNSUPPORTED and b"lane masks" in L.sgfhe_last_error_string(eng._h)
        assert np.all(out == SENTINEL) and np.all(stats == SENTINEL)
        with pytest.raises(S.SgfheError) as err:
            eng.circuit_probe(d, inputs, sk, bits)
        assert err.value.code == UNSUPPORTED
        x3, y3 = inputs[0], inputs[1]
        assert np.array_equal(eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n]),
                              ref.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n]))
        # the plan itself runs
        _set_mode([eng], None)
        got = eng.circuit_run(d, inputs)
        assert np.array_equal(_decrypt0(params, sk, got), d.evaluate_plain(bits.astype(bool)))
    finally:
        eng.set_random_flatten(False)
        eng.close()
        ref.close()


# ---- the builders ----------------------------------------------------------------------------------------------------

def test_masked_sort_reduce_and_equal_decrypt_to_python(S, oc):
    """bitonic_sort(3, 8, masked=True) over two groups against sorted() and word for word against replay_levels on a
    clone, 264 rows a group; lane_reduce at G = 8 for AND, OR and XOR against all / any / parity; packed_equal(8) against
    ==."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _setup64(S, oc, 491)
    ref = eng.clone()
    try:
        width, G, inst = 3, 8, 16
        c = S.bitonic_sort(width, G, masked=True)
        assert c.info()["rows_per_group"] == 264 and S.bitonic_sort(width, G).rows_per_group() == 336
        assert sum(rows for rows, _ in eng.debug_circuit_script_calls(c, inst)) == 264 * 2
        vals = np.array([5, 1, 7, 0, 3, 3, 6, 2, 4, 4, 4, 0, 7, 7, 1, 0])
        bits = np.array([(vals >> i) & 1 for i in range(width)], dtype=bool)
        inputs = _inputs(params, sk, bits, 492)
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(got, C.replay_levels(c, inputs, params.r, *_second_ctx(ref)))
        dec = _decrypt0(params, sk, got)
        nums = sum(dec[i].astype(int) << i for i in range(width))
        assert nums.tolist() == sorted(vals[:8].tolist()) + sorted(vals[8:].tolist())
        rng = np.random.default_rng(493)
        v = rng.integers(0, 2, size=(1, 5 * G)).astype(bool)
        v[0, :G], v[0, G:2 * G] = True, False
        words = v[0].reshape(5, G)
        lwe = _inputs(params, sk, v, 494)
        for which, fold in ((0, [all(w) for w in words]), (1, [any(w) for w in words]), (2, [sum(w) % 2 == 1 for w in words])):
            d = S.Circuit(1, group=G)
            d.output(C.lane_reduce(d, d.inputs[0], which, G))
            assert d.info()["rows_per_group"] == 7
            out = eng.circuit_run(d, lwe)[0]
            assert _decrypt0(params, sk, out).reshape(5, G)[:, 0].tolist() == fold, which
            assert not out.reshape(5, G, -1)[:, 1:].any()                               # FALSE elsewhere: the exact trivial LWE
        e = S.packed_equal(8)
        assert e.info()["rows_per_group"] == 15
        xy = rng.integers(0, 2, size=(2, 6 * 8)).astype(bool)
        xy[1, :24] = xy[0, :24]
        xy[1, 23] ^= True
        out = eng.circuit_run(e, _inputs(params, sk, xy, 495))[0]
        want = [list(p) == list(q) for p, q in zip(xy[0].reshape(6, 8), xy[1].reshape(6, 8))]
        assert want[:3] == [True, True, False] and _decrypt0(params, sk, out).reshape(6, 8)[:, 0].tolist() == want
        assert np.array_equal(_decrypt0(params, sk, out), e.evaluate_plain(xy)[0])
    finally:
        ref.close()
        eng.close()


# ---- the full-size ring ----------------------------------------------------------------------------------------------

def test_a_masked_plan_at_p1024_on_a_clone(S, oc, gpu_keys):
    """Params(1024), G = 8, two groups: a node on lanes {1, 4, 6}, a node on lane 4 that reads it plain and shifted, an
    unmasked node that reads both: 2 (3 + 1 + 8) rows.  On a clone of the session's engine, against replay_levels through
    bootstrap_batch on a second clone."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, shared = gpu_keys.engine(1024)
    eng, ref = shared.clone(), shared.clone()
    try:
        G, inst = 8, 16
        c = S.Circuit(2, group=G)
        x, y = c.inputs
        g = c.gate(x, ~y.lane(1), lanes=[1, 4, 6])
        h = c.gate(g[0], ~g[2].lane(2), lanes=[4])
        t = c.gate(~h[1].lane(3), g[1])
        c.output(g[2], ~h[1], t[0], ~t[2])
        assert c.info()["rows_per_group"] == 12
        bits = np.random.default_rng(497).integers(0, 2, size=(2, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 498)
        got = eng.circuit_run(c, inputs)
        want = C.replay_levels(c, inputs, params.r, lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2))
        assert got.shape == (4, inst, params.n + 1) and np.array_equal(got, want)
        assert np.array_equal(_decrypt0(params, sk, got), c.evaluate_plain(bits))
        assert not got[0][~_on([1, 4, 6], G, inst)].any()
    finally:
        ref.close()
        eng.close()


def test_examples_masked_sort_and_equal_run(S):
    """examples/encrypted_sort.py --masked and examples/encrypted_equal.py: encrypt -> one evaluate_circuit call -> decrypt,
    at Params(64); each asserts its own answer."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import encrypted_equal
    import encrypted_sort
    _, boots, inst = encrypted_sort.main(64, 3, 8, 2, masked=True)
    assert (boots, inst) == (2 * 264, 16)
    assert encrypted_equal.main(64, 8, 6)[1] == 6 * 15
