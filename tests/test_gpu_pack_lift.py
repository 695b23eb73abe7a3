"""Packing every circuit output without a refresh bootstrap (sgfhe_lwe_lift_modq, sgfhe_circuit_run_ct_ex with
SGFHE_CIRCUIT_PACK_LIFT): the primitive against `circuit.lift_words`, the run against the host
composition `circuit.replay_ct_direct(lift=True)` on the oracle and on a second ctx, its identity with
circuit_run_ct -> lwe_lift -> pack_lwe_modq on one draw stream, a pack stage wider than one group, lane-shifted
outputs, edge cases, a Params(1024) adder."""

import ctypes

import numpy as np
import pytest

import pack_direct_ref as R
import pack_lift_ref as LR

pytestmark = pytest.mark.gpu

KEY32 = R.KEY32
SENTINEL = 0xA5A5A5A5A5A5A5A5
DIRECT, LIFT = 1, 2      # SGFHE_CIRCUIT_PACK_DIRECT, SGFHE_CIRCUIT_PACK_LIFT (given together: flags = 3)


def _setup64(S, oc, seed, engines=1):
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(seed)
    bkey = o.bootstrap_key(sk, seed + 1)
    engs = []
    for _ in range(engines):
        e = S.Engine(params)
        e.upload_key(bkey)
        engs.append(e)
    return params, o, sk, bkey, engs


def _decrypt_ct(S, params, sk, w, v):
    """(w, v) [outputs][blocks][m] -> bits [outputs][blocks * n]."""
    return np.stack([np.concatenate([S.host.decrypt_rlwe(params, sk, w[o, t], v[o, t]) for t in range(w.shape[1])])
                     for o in range(w.shape[0])])


def _worst_phase(params, sk, w, v, plain, outs):
    n = params.n
    return max(R.phase_error(params, sk, w[o, t], v[o, t], plain[o, t * n:(t + 1) * n])
               for o in outs for t in range(w.shape[1]))


def _set_mode(engines, key):
    for e in engines:
        e.set_random_flatten(key is not None, key or 0)      # (the call counter starts again at 0)


def _engine_replay(c, a, b, params, ref):
    """The lifted run composed from a second ctx's own primitives: un-reduced bootstrap calls, host ModRed and lift,
    sgfhe_pack_lwe_modq (the ctx numbers its calls itself, in the order the composition makes them)."""
    from sgfhe_jl_amd import circuit as C
    return C.replay_ct_direct(c, a, b, params,
                              lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2, raw=True),
                              lambda call, group: ref.pack_lwe_modq(group), lift=True)


def test_lwe_lift_equals_lift_words(S):
    """sgfhe_lwe_lift_modq on 1 row and on 37 rows holding 0, r - 1 and random words; a word equal to r is refused
    before anything is written; no key is needed."""
    from sgfhe_jl_amd import circuit as C
    params = S.Params(64)
    n, r, Q = params.n, params.r, params.Q
    eng = S.Engine(params)
    rng = np.random.default_rng(201)
    for count in (1, 37):
        lwe = rng.integers(0, r, size=(count, n + 1), dtype=np.uint64)
        lwe[0, 0], lwe[-1, n], lwe[count // 2, 1] = 0, r - 1, r - 1
        got = eng.lwe_lift(lwe)
        assert got.shape == (count, n + 1, 2)
        assert np.array_equal(got, C.lift_words(lwe, Q, r))
    assert eng.lwe_lift(np.zeros((0, n + 1), np.uint64)).shape == (0, n + 1, 2)
    assert eng.lwe_lift(lwe.reshape(37, 1, n + 1)).shape == (37, 1, n + 1, 2)
    bad = lwe.copy()
    bad[36, n] = r
    out = np.full((37, n + 1, 2), SENTINEL, dtype=np.uint64)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert S.lib().sgfhe_lwe_lift_modq(eng._h, ptr(bad), 37, ptr(out)) == -1 and np.all(out == SENTINEL)
    assert S.lib().sgfhe_lwe_lift_modq(eng._h, ptr(bad), 0, ptr(out)) == 0 and np.all(out == SENTINEL)
    eng.close()


_ORACLE = {}


def _case64(S, oc, mode):
    """The circuit of the host test over two blocks with crafted inputs, and its oracle replay: once per flatten mode."""
    if mode not in _ORACLE:
        from sgfhe_jl_amd import circuit as C
        key = KEY32 if mode == "randomised" else None
        params, o, sk, bkey, _ = _setup64(S, oc, 211, engines=0)
        n = params.n
        c, lifted = LR.lift_circuit(S)
        bits = np.random.default_rng(212).integers(0, 2, size=(6, 2, n)).astype(bool)
        a, b = LR.craft_cts(S, params, sk, bits, 213)
        bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
        ref = C.replay_ct_direct(c, a, b, params, R.oracle_boot(o, bkey, key), R.oracle_tail(bp, bk, key), lift=True)
        _ORACLE[mode] = (params, sk, bkey, c, lifted, bits, a, b, ref)
    return _ORACLE[mode]


@pytest.mark.parametrize("N", ["n", "m"])
@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_circuit_lift_equals_the_oracle_replay(S, oc, mode, N):
    """ripple_adder(3) with an input, a negated input, TRUE and a negated XOR3 wire as further outputs, two blocks,
    inputs as PackedCiphertext (N = n) and as Ciphertext (N = m, split to the same LWEs): (w, v) word for word the
    oracle replay, out_lwe the bytes of the flags = 0 run, decryption the plain evaluation, and lift=True with
    direct=True the bytes of lift=True alone (both send PACK_DIRECT | PACK_LIFT: the ABI refuses the lift bit alone)."""
    key = KEY32 if mode == "randomised" else None
    params, sk, bkey, c, lifted, bits, a, b, ((rw, rv), rlwe) = _case64(S, oc, mode)
    if N == "m":
        a, b = LR.widen_cts(a, b, params.m, 214)
    eng = S.Engine(params)
    eng.upload_key(bkey)
    plain = c.evaluate_plain(bits.reshape(6, -1))
    _set_mode([eng], key)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, lift=True)
    _set_mode([eng], key)
    (w0, v0), lwe0 = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
    _set_mode([eng], key)
    (w3, v3), lwe3 = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True, lift=True)
    assert np.array_equal(lwe, lwe0), "out_lwe differs from the flags = 0 run (%s)" % mode
    assert np.array_equal(lwe, rlwe)
    assert np.array_equal(w, rw) and np.array_equal(v, rv), "packed outputs differ from the oracle replay (%s)" % mode
    assert np.array_equal(w3, w) and np.array_equal(v3, v) and np.array_equal(lwe3, lwe)
    assert not np.array_equal(w, w0)
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    assert np.array_equal(_decrypt_ct(S, params, sk, w0, v0), plain)
    lo = [o for o in range(c.n_outputs) if lifted[o]]
    print("worst packed phase error, %s, N = %s: lifted %d, refreshed %d, against Dr / 2 = %d"
          % (mode, N, _worst_phase(params, sk, w, v, plain, lo), _worst_phase(params, sk, w0, v0, plain, lo),
             params.Dr // 2))
    eng.close()


def test_lift_run_is_run_then_lift_then_tail_on_one_stream(S, oc):
    """Randomised, a ctx and its clone under the same key: the lifted run on one; on the other circuit_run_ct for the
    LWEs only, lwe_lift, pack_lwe_modq in groups.  The lifted ciphertexts get the same bytes (a direct one is packed
    from its raw rows, other bytes), and the next bootstrap call gives equal bytes: both consumed the same call
    numbers."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 221)
    n = params.n
    cl = eng.clone()
    c, lifted = LR.lift_circuit(S)
    blocks = 2
    bits = np.random.default_rng(222).integers(0, 2, size=(6, blocks, n)).astype(bool)
    a, b = LR.craft_cts(S, params, sk, bits, 223)
    _set_mode([eng, cl], KEY32)
    w, v = eng.circuit_run_ct(c, a, b, lift=True)
    lwe = cl.circuit_run_ct(c, a, b, packed=False, lwe=True)
    groups = lwe.reshape(c.n_outputs * blocks, n, n + 1)
    cw, cv = np.zeros_like(w).reshape(-1, params.m), np.zeros_like(v).reshape(-1, params.m)
    cpc = C.pack_calls(n)
    for q0 in range(0, len(groups), cpc):
        cw[q0:q0 + cpc], cv[q0:q0 + cpc] = cl.pack_lwe_modq(cl.lwe_lift(groups[q0:q0 + cpc]))
    cw, cv = cw.reshape(w.shape), cv.reshape(v.shape)
    for q in range(c.n_outputs):
        same = np.array_equal(w[q], cw[q]) and np.array_equal(v[q], cv[q])
        assert same == lifted[q], "output %d" % q
    plain = c.evaluate_plain(bits.reshape(6, -1))
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    assert np.array_equal(_decrypt_ct(S, params, sk, cw, cv), plain)
    x3, y3 = lwe[0, :3], lwe[3, :3]
    got = eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])
    assert np.array_equal(got, cl.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n]))
    # three level calls and one tail: call number 4
    assert np.array_equal(got, o.bootstrap_batch(bkey, x3[:, :n], x3[:, n], y3[:, :n], y3[:, n], rnd=(KEY32, 4)))
    cl.close()
    eng.close()


def test_pack_stage_wider_than_one_group_randomised(S, oc):
    """7 outputs x 20 blocks = 140 ciphertexts = groups of 128 and 12 at Params(64), direct and lifted ciphertexts
    mixed: outputs 3 and 4 are one run of 40 lifted ciphertexts, and output 6 (ciphertexts 120 .. 139, lifted) is cut
    by the group boundary into a run that ends the first group and one that opens the second.  Against the composition
    on a second ctx."""
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, 231, engines=2)
    n = params.n
    c = S.ripple_adder(3)
    s0, s1, s2, carry = (S.Wire(ref_) for ref_ in c.outputs)
    maj0, maj1 = S.Wire(c.n_inputs), S.Wire(c.n_inputs + 3)
    c.output(s0, carry, ~maj0, c.inputs[0], s1, maj1, ~s2)
    blocks = 20
    assert c.n_outputs * blocks == 140 and c.info()["levels"] == 3
    bits = np.random.default_rng(232).integers(0, 2, size=(6, blocks, n)).astype(bool)
    a, b = LR.craft_cts(S, params, sk, bits, 233)
    _set_mode([eng, ref], KEY32)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, lift=True)
    (rw, rv), rlwe = _engine_replay(c, a, b, params, ref)
    assert np.array_equal(lwe, rlwe)
    assert np.array_equal(w, rw) and np.array_equal(v, rv)
    plain = c.evaluate_plain(bits.reshape(6, -1))
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    # three level calls and two tails: the next call is number 5
    x3, y3 = lwe[1, :3], lwe[5, :3]
    got = eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])
    assert np.array_equal(got, o.bootstrap_batch(bkey, x3[:, :n], x3[:, n], y3[:, :n], y3[:, n], rnd=(KEY32, 5)))
    eng.close()
    ref.close()


def test_lane_shifted_outputs_are_lifted(S, oc):
    """Circuit(2, group=8): a gate wire read one lane down (lane 0 filled with FALSE) and a negated one read seven lanes
    up (every lane but 0 filled with TRUE) are lifted, beside a direct output and a shifted negated input; randomised,
    word for word the oracle replay."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 241)
    n = params.n
    c = S.Circuit(2, group=8)
    x, y = c.inputs
    g = c.gate(x, y)
    c.output(g[0], g[2].lane(-1), (~g[1]).lane(7), (~x).lane(-3))
    bits = np.random.default_rng(242).integers(0, 2, size=(2, 1, n)).astype(bool)
    a, b = LR.craft_cts(S, params, sk, bits, 243)
    _set_mode([eng], KEY32)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, lift=True)
    bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
    (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, R.oracle_boot(o, bkey, KEY32), R.oracle_tail(bp, bk, KEY32),
                                        lift=True)
    assert np.array_equal(lwe, rlwe)
    assert np.array_equal(w, rw) and np.array_equal(v, rv)
    plain = c.evaluate_plain(bits.reshape(2, -1))
    assert plain[2].reshape(-1, 8)[:, 1:].all() and not plain[1].reshape(-1, 8)[:, 0].any()      # the lane fill
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    eng.close()


def test_edge_cases(S, oc):
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 251)
    n, m = params.n, params.m
    L = S.lib()
    c, _ = LR.lift_circuit(S)
    blocks = 2
    bits = np.random.default_rng(252).integers(0, 2, size=(6, blocks, n)).astype(bool)
    a, b = LR.craft_cts(S, params, sk, bits, 253)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    ow = np.full((c.n_outputs, blocks, m), SENTINEL, dtype=np.uint64)
    ov, ol = ow.copy(), np.full((c.n_outputs, blocks * n, n + 1), SENTINEL, dtype=np.uint64)
    untouched = lambda: np.all(ow == SENTINEL) and np.all(ov == SENTINEL) and np.all(ol == SENTINEL)
    # bit 4 and above stay unknown, and so does the lift bit without the direct bit (it was unknown before the flag
    # existed: tests/test_gpu_pack_direct.py)
    for flags in (LIFT, 4, LIFT | 4, DIRECT | LIFT | 4, DIRECT | LIFT | 0x80000000):
        assert L.sgfhe_circuit_run_ct_ex(eng._h, c.handle(), blocks, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol), flags) == -1
    assert untouched()
    # a ctx without a key: the run is refused, the primitive needs none
    nokey = S.Engine(params)
    assert L.sgfhe_circuit_run_ct_ex(nokey._h, c.handle(), blocks, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol), DIRECT | LIFT) == -5
    assert untouched()
    nokey.close()
    # blocks = 0
    w0, v0 = eng.circuit_run_ct(c, np.zeros((6, 0, n), np.uint64), np.zeros((6, 0, n), np.uint64), lift=True)
    assert w0.shape == v0.shape == (c.n_outputs, 0, m)
    # out_w NULL with the flag: the flags = 0 run (the LWE outputs; the level calls of the draw stream and no more)
    want = eng.circuit_run_ct(c, a, b, packed=False, lwe=True)
    assert np.array_equal(eng.circuit_run_ct(c, a, b, packed=False, lwe=True, lift=True), want)
    eng.set_random_flatten(True, KEY32)
    eng.circuit_run_ct(c, a, b, packed=False, lwe=True, lift=True)
    x3, y3 = want[0, :3], want[3, :3]
    got = eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])
    assert np.array_equal(got, o.bootstrap_batch(bkey, x3[:, :n], x3[:, n], y3[:, :n], y3[:, n], rnd=(KEY32, 3)))
    eng.set_random_flatten(False)
    # the other forms of the run are unchanged by a lifted run before them, and a lifted run after
    # release_host_staging gives its bytes again
    refreshed, direct = eng.circuit_run_ct(c, a, b), eng.circuit_run_ct(c, a, b, direct=True)
    w, v = eng.circuit_run_ct(c, a, b, lift=True)
    again, dagain = eng.circuit_run_ct(c, a, b), eng.circuit_run_ct(c, a, b, direct=True)
    assert np.array_equal(again[0], refreshed[0]) and np.array_equal(again[1], refreshed[1])
    assert np.array_equal(dagain[0], direct[0]) and np.array_equal(dagain[1], direct[1])
    eng.release_host_staging()
    w2, v2 = eng.circuit_run_ct(c, a, b, lift=True)
    assert np.array_equal(w2, w) and np.array_equal(v2, v)
    # a circuit without a node: every output is lifted, no bootstrap runs at all
    p = S.Circuit(2)
    p.output(p.inputs[1], ~p.inputs[0], S.Circuit.FALSE)
    pw, pv = eng.circuit_run_ct(p, a[:2], b[:2], lift=True)
    assert np.array_equal(_decrypt_ct(S, params, sk, pw, pv), p.evaluate_plain(bits[:2].reshape(2, -1)))
    eng.close()


def test_adder_p1024_lift(S, oc, gpu_keys):
    """ripple_adder(2) over one block at Params(1024), deterministic, crafted inputs: the two sum bits (XOR3 wires,
    lifted) have the bytes of lwe_lift + pack_lwe_modq of the run's own out_lwe -- in the deterministic mode a
    ciphertext's tail does not depend on its group -- the carry-out is direct (packed from its raw rows, other bytes),
    and all three decrypt."""
    params, o, sk, eng = gpu_keys.engine(1024)
    n = params.n
    c = S.ripple_adder(2)
    rng = np.random.default_rng(261)
    xs, ys = rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    bits = np.array([(xs >> i) & 1 for i in range(2)] + [(ys >> i) & 1 for i in range(2)])
    a, b = LR.craft_cts(S, params, sk, bits[:, None, :], 262)
    try:
        eng.set_random_flatten(False)
        (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, lift=True)
        cw, cv = eng.pack_lwe_modq(eng.lwe_lift(lwe.reshape(3, n, n + 1)))
        assert np.array_equal(w[:2, 0], cw[:2]) and np.array_equal(v[:2, 0], cv[:2])
        dec = _decrypt_ct(S, params, sk, w, v).astype(np.int64)
        assert np.array_equal(sum(dec[i] << i for i in range(3)), xs + ys)
        assert np.array_equal(S.host.decrypt_rlwe(params, sk, cw[2], cv[2]), dec[2].astype(bool))
        plain = c.evaluate_plain(bits)
        print("worst packed phase error at Params(1024): sum bits %d, carry %d, against Dr / 2 = %d"
              % (_worst_phase(params, sk, w, v, plain, (0, 1)), _worst_phase(params, sk, w, v, plain, (2,)),
                 params.Dr // 2))
    finally:
        eng.set_random_flatten(False)
        eng.release_host_staging()
