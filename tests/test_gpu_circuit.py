"""Gate circuits on the device (sgfhe_circuit_run) against the oracle composed level by
level, in both flatten modes; the call-splitting contract of the randomised flatten; a 4-bit adder at
Params(1024) against the same levels replayed through bootstrap_batch on a second ctx; edge cases."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup64(S, oc, seed):
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(seed)
    bkey = o.bootstrap_key(sk, seed + 1)
    bk = S.BootstrapKey.from_canonical(params, bkey)
    return params, o, sk, bkey, bk


def _encrypt(o, sk, bits, seed):
    """bits [n_inputs][instances] -> the array form [n_inputs][instances][n + 1]."""
    bits = np.asarray(bits, dtype=np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits.reshape(-1), seed)
    return np.concatenate([a, b[:, None]], axis=1).reshape(bits.shape + (a.shape[1] + 1,))


def _decrypt(S, params, sk, words):
    n = params.n
    return S.host.decrypt_lwe(params, sk, words[..., :n], words[..., n]).reshape(words.shape[:-1])


def _random_circuit(S, rng, n_inputs, n_gates):
    """Every NOT pattern on node inputs, both constants as inputs, outputs on raw / negated inputs, constants
    and negated gate wires; mostly recent wires as inputs, so that the circuit is deep."""
    c = S.Circuit(n_inputs)
    wires = list(c.inputs)
    for g in range(n_gates):
        pick = []
        for _ in range(2):
            u = rng.integers(20)
            if u == 0:
                w = S.Circuit.FALSE
            elif u < 4 or len(wires) == n_inputs:
                w = wires[int(rng.integers(n_inputs))]
            else:
                w = wires[len(wires) - 1 - int(rng.integers(min(12, len(wires) - n_inputs)))]
            pick.append(w)
        nots = g % 4                                   # all four NOT patterns, in turn
        x, y = (~pick[0] if nots & 1 else pick[0]), (~pick[1] if nots & 2 else pick[1])
        wires.extend(c.gate(x, y))
    outs = [wires[-1], ~wires[-2], wires[-6], ~wires[-9], c.inputs[0], ~c.inputs[1], S.Circuit.FALSE, S.Circuit.TRUE]
    outs += [wires[n_inputs + int(rng.integers(len(wires) - n_inputs))] for _ in range(4)]
    c.output(*outs)
    return c


def _oracle_replay(S, o, bkey, c, inputs, params, rnd_seed=None):
    from sgfhe_jl_amd import circuit as C

    def boot(call, a1, b1, a2, b2):
        if rnd_seed is None:
            return o.bootstrap_batch(bkey, a1, b1, a2, b2)
        return o.bootstrap_batch(bkey, a1, b1, a2, b2, rnd=(rnd_seed, call))
    return C.replay_levels(c, inputs, params.r, boot)


def test_random_circuit_p64_vs_oracle_both_modes(S, oc):
    params, o, sk, bkey, bk = _setup64(S, oc, 41)
    rng = np.random.default_rng(7)
    c = _random_circuit(S, rng, 6, 150)
    info = c.info()
    assert info["levels"] > 10 and info["nodes"] > 60
    inst = 3
    bits = rng.integers(0, 2, size=(6, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 5)
    plain = c.evaluate_plain(bits)
    n = params.n
    # deterministic, EncryptedBit form
    enc = [[S.EncryptedBit(S.LWE(inputs[i, t, :n], inputs[i, t, n])) for t in range(inst)] for i in range(6)]
    outs = S.evaluate_circuit(bk, None, c, enc)
    got = np.array([[np.append(e.lwe.a, e.lwe.b) for e in row] for row in outs], dtype=np.uint64)
    want = _oracle_replay(S, o, bkey, c, inputs, params)
    assert got.shape == want.shape == (c.n_outputs, inst, n + 1)
    assert np.array_equal(got, want), "deterministic circuit differs from the oracle composed level by level"
    assert np.array_equal(_decrypt(S, params, sk, got), plain)
    # randomised, array form: the key of the draw stream is the first 32 bytes of the Generator
    got_r = S.evaluate_circuit(bk, np.random.default_rng(99), c, inputs)
    want_r = _oracle_replay(S, o, bkey, c, inputs, params, rnd_seed=np.random.default_rng(99).bytes(32))
    assert np.array_equal(got_r, want_r), "randomised circuit differs from the oracle at its (call, boot) numbers"
    assert not np.array_equal(got_r, got)
    assert np.array_equal(_decrypt(S, params, sk, got_r), plain)
    bk.engine.close()


def test_level_wider_than_one_call_p64_randomised(S, oc):
    """3 nodes x 3000 instances: one level of 9000 rows = calls 0 (rows 0 .. 8191) and 1 (the other 808).
    Sampled rows of each call match the oracle at (call, row - first row of the call)."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, bk = _setup64(S, oc, 43)
    n = params.n
    c = S.Circuit(2)
    x, y = c.inputs
    outs = [c.gate(x, y)[2], c.gate(~x, y)[0], c.gate(x, ~y)[1]]
    c.output(*outs)
    inst = 3000
    assert c.info() == dict(levels=1, nodes=3, widest=3, slots=5)
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2, size=(2, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 6)
    bk.engine.set_random_flatten(True, 1234)
    got = bk.engine.circuit_run(c, inputs)
    assert np.array_equal(_decrypt(S, params, sk, got), c.evaluate_plain(bits))
    nots = [(False, False, 2), (True, False, 0), (False, True, 1)]     # (NOT x, NOT y, gate) per node
    for call, rows in ((0, [0, 1, 2999, 3000, 5001, 6000, 8191]), (1, [8192, 8193, 8600, 8999])):
        rows = np.array(rows)
        assert np.all(rows // C.CALL_ROWS == call)
        rank, t = rows // inst, rows % inst
        xs = np.stack([C.lwe_not(inputs[0, i], params.r) if nots[k][0] else inputs[0, i] for k, i in zip(rank, t)])
        ys = np.stack([C.lwe_not(inputs[1, i], params.r) if nots[k][1] else inputs[1, i] for k, i in zip(rank, t)])
        ref = o.bootstrap_batch(bkey, xs[:, :n], xs[:, n], ys[:, :n], ys[:, n],
                                rnd=(1234, call, (rows - call * C.CALL_ROWS).astype(np.uint32)))
        for j, (k, i) in enumerate(zip(rank, t)):
            assert np.array_equal(got[k, i], ref[j, nots[k][2]]), "row %d (call %d)" % (rows[j], call)
    bk.engine.close()


def test_adder_p1024_vs_replayed_levels(S, oc):
    """A 4-bit ripple-carry adder x 64 instances at Params(1024), both modes: every output word equals the
    same levels replayed through Engine.bootstrap_batch on a second ctx holding the same key (same 32 key
    bytes and call numbers in the randomised mode); the sums decrypt to x + y."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import encrypted_adder
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(17)
    eng, ref = S.Engine(params), S.Engine(params)
    eng.generate_key(sk, 18)
    ref.generate_key(sk, 18)
    bits, inst = 4, 64
    c = encrypted_adder.adder_circuit(S, bits)
    rng = np.random.default_rng(19)
    xs, ys = rng.integers(0, 16, size=inst), rng.integers(0, 16, size=inst)
    plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)])
    inputs = _encrypt(o, sk, plain, 20)
    for key in (None, bytes(range(32))):
        for e in (eng, ref):
            e.set_random_flatten(key is not None, key or 0)
        got = eng.circuit_run(c, inputs)
        want = C.replay_levels(c, inputs, params.r, lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2))
        assert np.array_equal(got, want), "mode %s" % ("randomised" if key else "deterministic")
        dec = _decrypt(S, params, sk, got).astype(np.int64)
        assert np.array_equal(sum(dec[i] << i for i in range(bits + 1)), xs + ys)
    eng.close()
    ref.close()


def test_edge_cases(S, oc):
    params, o, sk, bkey, bk = _setup64(S, oc, 45)
    n = params.n
    eng = bk.engine
    rng = np.random.default_rng(3)
    c = _random_circuit(S, rng, 4, 30)
    bits = rng.integers(0, 2, size=(4, 5)).astype(bool)
    inputs = _encrypt(o, sk, bits, 8)
    # instances = 0: nothing to do
    empty = eng.circuit_run(c, np.zeros((4, 0, n + 1), dtype=np.uint64))
    assert empty.shape == (c.n_outputs, 0, n + 1)
    # a ctx without a key: SGFHE_ERR_NO_KEY, nothing written
    nokey = S.Engine(params)
    out = np.full((c.n_outputs, 5, n + 1), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = S.lib().sgfhe_circuit_run(nokey._h, c.handle(), 5, inputs.ctypes.data_as(ctypes.c_void_p),
                                   out.ctypes.data_as(ctypes.c_void_p))
    assert rc == -5 and np.all(out == 0xA5A5A5A5A5A5A5A5)
    with pytest.raises(S.SgfheError):
        nokey.circuit_run(c, inputs)
    nokey.close()
    # one plan on the ctx and two clones: identical bytes; release_host_staging between runs changes nothing
    first = eng.circuit_run(c, inputs)
    assert np.array_equal(_decrypt(S, params, sk, first), c.evaluate_plain(bits))
    clones = [eng.clone(), eng.clone()]
    for cl in clones:
        assert np.array_equal(cl.circuit_run(c, inputs), first)
    eng.release_host_staging()
    assert np.array_equal(eng.circuit_run(c, inputs), first)
    clones[0].release_host_staging()
    assert np.array_equal(clones[0].circuit_run(c, inputs), first)
    for cl in clones:
        cl.close()
    eng.close()
