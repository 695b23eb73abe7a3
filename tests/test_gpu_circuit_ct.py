"""Gate circuits on RLWE ciphertexts (sgfhe_circuit_run_ct): split_ciphertext and
pack_encrypted_bits on the device inside the circuit run, against the C oracle, against the same run composed
on the host through a second ctx (circuit.replay_ct), in both flatten modes; the pack stage wider than one call;
ciphertexts of length m fed back in; a Params(1024) adder; edge cases."""

import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(1, 33))
SENTINEL = 0xA5A5A5A5A5A5A5A5


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


def _encrypt_cts(S, params, sk, bits, seed):
    """bits [n_inputs][blocks][n] -> rlwe (a, b), each [n_inputs][blocks][n]: one PackedCiphertext per (input,
    block), _encrypt_private (src/fhe.jl:310-328) with its draws from a numpy Generator."""
    rng = np.random.default_rng(seed)
    bits = np.asarray(bits, dtype=np.uint8)
    a = np.zeros(bits.shape, dtype=np.uint64)
    b = np.zeros(bits.shape, dtype=np.uint64)
    wr = params.Dr // 8
    for i in range(bits.shape[0]):
        for t in range(bits.shape[1]):
            u = rng.integers(0, 2, size=params.n).astype(np.uint8)
            w = rng.integers(-wr, wr + 1, size=params.n).astype(np.int64)
            a[i, t], b[i, t] = S.host.encrypt_private(params, sk, u, w, bits[i, t])
    return a, b


def _host_split(S, params, a, b):
    """[n_inputs][blocks][N] -> [n_inputs][blocks * n][n + 1] through sgfhe_host_split_ciphertext."""
    n = params.n
    out = np.zeros((a.shape[0], a.shape[1] * n, n + 1), dtype=np.uint64)
    for i in range(a.shape[0]):
        for t in range(a.shape[1]):
            la, lb = S.host.split_ciphertext(params, a[i, t], b[i, t])
            out[i, t * n:(t + 1) * n, :n], out[i, t * n:(t + 1) * n, n] = la, lb
    return out


def _decrypt_lwe(S, params, sk, words):
    n = params.n
    return S.host.decrypt_lwe(params, sk, words[..., :n], words[..., n]).reshape(words.shape[:-1])


def _decrypt_ct(S, params, sk, w, v):
    """(w, v) [outputs][blocks][m] -> bits [outputs][blocks * n]."""
    return np.stack([np.concatenate([S.host.decrypt_rlwe(params, sk, w[o, t], v[o, t]) for t in range(w.shape[1])])
                     for o in range(w.shape[0])])


def _random_circuit(S, rng, n_inputs, n_gates, gate_outputs_only=False):
    """The generator of tests/test_gpu_circuit.py: every NOT pattern on node inputs, both constants, mostly recent
    wires as inputs so that the circuit is deep; outputs on raw / negated inputs, constants and (negated) gate
    wires -- or on gate wires alone."""
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
        nots = g % 4
        x, y = (~pick[0] if nots & 1 else pick[0]), (~pick[1] if nots & 2 else pick[1])
        wires.extend(c.gate(x, y))
    outs = [wires[-1], ~wires[-2], wires[-6], ~wires[-9]]
    if not gate_outputs_only:
        outs += [c.inputs[0], ~c.inputs[1], S.Circuit.FALSE, S.Circuit.TRUE]
    outs += [wires[n_inputs + int(rng.integers(len(wires) - n_inputs))] for _ in range(4)]
    c.output(*outs)
    return c


def _set_mode(engines, key):
    for e in engines:
        e.set_random_flatten(key is not None, key or 0)      # (the call counter starts again at 0)


def _replay(S, c, a, b, params, ref):
    from sgfhe_jl_amd import circuit as C
    return C.replay_ct(c, a, b, params, lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2),
                       lambda call, pa, pb: ref.pack_encrypted_bits(pa, pb))


def test_identity_split_pack_vs_oracle_both_modes(S, oc):
    """test/api.test.jl:86-108: encrypt -> split_ciphertext -> pack_encrypted_bits -> decrypt, as one circuit run
    whose outputs are its inputs (one of them negated) and both constants; two blocks."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 51)
    n, m, r = params.n, params.m, params.r
    c = S.Circuit(2)
    x, y = c.inputs
    c.output(x, ~y, S.Circuit.FALSE, S.Circuit.TRUE)
    blocks = 2
    bits = np.random.default_rng(52).integers(0, 2, size=(2, blocks, n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 53)
    lwes = _host_split(S, params, a, b)
    true = np.zeros((blocks * n, n + 1), dtype=np.uint64)
    true[:, n] = r // 4
    want_lwe = [lwes[0], C.lwe_not(lwes[1], r), np.zeros_like(true), true]
    want_bits = [bits[0].reshape(-1), ~bits[1].reshape(-1), np.zeros(blocks * n, bool), np.ones(blocks * n, bool)]
    for key in (None, KEY32):
        _set_mode([eng], key)
        w, v = eng.circuit_run_ct(c, a, b)
        assert w.shape == v.shape == (4, blocks, m)
        for out in range(4):
            for t in range(blocks):
                g = want_lwe[out][t * n:(t + 1) * n]
                q = out * blocks + t                      # no level: the one pack call is call 0, ciphertext q
                rw, rv = o.pack_encrypted_bits(bkey, g[:, :n], g[:, n], rnd=(key, q, 0) if key else None)
                assert np.array_equal(w[out, t], rw) and np.array_equal(v[out, t], rv), \
                    "output %d block %d, %s" % (out, t, "randomised" if key else "deterministic")
        assert np.array_equal(_decrypt_ct(S, params, sk, w, v), np.stack(want_bits))
    # the scheme-level call: PackedCiphertexts in, Ciphertexts out
    bk = S.BootstrapKey.from_canonical(params, bkey, engine=eng)
    cts = [[S.PackedCiphertext(params, S.RLWE(a[i, t], b[i, t])) for t in range(blocks)] for i in range(2)]
    outs = S.evaluate_circuit_ct(bk, None, c, cts)
    assert len(outs) == 4 and all(len(row) == blocks and isinstance(row[0], S.Ciphertext) for row in outs)
    skey = S.PrivateKey.__new__(S.PrivateKey)
    skey.params, skey.key = params, sk
    assert np.array_equal(S.decrypt(skey, outs[1][1]), ~bits[1, 1])
    eng.close()


def _deep_run(S, oc, seed):
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, seed, engines=2)
    rng = np.random.default_rng(seed + 2)
    c = _random_circuit(S, rng, 6, 150)
    blocks = 3
    bits = rng.integers(0, 2, size=(6, blocks, params.n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, seed + 3)
    return params, o, sk, bkey, eng, ref, c, blocks, bits, a, b


def test_random_deep_circuit_vs_replay_both_modes(S, oc):
    params, o, sk, bkey, eng, ref, c, blocks, bits, a, b = _deep_run(S, oc, 61)
    n = params.n
    info = c.info()
    assert info["levels"] > 10 and info["nodes"] > 60
    plain = c.evaluate_plain(bits.reshape(6, -1))
    split = _host_split(S, params, a, b)
    first = None
    for key in (None, KEY32):
        _set_mode([eng, ref], key)
        (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
        (rw, rv), rlwe = _replay(S, c, a, b, params, ref)
        mode = "randomised" if key else "deterministic"
        assert np.array_equal(lwe, rlwe), "LWE outputs differ from the composition (%s)" % mode
        assert np.array_equal(w, rw) and np.array_equal(v, rv), "packed outputs differ from the composition (%s)" % mode
        _set_mode([ref], key)
        assert np.array_equal(lwe, ref.circuit_run(c, split)), "out_lwe differs from circuit_run on the host split"
        assert np.array_equal(_decrypt_lwe(S, params, sk, lwe), plain)
        assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
        if first is None:
            first = w
        else:
            assert not np.array_equal(first, w)
    eng.close()
    ref.close()


def test_pack_stage_wider_than_one_call_randomised(S, oc):
    """70 outputs x 2 blocks = 140 ciphertexts = pack calls of 128 and 12 at Params(64), after the L level calls:
    ciphertexts 0, 127, 128 and 139 against the oracle at (call, ct) = (L, 0), (L, 127), (L + 1, 0), (L + 1, 11)."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 71)
    n = params.n
    c = S.Circuit(2)
    x, y = c.inputs
    g1 = c.gate(x, y)
    g2 = c.gate(g1[0], ~g1[2])
    c.output(*([g2[0], g2[1], ~g2[2], x, S.Circuit.TRUE] * 14))
    assert c.n_outputs == 70 and c.info()["levels"] == 2
    blocks, L = 2, 2                                     # two levels of 128 rows: level calls 0 and 1
    bits = np.random.default_rng(72).integers(0, 2, size=(2, blocks, n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 73)
    eng.set_random_flatten(True, KEY32)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
    plain = c.evaluate_plain(bits.reshape(2, -1))
    assert np.array_equal(_decrypt_lwe(S, params, sk, lwe), plain)
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    for q, call, ct in ((0, L, 0), (127, L, 127), (128, L + 1, 0), (139, L + 1, 11)):
        out, t = q // blocks, q % blocks
        g = lwe[out, t * n:(t + 1) * n]
        rw, rv = o.pack_encrypted_bits(bkey, g[:, :n], g[:, n], rnd=(KEY32, ct, call))
        assert np.array_equal(w[out, t], rw) and np.array_equal(v[out, t], rv), "ciphertext %d" % q
    eng.close()


def test_ciphertexts_of_length_m_and_chaining(S, oc):
    """The (w, v) of a run (N = m) as the inputs of the next: the device split of a Ciphertext equals
    sgfhe_host_split_ciphertext, and a second circuit on them equals the composition and decrypts.  The second
    circuit's outputs are gate wires: every packed bit has been through a bootstrap since the last pack, the flow
    of docs/src/manual.md:119-121,190-192."""
    params, o, sk, bkey, eng, ref, c, blocks, bits, a, b = _deep_run(S, oc, 81)
    n = params.n
    plain1 = c.evaluate_plain(bits.reshape(6, -1))
    w, v = eng.circuit_run_ct(c, a, b)
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain1)
    ident = S.Circuit(c.n_outputs)
    ident.output(*ident.inputs)
    got = eng.circuit_run_ct(ident, w, v, packed=False, lwe=True)
    assert np.array_equal(got, _host_split(S, params, w, v)), "device split of N = m ciphertexts"
    c2 = _random_circuit(S, np.random.default_rng(83), c.n_outputs, 40, gate_outputs_only=True)
    plain2 = c2.evaluate_plain(plain1)
    for key in (None, KEY32):
        _set_mode([eng, ref], key)
        (w2, v2), lwe2 = eng.circuit_run_ct(c2, w, v, packed=True, lwe=True)
        (rw, rv), rlwe = _replay(S, c2, w, v, params, ref)
        assert np.array_equal(lwe2, rlwe) and np.array_equal(w2, rw) and np.array_equal(v2, rv)
        assert np.array_equal(_decrypt_lwe(S, params, sk, lwe2), plain2)
        assert np.array_equal(_decrypt_ct(S, params, sk, w2, v2), plain2)
    eng.close()
    ref.close()


def test_adder_p1024_ciphertexts_in_and_out(S, oc, gpu_keys):
    """A 4-bit adder over one block (1024 instances) at Params(1024), both modes: bytes equal the composition
    through a second ctx on the same key; the sums decrypt to x + y from the packed outputs alone."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import encrypted_adder
    params, o, sk, eng = gpu_keys.engine(1024)
    ref = eng.clone()
    nbits, inst = 4, params.n
    c = encrypted_adder.adder_circuit(S, nbits)
    rng = np.random.default_rng(91)
    xs, ys = rng.integers(0, 16, size=inst), rng.integers(0, 16, size=inst)
    plain = np.array([(xs >> i) & 1 for i in range(nbits)] + [(ys >> i) & 1 for i in range(nbits)])
    a, b = _encrypt_cts(S, params, sk, plain[:, None, :], 92)
    try:
        for key in (None, KEY32):
            _set_mode([eng, ref], key)
            w, v = eng.circuit_run_ct(c, a, b)
            (rw, rv), _ = _replay(S, c, a, b, params, ref)
            assert np.array_equal(w, rw) and np.array_equal(v, rv), "mode %s" % ("randomised" if key else "deterministic")
            dec = _decrypt_ct(S, params, sk, w, v).astype(np.int64)
            assert np.array_equal(sum(dec[i] << i for i in range(nbits + 1)), xs + ys)
    finally:
        ref.close()
        eng.set_random_flatten(False)


def test_edge_cases(S, oc):
    params, o, sk, bkey, (eng, fresh) = _setup64(S, oc, 95, engines=2)
    n, m = params.n, params.m
    L = S.lib()
    rng = np.random.default_rng(96)
    c = _random_circuit(S, rng, 4, 30)
    blocks = 2
    bits = rng.integers(0, 2, size=(4, blocks, n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 97)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    # blocks = 0: nothing to do
    w0, v0 = eng.circuit_run_ct(c, np.zeros((4, 0, n), np.uint64), np.zeros((4, 0, n), np.uint64))
    assert w0.shape == v0.shape == (c.n_outputs, 0, m)
    # a ctx without a key: SGFHE_ERR_NO_KEY, nothing written
    nokey = S.Engine(params)
    ow = np.full((c.n_outputs, blocks, m), SENTINEL, dtype=np.uint64)
    ov, ol = ow.copy(), np.full((c.n_outputs, blocks * n, n + 1), SENTINEL, dtype=np.uint64)
    rc = L.sgfhe_circuit_run_ct(nokey._h, c.handle(), blocks, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol))
    assert rc == -5 and np.all(ow == SENTINEL) and np.all(ov == SENTINEL) and np.all(ol == SENTINEL)
    with pytest.raises(S.SgfheError):
        nokey.circuit_run_ct(c, a, b)
    nokey.close()
    # N neither n nor m; no output form; out_w without out_v (and the other way round): nothing written
    assert L.sgfhe_circuit_run_ct(eng._h, c.handle(), blocks, ptr(a), ptr(b), 2 * n, ptr(ow), ptr(ov), ptr(ol)) == -1
    assert L.sgfhe_circuit_run_ct(eng._h, c.handle(), blocks, ptr(a), ptr(b), n, None, None, None) == -1
    assert L.sgfhe_circuit_run_ct(eng._h, c.handle(), blocks, ptr(a), ptr(b), n, ptr(ow), None, None) == -1
    assert L.sgfhe_circuit_run_ct(eng._h, c.handle(), blocks, ptr(a), ptr(b), n, None, ptr(ov), ptr(ol)) == -1
    assert L.sgfhe_circuit_run_ct(eng._h, c.handle(), blocks, None, ptr(b), n, ptr(ow), ptr(ov), ptr(ol)) == -1
    assert np.all(ow == SENTINEL) and np.all(ov == SENTINEL) and np.all(ol == SENTINEL)
    with pytest.raises(ValueError):
        eng.circuit_run_ct(c, a, b, packed=False, lwe=False)
    with pytest.raises(ValueError):
        eng.circuit_run_ct(c, a[:3], b[:3])
    # sgfhe_pack_encrypted_bits before a ct run, on a ctx that never saw one, and after: the same bytes
    split = _host_split(S, params, a, b)
    pa, pb = split[0, :n, :n][None], split[0, :n, n][None]
    want_pack = fresh.pack_encrypted_bits(pa, pb)
    before = eng.pack_encrypted_bits(pa, pb)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
    after = eng.pack_encrypted_bits(pa, pb)
    for got in (before, after):
        assert np.array_equal(got[0], want_pack[0]) and np.array_equal(got[1], want_pack[1])
    plain = c.evaluate_plain(bits.reshape(4, -1))
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    # each output form alone gives the bytes it has in the run of both
    w1, v1 = eng.circuit_run_ct(c, a, b)
    assert np.array_equal(w1, w) and np.array_equal(v1, v)
    assert np.array_equal(eng.circuit_run_ct(c, a, b, packed=False, lwe=True), lwe)
    # a clone gives the ctx's bytes; release_host_staging between runs changes nothing
    cl = eng.clone()
    wc, vc = cl.circuit_run_ct(c, a, b)
    assert np.array_equal(wc, w) and np.array_equal(vc, v)
    cl.close()
    eng.release_host_staging()
    (w2, v2), lwe2 = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
    assert np.array_equal(w2, w) and np.array_equal(v2, v) and np.array_equal(lwe2, lwe)
    eng.release_host_staging()
    after = eng.pack_encrypted_bits(pa, pb)
    assert np.array_equal(after[0], want_pack[0]) and np.array_equal(after[1], want_pack[1])
    # an LWE-only run consumes exactly the level calls of the draw stream: the next bootstrap_batch is call `levels`
    levels = c.info()["levels"]
    assert c.info()["widest"] * blocks * n <= 8192                       # (one call per level here)
    eng.set_random_flatten(True, KEY32)
    eng.circuit_run_ct(c, a, b, packed=False, lwe=True)
    x, y = split[0, :3], split[1, :3]
    got = eng.bootstrap_batch(x[:, :n], x[:, n], y[:, :n], y[:, n])
    want = o.bootstrap_batch(bkey, x[:, :n], x[:, n], y[:, :n], y[:, n], rnd=(KEY32, levels))
    assert np.array_equal(got, want)
    # ... and a packed run one call more per pack call (here one)
    eng.set_random_flatten(True, KEY32)
    eng.circuit_run_ct(c, a, b)
    got = eng.bootstrap_batch(x[:, :n], x[:, n], y[:, :n], y[:, n])
    want = o.bootstrap_batch(bkey, x[:, :n], x[:, n], y[:, :n], y[:, n], rnd=(KEY32, levels + 1))
    assert np.array_equal(got, want)
    eng.close()
    fresh.close()


def test_example_adder_ct_runs(S):
    """examples/encrypted_adder_ct.py: encrypt -> evaluate_circuit_ct -> decrypt, 4 bits, two blocks at Params(64)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import encrypted_adder_ct
    encrypted_adder_ct.main(4, 64, 2)
