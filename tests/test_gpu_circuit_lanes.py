"""Lane-shifted wire references on the device (sgfhe_circuit_create_lanes): the lane kernels
against the host model -- `circuit.replay_levels` / `replay_ct` / `replay_ct_direct`, which apply the shifts in numpy
-- driven by the oracle or by a second ctx's own bootstrap calls, in both flatten modes; a call boundary inside a
group; the zero-shift lanes plan against the plain plan; the ciphertext form with the packed adder; the probe; the
new error cases; Params(1024).  Every comparison is for equality of every word."""

import ctypes
import os
import sys

import numpy as np
import pytest

import noise_ref as NR

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(3, 35))
SENTINEL = 0xA5A5A5A5A5A5A5A5
ERR_INVALID_ARG = -1
DIRECT = 1      # SGFHE_CIRCUIT_PACK_DIRECT


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


def _encrypt(o, sk, bits, seed):
    """bits [n_inputs][instances] -> the array form [n_inputs][instances][n + 1]."""
    bits = np.asarray(bits, dtype=np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits.reshape(-1), seed)
    return np.concatenate([a, b[:, None]], axis=1).reshape(bits.shape + (a.shape[1] + 1,))


def _encrypt_cts(S, params, sk, bits, seed):
    """bits [n_inputs][blocks][n] -> rlwe (a, b): one PackedCiphertext per (input, block)."""
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


def _decrypt(S, params, sk, words):
    n = params.n
    return S.host.decrypt_lwe(params, sk, words[..., :n], words[..., n]).reshape(words.shape[:-1])


def _decrypt_ct(S, params, sk, w, v):
    """(w, v) [outputs][blocks][m] -> bits [outputs][blocks * n]."""
    return np.stack([np.concatenate([S.host.decrypt_rlwe(params, sk, w[o, t], v[o, t]) for t in range(w.shape[1])])
                     for o in range(w.shape[0])])


def _set_mode(engines, key):
    for e in engines:
        e.set_random_flatten(key is not None, key or 0)      # (the call counter starts again at 0)


def _random_lanes_circuit(S, seed=11):
    """4 inputs, 10 nodes, G = 8: every gate input carries a shift from {0, +-1, +-7, other} and every NOT pattern
    comes up; the outputs keep every node live and are shifted and negated themselves.  With lanes 0 and 7 and
    d = +-7 a reference keeps exactly one lane of a group."""
    rng = np.random.default_rng(seed)
    G = 8
    c = S.Circuit(4, group=G)
    wires = list(c.inputs)
    shifts = [0, 1, -1, 7, -7]

    def pick(k):
        w = S.Circuit.FALSE if rng.integers(16) == 0 else wires[len(wires) - 1 - int(rng.integers(min(9, len(wires))))]
        d = shifts[k % 6] if k % 6 < 5 else int(rng.integers(2, 7)) * (1 if rng.integers(2) else -1)
        return w.lane(d)

    k = 0
    for g in range(10):
        x, y = pick(k), pick(k + 3)
        k += 1
        wires.extend(c.gate(~x if g & 1 else x, ~y if g & 2 else y))
    gate_wires = wires[4:]
    outs = [gate_wires[3 * g + int(rng.integers(3))] for g in range(10)]              # one wire of every node
    outs = [w.lane(shifts[i % 5]) for i, w in enumerate(outs)]
    outs[1], outs[4] = ~outs[1], ~outs[4]
    c.output(*(outs + [c.inputs[0].lane(7), ~c.inputs[1].lane(-7), S.Circuit.TRUE.lane(3), c.inputs[2]]))
    assert c.info()["nodes"] == 10 and c.info()["levels"] >= 3
    used = {d for pair in c.gate_shifts for d in pair}
    assert {0, 1, -1, 7, -7} <= used and len(used) > 5
    return c


def _oracle_replay(o, bkey, c, inputs, params, rnd_seed=None):
    from sgfhe_jl_amd import circuit as C

    def boot(call, a1, b1, a2, b2):
        if rnd_seed is None:
            return o.bootstrap_batch(bkey, a1, b1, a2, b2)
        return o.bootstrap_batch(bkey, a1, b1, a2, b2, rnd=(rnd_seed, call, np.arange(len(b1), dtype=np.uint32)))
    return C.replay_levels(c, inputs, params.r, boot)


def test_random_lanes_circuit_p64_vs_oracle_both_modes(S, oc):
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 201)
    c = _random_lanes_circuit(S)
    inst = 24
    bits = np.random.default_rng(202).integers(0, 2, size=(4, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 203)
    plain = c.evaluate_plain(bits)
    assert 0 < plain.sum() < plain.size
    got = None
    for key in (None, KEY32):
        _set_mode([eng], key)
        prev, got = got, eng.circuit_run(c, inputs)
        want = _oracle_replay(o, bkey, c, inputs, params, rnd_seed=key)
        assert got.shape == want.shape == (c.n_outputs, inst, params.n + 1)
        assert np.array_equal(got, want), "%s run differs from the oracle composed level by level" % \
            ("randomised" if key else "deterministic")
        assert np.array_equal(_decrypt(S, params, sk, got), plain)
    assert not np.array_equal(prev, got)
    eng.close()


def test_call_boundary_inside_a_group_randomised(S, oc):
    """G = 48 over 2736 = 57 * 48 instances.  Level 1 has 3 nodes = 8208 rows: call 0 ends at row 8192 = node 2,
    instance 2720 = lane 32 of its group, call 1 holds the other 16 rows.  Level 2 reads .lane(-47) and .lane(+1) of
    level-1 wires, the second across that boundary; against replay_levels through bootstrap_batch on a clone."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 211)
    ref = eng.clone()
    G, inst = 48, 2736
    c = S.Circuit(2, group=G)
    x, y = c.inputs
    n0, n1, n2 = c.gate(x, y), c.gate(~x, y), c.gate(x, ~y.lane(5))
    top = c.gate(n0[2].lane(-47), ~n2[1].lane(1))
    c.output(top[0], top[2], n1[0].lane(-1), n2[2])
    info = c.info()
    assert (info["levels"], info["nodes"], info["widest"]) == (2, 4, 3)
    assert 3 * inst == 8208 and (C.CALL_ROWS - 2 * inst) % G == 32
    bits = np.random.default_rng(212).integers(0, 2, size=(2, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 213)
    _set_mode([eng, ref], KEY32)
    got = eng.circuit_run(c, inputs)
    calls = []

    def boot(call, a1, b1, a2, b2):
        calls.append(len(b1))
        return ref.bootstrap_batch(a1, b1, a2, b2)
    want = C.replay_levels(c, inputs, params.r, boot)
    assert calls == [8192, 16, inst]
    assert np.array_equal(got, want)
    assert np.array_equal(_decrypt(S, params, sk, got), c.evaluate_plain(bits))
    ref.close()
    eng.close()


def test_zero_shift_lanes_plan_equals_the_plain_plan(S, oc):
    """The same arrays through sgfhe_circuit_create and through sgfhe_circuit_create_lanes(group = 8, NULL shifts):
    the lane kernels with every shift 0 write the bytes of the old kernels, in both modes."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 221)
    rng = np.random.default_rng(222)
    plain_c, lanes_c = S.Circuit(3), S.Circuit(3, group=8)
    for c in (plain_c, lanes_c):
        r2 = np.random.default_rng(223)
        wires = list(c.inputs) + [S.Circuit.FALSE]
        for g in range(12):
            x, y = (wires[int(r2.integers(len(wires)))] for _ in range(2))
            wires.extend(c.gate(~x if g & 1 else x, ~y if g & 2 else y))
        c.output(wires[-1], ~wires[-2], wires[-6], c.inputs[0], ~c.inputs[1], S.Circuit.TRUE, wires[8])
    assert plain_c.gates == lanes_c.gates and plain_c.outputs == lanes_c.outputs
    L = S.lib()
    grp = ctypes.c_uint32()
    assert L.sgfhe_circuit_group(plain_c.handle(), ctypes.byref(grp)) == 0 and grp.value == 1
    assert L.sgfhe_circuit_group(lanes_c.handle(), ctypes.byref(grp)) == 0 and grp.value == 8
    inst = 16
    bits = rng.integers(0, 2, size=(3, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 224)
    for key in (None, KEY32):
        _set_mode([eng], key)
        a = eng.circuit_run(plain_c, inputs)
        _set_mode([eng], key)
        b = eng.circuit_run(lanes_c, inputs)
        assert a.tobytes() == b.tobytes(), "randomised" if key else "deterministic"
    assert np.array_equal(_decrypt(S, params, sk, a), plain_c.evaluate_plain(bits))
    eng.close()


def _word_bits(vals, width):
    return np.array([(int(v) >> i) & 1 for v in vals for i in range(width)], dtype=bool)


def test_packed_adder_ciphertext_form(S, oc):
    """packed_adder(16) at n = 64: 4 words per ciphertext, 2 blocks.  Outputs: the sum (an unshifted gate wire: direct),
    the same wire .lane(+1) and a negated input .lane(-15) (both refreshed under SGFHE_CIRCUIT_PACK_DIRECT)."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, 231, engines=2)
    n, W, blocks = params.n, 16, 2
    c = C.packed_adder(W)
    total = S.Wire(c.outputs[0])
    assert total.id >= c.n_inputs and c.output_shifts[0] == 0
    c.output(total, total.lane(1), ~c.inputs[0].lane(-15))
    words = blocks * n // W
    rng = np.random.default_rng(232)
    xs, ys = rng.integers(0, 2 ** W, size=words), rng.integers(0, 2 ** W, size=words)
    xs[0], ys[0] = 2 ** W - 1, 1
    bits = np.stack([_word_bits(xs, W), _word_bits(ys, W)]).reshape(2, blocks, n)
    plain = c.evaluate_plain(bits.reshape(2, -1))
    a_n, b_n = _encrypt_cts(S, params, sk, bits, 233)
    ident = S.Circuit(2)
    ident.output(*ident.inputs)
    a_m, b_m = eng.circuit_run_ct(ident, a_n, b_n)               # the same bits as Ciphertexts (N = m)
    assert a_m.shape == (2, blocks, params.m)

    def sums(dec):
        return (dec[0].reshape(words, W).astype(np.int64) << np.arange(W)).sum(axis=1)

    boot = lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2)
    pack = lambda call, pa, pb: ref.pack_encrypted_bits(pa, pb)
    for a, b in ((a_n, b_n), (a_m, b_m)):
        for key in (None, KEY32):
            what = "N = %d, %s" % (a.shape[2], "randomised" if key else "deterministic")
            _set_mode([eng, ref], key)
            (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
            (rw, rv), rlwe = C.replay_ct(c, a, b, params, boot, pack)
            assert np.array_equal(lwe, rlwe), "out_lwe differs from replay_ct (%s)" % what
            assert np.array_equal(w, rw) and np.array_equal(v, rv), "(w, v) differ from replay_ct (%s)" % what
            dec = _decrypt_ct(S, params, sk, w, v)
            assert np.array_equal(dec, plain) and np.array_equal(_decrypt(S, params, sk, lwe), plain)
            assert np.array_equal(sums(dec), (xs + ys) % 2 ** W), what
            # direct: out_lwe of the flags = 0 run; the shifted and the input outputs refreshed
            _set_mode([eng, ref], key)
            (dw, dv), dlwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True)
            assert np.array_equal(dlwe, lwe), "direct out_lwe differs from the flags = 0 run (%s)" % what
            (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params,
                                                lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2, raw=True),
                                                lambda call, group: ref.pack_lwe_modq(group))
            assert np.array_equal(rlwe, lwe)
            assert np.array_equal(dw, rw) and np.array_equal(dv, rv), "(w, v) differ from replay_ct_direct (%s)" % what
            assert not np.array_equal(dw[0], w[0])
            assert np.array_equal(_decrypt_ct(S, params, sk, dw, dv), plain)
    eng.close()
    ref.close()


def _all_wires_circuit(S, c):
    """The same nodes and shifts with every input and every wire of every live node as an unshifted output."""
    live = sorted(g for nodes in c.schedule() for g in nodes)
    d = S.Circuit(c.n_inputs, group=c.group)
    for (x, y), (dx, dy) in zip(c.gates, c.gate_shifts):
        d.gate(S.Wire(x, dx), S.Wire(y, dy))
    wires = list(range(c.n_inputs)) + [c.n_inputs + 3 * g + w for g in live for w in range(3)]
    d.output(*[S.Wire(w) for w in wires])
    assert d.schedule() == c.schedule()
    return d, wires


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_probe_of_a_lanes_circuit(S, oc, mode):
    key = KEY32 if mode == "randomised" else None
    params, o, sk, bkey, (A, B) = _setup64(S, oc, 241, engines=2)
    c = _random_lanes_circuit(S)
    d, wires = _all_wires_circuit(S, c)
    inst = 24
    bits = np.random.default_rng(242).integers(0, 2, size=(4, inst)).astype(np.uint8)
    inputs = _encrypt(o, sk, bits, 243)
    _set_mode([A, B], key)
    out, stats = A.circuit_probe(c, inputs, sk, bits)
    assert np.array_equal(out, B.circuit_run(c, inputs))
    _set_mode([B], key)
    lwes = B.circuit_run(d, inputs)
    plain = d.evaluate_plain(bits)
    assert len(stats) == c.n_inputs + 3 * c.n_gates and len(wires) == len(stats)      # (every node is live)
    for w, rows, exp in zip(wires, lwes, plain):
        assert stats[w] == S.NoiseStats(*NR.record_zr(params, sk, rows, exp)), w
        assert stats[w].rows == inst and stats[w].wrong == 0, w
    A.close()
    B.close()


def test_lanes_errors_leave_the_outputs_untouched(S, oc):
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 251)
    n, m = params.n, params.m
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    # instances = 20 with G = 8
    c = _random_lanes_circuit(S)
    bits = np.random.default_rng(252).integers(0, 2, size=(4, 24)).astype(bool)
    inputs = _encrypt(o, sk, bits, 253)
    short = np.ascontiguousarray(inputs[:, :20])
    out = np.full((c.n_outputs, 20, n + 1), SENTINEL, dtype=np.uint64)
    assert L.sgfhe_circuit_run(eng._h, c.handle(), 20, ptr(short), ptr(out)) == ERR_INVALID_ARG
    stats = np.full((c.n_inputs + 3 * c.n_gates, 8), SENTINEL, dtype=np.uint64)
    sk64 = np.ascontiguousarray(sk, dtype=np.uint64)
    b8 = np.ascontiguousarray(bits[:, :20].astype(np.uint8))
    assert L.sgfhe_circuit_run_probe(eng._h, c.handle(), 20, ptr(short), ptr(out), ptr(sk64), ptr(b8),
                                     ptr(stats)) == ERR_INVALID_ARG
    assert np.all(out == SENTINEL) and np.all(stats == SENTINEL)
    with pytest.raises(S.SgfheError) as ei:
        eng.circuit_run(c, short)
    assert ei.value.code == ERR_INVALID_ARG
    # the ciphertext form with G = 48 at n = 64: a group would straddle two ciphertexts
    c48 = S.Circuit(1, group=48)
    g = c48.gate(c48.inputs[0], c48.inputs[0].lane(1))
    c48.output(g[0])
    cb = np.random.default_rng(254).integers(0, 2, size=(1, 3, n)).astype(bool)       # 192 instances = 4 groups of 48
    a, b = _encrypt_cts(S, params, sk, cb, 255)
    ow = np.full((1, 3, m), SENTINEL, dtype=np.uint64)
    ov, ol = ow.copy(), np.full((1, 3 * n, n + 1), SENTINEL, dtype=np.uint64)
    for flags in (0, DIRECT):
        assert L.sgfhe_circuit_run_ct_ex(eng._h, c48.handle(), 3, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol),
                                         flags) == ERR_INVALID_ARG
    assert L.sgfhe_circuit_run_ct(eng._h, c48.handle(), 3, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol)) == ERR_INVALID_ARG
    assert np.all(ow == SENTINEL) and np.all(ov == SENTINEL) and np.all(ol == SENTINEL)
    # correct runs on the same ctx afterwards: the LWE form of both circuits, and G = 16 in the ciphertext form
    got = eng.circuit_run(c, inputs)
    assert np.array_equal(_decrypt(S, params, sk, got), c.evaluate_plain(bits))
    lwe48 = _encrypt(o, sk, cb.reshape(1, -1), 256)
    assert np.array_equal(_decrypt(S, params, sk, eng.circuit_run(c48, lwe48)), c48.evaluate_plain(cb.reshape(1, -1)))
    c16 = S.Circuit(1, group=16)
    g = c16.gate(c16.inputs[0], c16.inputs[0].lane(1))
    c16.output(g[0])
    w, v = eng.circuit_run_ct(c16, a, b)
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), c16.evaluate_plain(cb.reshape(1, -1)))
    eng.close()


def test_packed_adder_p1024_vs_replayed_levels(S, oc):
    """packed_adder(16) over 64 instances (4 words) at Params(1024), both modes: every output word equals the same
    levels replayed through Engine.bootstrap_batch on a second ctx sharing the key; the outputs decrypt to the sums.
    The two ctxs are this test's own (a ctx and its clone): the session's shared engines are left as they are."""
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(263)
    eng = S.Engine(params)
    eng.generate_key(sk, 264)
    ref = eng.clone()
    W, inst = 16, 64
    c = C.packed_adder(W)
    rng = np.random.default_rng(261)
    xs, ys = rng.integers(0, 2 ** W, size=inst // W), rng.integers(0, 2 ** W, size=inst // W)
    xs[0], ys[0] = 2 ** W - 1, 1
    plain = np.stack([_word_bits(xs, W), _word_bits(ys, W)])
    inputs = _encrypt(o, sk, plain, 262)
    try:
        for key in (None, bytes(range(32))):
            _set_mode([eng, ref], key)
            got = eng.circuit_run(c, inputs)
            want = C.replay_levels(c, inputs, params.r, lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2))
            assert np.array_equal(got, want), "mode %s" % ("randomised" if key else "deterministic")
            dec = _decrypt(S, params, sk, got).astype(np.int64).reshape(2, inst // W, W)
            assert np.array_equal((dec[0] << np.arange(W)).sum(axis=1), (xs + ys) % 2 ** W)
            assert np.array_equal(dec[1, :, W - 1], (xs + ys) >> W)
    finally:
        ref.close()
        eng.close()


def test_example_packed_adder_ct_runs(S):
    """examples/packed_adder_ct.py: encrypt -> one evaluate_circuit_ct call -> decrypt, 4 words of 16 bits per
    ciphertext at Params(64), two blocks, refreshed and direct."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import packed_adder_ct
    packed_adder_ct.main(64, 2)
    packed_adder_ct.main(64, 1, direct=True)
