"""Three-input nodes on the device (sgfhe_circuit_create3): k_circ_gather, which stages such a
node as the sum node of three unit weights, (x + y + z, 0), and the XOR3 kernels against the host model -- `circuit.replay_levels` / `replay_ct` / `replay_ct_direct` -- driven by the oracle's
two-input bootstrap on (x + y, z), or by a second ctx's own bootstrap calls, in both flatten modes; decryption
against `evaluate_plain`; lanes with a call boundary inside a level; the ciphertext form refreshed and direct; the
probe; the all-NONE plan against the plain plan; Params(1024).  Every comparison is for equality of every word.

Noise: XOR3 = x + y + z - 2 MAJ is not bootstrapped.  At Params(64) Dr/2 = 128 and a fresh encryption has
|e| <= Dr/8 = 32, a bootstrapped row a few units: three fresh inputs stay below Dr/2, and the random circuit below
feeds an XOR3 wire on only where the sum stays small (checked from the oracle replay with the secret key before
anything is compared)."""

import ctypes

import numpy as np
import pytest

import noise_ref as NR

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(5, 37))
NONE = 0x7FFFFFFE


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


def _oracle_replay(o, bkey, c, inputs, params, rnd_seed=None):
    from sgfhe_jl_amd import circuit as C

    def boot(call, a1, b1, a2, b2):
        if rnd_seed is None:
            return o.bootstrap_batch(bkey, a1, b1, a2, b2)
        return o.bootstrap_batch(bkey, a1, b1, a2, b2, rnd=(rnd_seed, call, np.arange(len(b1), dtype=np.uint32)))
    return C.replay_levels(c, inputs, params.r, boot)


def _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain):
    got = None
    for key in (None, KEY32):
        what = "randomised" if key else "deterministic"
        _set_mode([eng], key)
        prev, got = got, eng.circuit_run(c, inputs)
        want = _oracle_replay(o, bkey, c, inputs, params, rnd_seed=key)
        assert got.shape == want.shape == (c.n_outputs, inputs.shape[1], params.n + 1)
        assert np.array_equal(got, want), "%s run differs from the oracle composed level by level" % what
        assert np.array_equal(_decrypt(S, params, sk, got), plain), what
    assert not np.array_equal(prev, got)


def test_truth_table_every_not_pattern_p64(S, oc):
    """One level of 8 gate3 nodes, one per NOT pattern, on three inputs; 16 instances cover every bit pattern twice;
    every MAJ, ONE_OR_TWO and XOR3 wire is an output."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 301)
    c = S.Circuit(3)
    x, y, z = c.inputs
    outs = []
    for pat in range(8):
        outs.extend(c.gate3(~x if pat & 1 else x, ~y if pat & 2 else y, ~z if pat & 4 else z))
    c.output(*outs)
    assert c.info() == dict(levels=1, nodes=8, widest=8, slots=27)
    inst = 16
    bits = np.array([[(t >> i) & 1 for t in range(inst)] for i in range(3)], dtype=bool)
    plain = c.evaluate_plain(bits)
    s = bits.sum(axis=0)
    assert np.array_equal(plain[0], s >= 2) and np.array_equal(plain[1], (s == 1) | (s == 2)) and \
        np.array_equal(plain[2], s % 2 == 1)
    inputs = _encrypt(o, sk, bits, 302)
    _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain)
    eng.close()


def _mixed_circuit(S, seed):
    """4 inputs, 60 nodes, two- and three-input nodes sharing levels.  Wire classes: RAW (a circuit input: a fresh
    encryption), CLEAN (a bootstrapped row -- AND / OR / XOR, MAJ, ONE_OR_TWO -- or a constant) and X3 (an XOR3 wire,
    which carries its node's input errors on).  An X3 wire is fed on only when its own node had at most one RAW input
    and no X3 input, and then only together with CLEAN wires; the third input is sometimes FALSE or TRUE, so MAJ
    degenerates to AND or OR.  Outputs: one wire of every node, so that all 60 are live -- XOR3 and MAJ wires of the
    three-input nodes in turn, every third one negated."""
    rng = np.random.default_rng(seed)
    c = S.Circuit(4)
    raw, clean, x3 = list(c.inputs), [S.Circuit.FALSE, S.Circuit.TRUE], []
    outs = []

    def some(pool, recent=18):
        w = pool[len(pool) - 1 - int(rng.integers(min(recent, len(pool))))]
        return ~w if rng.integers(2) else w

    def clean_gate():
        return some(clean) if len(clean) > 2 and rng.integers(8) else some(raw)

    for g in range(60):
        kind = int(rng.integers(10))
        if kind < 3:                                              # a two-input node
            ins = [some(raw) if rng.integers(3) == 0 else clean_gate() for _ in range(2)]
            clean.extend(c.gate(*ins))
            outs.append(clean[-1 - g % 3])
            continue
        if x3 and kind < 5:                                       # an X3 wire with CLEAN company
            ins = [some(x3, 6), some(clean), some(clean)]
        elif kind < 7:                                            # at most one RAW input: its XOR3 may be fed on
            ins = [some(raw), some(clean), some(clean)]
        else:                                                     # anything RAW or CLEAN; XOR3 goes to the outputs only
            ins = [some(raw) if rng.integers(2) else some(clean) for _ in range(3)]
        order = rng.permutation(3)
        ins = [ins[k] for k in order]
        if kind in (5, 9):                                        # a constant third input: AND / OR / XOR, or OR / NAND / XNOR
            ins[2] = S.Circuit.TRUE if rng.integers(2) else S.Circuit.FALSE
        maj, one, xor3 = c.gate3(*ins)
        clean.extend([maj, one])
        n_raw = sum(w.id < c.n_inputs for w in ins)
        if n_raw <= 1 and not any(w.id in {v.id for v in x3} for w in ins):
            x3.append(xor3)
        outs.append(xor3 if len(outs) % 2 else maj)
    c.output(*[~w if i % 3 == 0 else w for i, w in enumerate(outs)])
    return c


def _input_sum_errors(S, o, bkey, sk, params, c, inputs, bits):
    """Per node of `c`: the largest |error| of the SUM of its inputs, from the oracle replay (deterministic) of a
    circuit with the same nodes whose outputs are every node's input references."""
    d = S.Circuit(c.n_inputs, group=c.group)
    refs = []
    for g, (gate, shifts) in enumerate(zip(c.gates, c.gate_shifts)):
        ws = [S.Wire(ref, sh) for ref, sh in zip(gate, shifts)]
        (d.gate3 if len(ws) == 3 else d.gate)(*ws)
        refs.extend((g, w) for w in ws)
    d.output(*[w for _, w in refs])
    lwes = _oracle_replay(o, bkey, d, inputs, params)
    plain = d.evaluate_plain(bits).astype(np.int64)
    worst = {}
    for g in range(c.n_gates):
        idx = [i for i, (h, _) in enumerate(refs) if h == g]
        total = lwes[idx].sum(axis=0, dtype=np.uint64) & np.uint64(params.r - 1)
        s = plain[idx].sum(axis=0)
        ph = NR.phases_zr(params, sk, total).astype(np.int64)
        e = (ph - s * params.Dr) % params.r
        e = np.where(e > params.r // 2, e - params.r, e)
        worst[g] = int(np.abs(e).max())
    return worst


def test_mixed_random_circuit_p64_vs_oracle_both_modes(S, oc):
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 311)
    c = _mixed_circuit(S, 312)
    info = c.info()
    three = [g for nodes in c.schedule() for g in nodes if len(c.gates[g]) == 3]
    two = [g for nodes in c.schedule() for g in nodes if len(c.gates[g]) == 2]
    assert info["nodes"] == 60 and info["levels"] >= 4 and len(three) >= 20 and len(two) >= 8
    assert any(len({len(c.gates[g]) for g in nodes}) == 2 for nodes in c.schedule())          # both kinds in one level
    assert any(len(c.gates[g]) == 3 and (c.gates[g][2] & 0x7FFFFFFF) == 0x7FFFFFFF for g in three)
    xor3_ids = {c.n_inputs + 3 * g + 2 for g in three}
    assert any((ref & 0x7FFFFFFF) in xor3_ids for g in three + two for ref in c.gates[g])       # an XOR3 wire is fed on
    maj_ids = {c.n_inputs + 3 * g for g in three}
    for ids in (xor3_ids, maj_ids):                                                             # negated outputs on both
        assert any(ref & 0x80000000 and (ref & 0x7FFFFFFF) in ids for ref in c.outputs)
    inst = 3
    bits = np.random.default_rng(313).integers(0, 2, size=(4, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 314)
    # the condition on the inputs, checked first: every node's input-sum error is below Dr/2
    worst = _input_sum_errors(S, o, bkey, sk, params, c, inputs, bits)
    print("largest input-sum error per node kind: three-input %d, two-input %d, against Dr/2 = %d"
          % (max(worst[g] for g in three), max(worst[g] for g in two), params.Dr // 2))
    assert max(worst.values()) < params.Dr // 2, worst
    plain = c.evaluate_plain(bits)
    assert 0 < plain.sum() < plain.size
    _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain)
    eng.close()


def test_lanes_third_input_shifted_call_boundary_randomised(S, oc):
    """G = 8 over 2736 = 342 * 8 instances; one level of 3 three-input nodes = 8208 rows: call 0 ends at row 8192 =
    node 2, instance 2720 (lane 0 of its group), call 1 holds the other 16 rows.  Third inputs shifted by -1 and +7.
    Sampled rows of each call match the oracle at (call, row - first row of the call)."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 321)
    n, r = params.n, params.r
    G, inst = 8, 2736
    c = S.Circuit(3, group=G)
    x, y, z = c.inputs
    nodes = [(x, y, z.lane(-1)), (~x, y.lane(1), ~z.lane(7)), (x.lane(-7), ~y, z.lane(-1))]
    c.output(*[w for ins in nodes for w in c.gate3(*ins)])
    assert c.info() == dict(levels=1, nodes=3, widest=3, slots=12)
    assert 3 * inst == 8208 and (C.CALL_ROWS - 2 * inst) % G == 0
    bits = np.random.default_rng(322).integers(0, 2, size=(3, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 323)
    eng.set_random_flatten(True, 4321)
    got = eng.circuit_run(c, inputs)
    assert np.array_equal(_decrypt(S, params, sk, got), c.evaluate_plain(bits))

    def val(w):      # the referenced LWEs of every instance: lane shift, FALSE fill, then NOT
        v = C.lane_shift(inputs[w.id], w.shift, G)
        return C.lwe_not(v, r) if w.negated else v

    vals = [[val(w) for w in ins] for ins in nodes]
    mask = np.uint64(r - 1)
    samples = ((0, [0, 1, 7, 8, 2735, 2736, 2737, 2743, 5471, 5472, 5479, 8184, 8191]),
               (1, [8192, 8193, 8199, 8200, 8207]))
    for call, rows in samples:
        rows = np.array(rows)
        assert np.all(rows // C.CALL_ROWS == call)
        rank, t = rows // inst, rows % inst
        X = np.stack([vals[k][0][i] for k, i in zip(rank, t)])
        Y = np.stack([vals[k][1][i] for k, i in zip(rank, t)])
        Z = np.stack([vals[k][2][i] for k, i in zip(rank, t)])
        a = (X + Y) & mask
        ref = o.bootstrap_batch(bkey, a[:, :n], a[:, n], Z[:, :n], Z[:, n],
                                rnd=(4321, call, (rows - call * C.CALL_ROWS).astype(np.uint32)))
        for j, (k, i) in enumerate(zip(rank, t)):
            what = "row %d (call %d)" % (rows[j], call)
            assert np.array_equal(got[3 * k, i], ref[j, 0]), "MAJ, " + what
            assert np.array_equal(got[3 * k + 1, i], ref[j, 1]), "ONE_OR_TWO, " + what
            assert np.array_equal(got[3 * k + 2, i], (a[j] + Z[j] - np.uint64(2) * ref[j, 0]) & mask), "XOR3, " + what
    eng.close()


def test_ripple_adder_ciphertext_form_refreshed_and_direct(S, oc):
    """ripple_adder(4) with N = n, one block: 4 levels of one node, 5 output ciphertexts.  Refreshed against replay_ct,
    direct against replay_ct_direct; out_lwe of the direct run is that of the flags = 0 run; the carry-out (MAJ) is
    direct and the four sum bits (XOR3) are refreshed: the direct replay makes 4 level calls and ONE refresh call of
    4 n rows."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, 331, engines=2)
    n, W, blocks = params.n, 4, 1
    c = S.ripple_adder(W)
    rng = np.random.default_rng(332)
    xs, ys = rng.integers(0, 2 ** W, size=blocks * n), rng.integers(0, 2 ** W, size=blocks * n)
    xs[0], ys[0] = 2 ** W - 1, 1
    xs[1], ys[1] = 2 ** W - 1, 2 ** W - 1
    bits = np.array([(xs >> i) & 1 for i in range(W)] + [(ys >> i) & 1 for i in range(W)], dtype=bool).reshape(2 * W, blocks, n)
    plain = c.evaluate_plain(bits.reshape(2 * W, -1))
    a, b = _encrypt_cts(S, params, sk, bits, 333)

    def total(dec):
        return (dec.astype(np.int64) << np.arange(W + 1)[:, None]).sum(axis=0)

    for key in (None, KEY32):
        what = "randomised" if key else "deterministic"
        _set_mode([eng, ref], key)
        (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
        (rw, rv), rlwe = C.replay_ct(c, a, b, params, lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2),
                                     lambda call, pa, pb: ref.pack_encrypted_bits(pa, pb))
        assert np.array_equal(lwe, rlwe), "out_lwe differs from replay_ct (%s)" % what
        assert np.array_equal(w, rw) and np.array_equal(v, rv), "(w, v) differ from replay_ct (%s)" % what
        dec = _decrypt_ct(S, params, sk, w, v)
        assert np.array_equal(dec, plain) and np.array_equal(_decrypt(S, params, sk, lwe), plain)
        assert np.array_equal(total(dec), xs + ys), what
        _set_mode([eng, ref], key)
        (dw, dv), dlwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True)
        assert np.array_equal(dlwe, lwe), "direct out_lwe differs from the flags = 0 run (%s)" % what
        raw_calls, tails = [], []

        def boot_raw(call, a1, b1, a2, b2):
            raw_calls.append(len(b1))
            return ref.bootstrap_batch(a1, b1, a2, b2, raw=True)

        def tail(call, group):
            tails.append(len(group))
            return ref.pack_lwe_modq(group)

        (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, boot_raw, tail)
        assert raw_calls == [n] * W + [W * n] and tails == [W + 1]       # 4 sum bits refreshed, the carry-out direct
        assert np.array_equal(rlwe, lwe)
        assert np.array_equal(dw, rw) and np.array_equal(dv, rv), "(w, v) differ from replay_ct_direct (%s)" % what
        assert not np.array_equal(dw[W], w[W])                            # the carry-out took the other path
        assert np.array_equal(total(_decrypt_ct(S, params, sk, dw, dv)), xs + ys), what
    eng.close()
    ref.close()


def _probe_circuit(S):
    """Level 1: two three-input nodes and a two-input node on the fresh inputs; level 2: a three-input node on
    bootstrapped wires and a constant-third-input node."""
    c = S.Circuit(3)
    x, y, z = c.inputs
    n0 = c.gate3(x, y, z)
    n1 = c.gate3(~x, y, ~z)
    n2 = c.gate(x, z)
    n3 = c.gate3(n0[0], ~n1[1], n2[2])
    n4 = c.gate3(n0[2], n2[0], S.Circuit.TRUE)
    c.output(n3[2], ~n4[0], n1[2], n4[2])
    return c, (0, 1)            # the nodes whose three inputs are fresh encryptions


def test_probe_records_of_a_gate3_run(S, oc):
    """The records of sgfhe_circuit_run_probe equal tests/noise_ref.py on the rows of a second run that outputs every
    wire; the XOR3 wires of nodes on fresh inputs show a larger max |e| than any MAJ wire, and no row is wrong."""
    params, o, sk, bkey, (A, B) = _setup64(S, oc, 341, engines=2)
    c, fresh = _probe_circuit(S)
    d = S.Circuit(c.n_inputs)
    for gate in c.gates:
        (d.gate3 if len(gate) == 3 else d.gate)(*[S.Wire(ref) for ref in gate])
    wires = list(range(c.n_inputs + 3 * c.n_gates))
    d.output(*[S.Wire(w) for w in wires])
    assert d.schedule() == c.schedule() == [[0, 1, 2], [3, 4]]
    inst = 24
    bits = np.random.default_rng(342).integers(0, 2, size=(3, inst)).astype(np.uint8)
    inputs = _encrypt(o, sk, bits, 343)
    for key in (None, KEY32):
        _set_mode([A, B], key)
        out, stats = A.circuit_probe(c, inputs, sk, bits)
        assert np.array_equal(out, B.circuit_run(c, inputs))
        _set_mode([B], key)
        lwes = B.circuit_run(d, inputs)
        plain = d.evaluate_plain(bits)
        assert len(stats) == len(wires)
        for w, rows, exp in zip(wires, lwes, plain):
            assert stats[w] == S.NoiseStats(*NR.record_zr(params, sk, rows, exp)), w
            assert stats[w].rows == inst and stats[w].wrong == 0, w
        maj = [stats[c.n_inputs + 3 * g].max_abs for g in range(c.n_gates) if len(c.gates[g]) == 3]
        xor3 = [stats[c.n_inputs + 3 * g + 2].max_abs for g in fresh]
        print("max |e|: inputs %s, MAJ %s, XOR3 of the nodes on fresh inputs %s, Dr/2 = %d"
              % ([stats[i].max_abs for i in range(3)], maj, xor3, params.Dr // 2))
        assert min(xor3) > max(maj)
    kinds = {d_["wire"]: d_["kind"] for d_ in S.noise_report(c, stats)}
    assert kinds[3] == "MAJ" and kinds[4] == "ONE_OR_TWO" and kinds[5] == "XOR3" and kinds[9] == "AND" and kinds[0] == "input"
    A.close()
    B.close()


def test_all_none_create3_plan_runs_the_plain_plan_bytes(S, oc):
    """A sgfhe_circuit_create3 plan with every third reference SGFHE_CIRCUIT_NONE gives the bytes of the
    sgfhe_circuit_create plan of the same arrays, in both modes."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 351)
    r2 = np.random.default_rng(352)
    plain_c = S.Circuit(3)
    wires = list(plain_c.inputs) + [S.Circuit.FALSE]
    for g in range(12):
        x, y = (wires[int(r2.integers(len(wires)))] for _ in range(2))
        wires.extend(plain_c.gate(~x if g & 1 else x, ~y if g & 2 else y))
    plain_c.output(wires[-1], ~wires[-2], wires[-6], plain_c.inputs[0], ~plain_c.inputs[1], S.Circuit.TRUE, wires[8])
    none_c = S.Circuit(3)
    none_c.gates, none_c.gate_shifts = list(plain_c.gates), list(plain_c.gate_shifts)
    none_c.outputs, none_c.output_shifts = list(plain_c.outputs), list(plain_c.output_shifts)
    L = S.lib()
    g3 = np.ascontiguousarray(np.array([g + (NONE,) for g in plain_c.gates], dtype=np.uint32))
    s3 = np.ascontiguousarray(np.array([(0, 0, 5 - g) for g in range(12)], dtype=np.int32))       # ignored beside NONE
    outs = np.ascontiguousarray(np.array(plain_c.outputs, dtype=np.uint32))
    h = ctypes.c_void_p()
    vp = lambda a_: a_.ctypes.data_as(ctypes.c_void_p)
    assert L.sgfhe_circuit_create3(3, vp(g3), vp(s3), 12, vp(outs), None, len(outs), 1, ctypes.byref(h)) == 0
    none_c._L, none_c._plan = L, h                                   # (freed with the object, like its own plan)
    assert none_c.info() == plain_c.info()
    inst = 16
    bits = np.random.default_rng(353).integers(0, 2, size=(3, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 354)
    for key in (None, KEY32):
        _set_mode([eng], key)
        a = eng.circuit_run(plain_c, inputs)
        _set_mode([eng], key)
        b = eng.circuit_run(none_c, inputs)
        assert a.tobytes() == b.tobytes(), "randomised" if key else "deterministic"
    assert np.array_equal(_decrypt(S, params, sk, a), plain_c.evaluate_plain(bits))
    eng.close()


def test_ripple_adder_p1024_decrypts_to_the_sums(S, oc):
    """ripple_adder(4) over 8 instances at Params(1024): the five output bits decrypt to x + y.  The ctx is this
    test's own: the session's shared engines are left as they are."""
    params = S.Params(1024)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(363)
    eng = S.Engine(params)
    eng.generate_key(sk, 364)
    W, inst = 4, 8
    c = S.ripple_adder(W)
    xs = np.array([15, 15, 0, 9, 6, 7, 8, 5])
    ys = np.array([1, 15, 0, 6, 9, 1, 8, 10])
    plain = np.array([(xs >> i) & 1 for i in range(W)] + [(ys >> i) & 1 for i in range(W)], dtype=bool)
    inputs = _encrypt(o, sk, plain, 362)
    try:
        got = eng.circuit_run(c, inputs)
        dec = _decrypt(S, params, sk, got).astype(np.int64)
        assert np.array_equal((dec << np.arange(W + 1)[:, None]).sum(axis=0), xs + ys)
    finally:
        eng.close()
