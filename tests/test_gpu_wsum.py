"""Weighted-sum nodes on the device (sgfhe_circuit_create_w): k_circ_gather and the
XOR3 kernels against the host model -- `circuit.replay_levels` / `replay_ct` / `replay_ct_direct` -- driven by the
oracle's two-input bootstrap on (U, FALSE), or by a second ctx's own bootstrap calls, in both flatten modes; decryption
against `evaluate_plain`; lanes with a call boundary inside a level; fan-in 64; the ciphertext form refreshed, direct and
lifted; the probe; the old entry points; Params(1024).  Every comparison is for equality of every word.

Noise: a node is correct while the error of its input sum stays below Dr/2 (128 at Params(64)), and a weight of 2
doubles a wire's error.  A fresh encryption has |e| <= Dr/8 = 32 here and a bootstrapped row a few units, so the
circuits below give weight 2 to bootstrapped rows only; the random circuit's condition is checked from the oracle
replay with the secret key before anything is compared."""

import ctypes
import itertools
import os

import numpy as np
import pytest

import expect
import noise_ref as NR
import pack_direct_ref as R
import pack_lift_ref as LR
import wsum_ref as WR

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(7, 39))


@pytest.fixture(scope="module")
def wexp(exp):
    """Recorded oracle digests of this file's one expensive comparison (tests/expect.py), in a table of its own."""
    X = expect.Expect(path=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpu_expect_wsum.json"))
    yield X
    X.save()


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


def _oracle_boot(o, bkey, rnd_seed=None):
    """The oracle's bootstrap for replay_levels, on its NTT-domain key (the same bytes, faster)."""
    from conftest import oracle_threads
    T = oracle_threads()
    khat = expect.Lazy(lambda: o.key_transform(bkey, threads=T))

    def boot(call, a1, b1, a2, b2):
        if rnd_seed is None:
            return o.bootstrap_batch(khat(), a1, b1, a2, b2, opt=True, threads=T)
        return o.bootstrap_batch(khat(), a1, b1, a2, b2, opt=True, threads=T,
                                 rnd=(rnd_seed, call, np.arange(len(b1), dtype=np.uint32)))
    return boot


def _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain):
    from sgfhe_jl_amd import circuit as C
    got = None
    for key in (None, KEY32):
        what = "randomised" if key else "deterministic"
        _set_mode([eng], key)
        prev, got = got, eng.circuit_run(c, inputs)
        want = C.replay_levels(c, inputs, params.r, _oracle_boot(o, bkey, key))
        assert got.shape == want.shape == (c.n_outputs, inputs.shape[1], params.n + 1)
        assert np.array_equal(got, want), "%s run differs from the oracle composed level by level" % what
        assert np.array_equal(_decrypt(S, params, sk, got), plain), what
    assert not np.array_equal(prev, got)


def truth_table_circuit(S):
    """Three inputs refreshed, then one sum node per weight tuple in {-2, -1, 1, 2}^k, k = 1, 2, 3, on the refreshed
    wires, the NOT pattern going round with the node's number; every HI, MID and LOW wire is an output."""
    c = S.Circuit(3)
    fresh = [c.refresh(w) for w in c.inputs]
    outs, tuples = [], []
    for k in (1, 2, 3):
        for weights in itertools.product([-2, -1, 1, 2], repeat=k):
            pat = len(tuples) % 8
            terms = [(w, ~fresh[i] if pat >> i & 1 else fresh[i]) for i, w in enumerate(weights)]
            outs.extend(c.sum_node(terms))
            tuples.append((weights, pat))
    c.output(*outs)
    return c, tuples


def test_truth_table_every_weight_tuple_p64(S, oc):
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 501)
    c, tuples = truth_table_circuit(S)
    assert len(tuples) == 84 and c.has_wsum and c.info()["nodes"] == 87 and c.info()["levels"] == 2
    bits = np.array([[0, 1, 1, 0, 1], [0, 1, 0, 1, 1], [0, 1, 0, 0, 1]], dtype=bool)      # 5 instances
    bits[2, 4] = 0
    plain = c.evaluate_plain(bits)
    for j, (weights, pat) in enumerate(tuples):
        vals = [bits[i] ^ bool(pat >> i & 1) for i in range(len(weights))]
        assert all(np.array_equal(p, q) for p, q in zip(plain[3 * j:3 * j + 3], WR.sum_node_model(weights, vals)))
    inputs = _encrypt(o, sk, bits, 502)
    _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain)
    eng.close()


def test_unit_weight_sum_node_gives_the_bytes_of_gate3(S, oc):
    """(1, x), (1, y), (1, z) against gate3(x, y, z), on all three wires in both modes: as a plan of its own (it takes
    sgfhe_circuit_create3) and inside a plan that holds a sum node of another shape as well."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 511)
    a = S.Circuit(3)
    x, y, z = a.inputs
    ins = (x, ~y, z)
    a.output(*a.gate3(*ins))
    b = S.Circuit(3)
    b.output(*b.sum_node([(1, w) for w in b.inputs[:1] + [~b.inputs[1], b.inputs[2]]]))
    w = S.Circuit(3)
    unit = w.sum_node([(1, w.inputs[0]), (1, ~w.inputs[1]), (1, w.inputs[2])])
    w.output(*(unit + (w.refresh(w.inputs[0]),)))
    assert not a.has_wsum and not b.has_wsum and w.has_wsum and ins
    inst = 16
    bits = np.array([[(t >> i) & 1 for t in range(inst)] for i in range(3)], dtype=bool)
    inputs = _encrypt(o, sk, bits, 512)
    for key in (None, KEY32):
        outs = []
        for c in (a, b, w):
            _set_mode([eng], key)
            outs.append(eng.circuit_run(c, inputs))
        assert outs[0].tobytes() == outs[1].tobytes(), "create3 route"
        assert outs[0].tobytes() == outs[2][:3].tobytes(), "create_w route"
        assert np.array_equal(_decrypt(S, params, sk, outs[2]), w.evaluate_plain(bits))
    eng.close()


def random_circuit(S, seed, n_nodes=60):
    """4 inputs, `n_nodes` nodes: classic, gate3 and sum nodes of fan-in 1 .. 12 sharing levels, with NOTs and
    constants.  Wire classes: RAW (a circuit input: a fresh encryption), CLEAN (a bootstrapped row -- AND / OR / XOR,
    MAJ, ONE_OR_TWO, HI, MID -- or a constant) and LIN (an XOR3 / LOW wire, which carries its node's input-sum error
    on).  Weight 2 goes to CLEAN terms only; a node takes at most one RAW term, of weight 1, except the classic and
    gate3 nodes on fresh inputs; a LIN wire is fed on, with weight 1 and CLEAN company, only when its own node had CLEAN
    terms alone and a fan-in of at most 4.  Outputs: one wire of every node, so that all are live, every third one
    negated."""
    rng = np.random.default_rng(seed)
    c = S.Circuit(4)
    raw, clean, lin = list(c.inputs), [S.Circuit.FALSE, S.Circuit.TRUE], []
    outs = []

    def some(pool, recent=24):
        w = pool[len(pool) - 1 - int(rng.integers(min(recent, len(pool))))]
        return ~w if rng.integers(2) else w

    for g in range(n_nodes):
        kind = (0, 0, 1, 1, 2, 2, 2, 2, 2, 2)[int(rng.integers(10))] if g >= 6 else g % 3
        if kind == 0:                                             # a classic node
            ws = c.gate(some(raw) if g < 6 or rng.integers(3) == 0 else some(clean), some(clean) if g >= 6 else some(raw))
            clean.extend(ws)
            outs.append(ws[g % 3])
        elif kind == 1:                                           # a three-input node
            ins = [some(raw), some(clean), some(clean)] if g >= 6 else [some(raw) for _ in range(3)]
            maj, one, x3 = c.gate3(*[ins[k] for k in rng.permutation(3)])
            clean.extend([maj, one])
            outs.append(x3 if g % 2 else maj)
        else:                                                     # a sum node
            fan = int(rng.integers(1, 13)) if g >= 6 else 1
            terms, pure = [], True
            if rng.integers(3) == 0 or g < 6:
                terms.append((int(rng.choice([-1, 1])), some(raw)))
                pure = False
            elif lin and rng.integers(3) == 0:
                terms.append((int(rng.choice([-1, 1])), some(lin, 4)))
                pure = False
            while len(terms) < fan:
                terms.append((int(rng.choice([-2, -1, 1, 2])), some(clean)))
            terms = [terms[k] for k in rng.permutation(len(terms))]
            hi, mid, low = c.sum_node(terms)
            clean.extend([hi, mid])
            if pure and fan <= 4:
                lin.append(low)
            outs.append((hi, mid, low)[g % 3])
    c.output(*[~w if i % 3 == 0 else w for i, w in enumerate(outs)])
    return c


def test_random_circuit_70_instances_p64_vs_oracle_both_modes(S, oc, wexp):
    """The oracle's answers -- 4200 bootstraps per mode -- are recorded digests (tests/expect.py: equal SHA-256 is
    equal bytes, and a mismatch falls through to the live oracle).  The deterministic run is of the circuit that also
    outputs every term of every node; once it is known to be the oracle's replay word for word, the condition of the
    noise rule is checked on it with the secret key, before anything else is compared."""
    from sgfhe_jl_amd import circuit as C
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(521)
    bkey = o.bootstrap_key(sk, 522)
    eng = wexp.engine(S, params)
    eng.upload_key(bkey)
    c = random_circuit(S, 522)
    kinds = [c.kind(g) for g in range(c.n_gates)]
    fans = {len(c.gates[g]) for g in range(c.n_gates) if kinds[g] == "sum"}
    assert c.info()["nodes"] == 60 and c.info()["levels"] >= 4 and c.has_wsum
    assert min(kinds.count(k) for k in ("classic", "gate3", "sum")) >= 8 and {1, 12} <= fans and len(fans) >= 8
    assert any(len({kinds[g] for g in nodes}) == 3 for nodes in c.schedule())              # all kinds in one level
    assert any(ref & 0x80000000 for g in range(c.n_gates) if kinds[g] == "sum" for ref in c.gates[g])
    low_ids = {c.n_inputs + 3 * g + 2 for g in range(c.n_gates) if kinds[g] == "sum"}
    assert any((ref & 0x7FFFFFFF) in low_ids for g in range(c.n_gates) for ref in c.gates[g])   # a LOW wire is fed on
    inst, n_out = 70, c.n_outputs
    bits = np.random.default_rng(523).integers(0, 2, size=(4, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 524)
    d, terms = WR.with_term_outputs(S, c, keep_outputs=True)
    assert d.schedule() == c.schedule()
    _set_mode([eng], None)
    det = wexp.check("random522/deterministic", eng.circuit_run(d, inputs),
                     lambda: C.replay_levels(d, inputs, params.r, _oracle_boot(o, bkey)))
    # the condition on the inputs: every node's input-sum error is below Dr/2, no node left out
    worst = WR.sum_errors(params, sk, c.n_gates, terms, det[n_out:], d.evaluate_plain(bits)[n_out:])
    print("largest input-sum error: sum nodes %d, three-input %d, classic %d, against Dr/2 = %d"
          % tuple([max(worst[g] for g in range(c.n_gates) if kinds[g] == k) for k in ("sum", "gate3", "classic")]
                  + [params.Dr // 2]))
    assert len(worst) == 60 and max(worst.values()) < params.Dr // 2, worst
    plain = c.evaluate_plain(bits)
    assert 0 < plain.sum() < plain.size
    assert np.array_equal(_decrypt(S, params, sk, det[:n_out]), plain)
    _set_mode([eng], None)
    own = eng.circuit_run(c, inputs)
    assert wexp.record or own.tobytes() == det[:n_out].tobytes()
    _set_mode([eng], KEY32)
    rnd = wexp.check("random522/randomised", eng.circuit_run(c, inputs),
                     lambda: C.replay_levels(c, inputs, params.r, _oracle_boot(o, bkey, KEY32)))
    assert np.array_equal(_decrypt(S, params, sk, rnd), plain) and not np.array_equal(rnd, det[:n_out])
    eng.close()


def test_lanes_shifted_terms_and_a_call_boundary_randomised(S, oc):
    """G = 8 over 2736 = 342 * 8 instances.  Level 1 refreshes the three inputs and level 2 holds three sum nodes on
    the refreshed wires: each level is 8208 rows, so its first call ends at row 8192 = node 2, instance 2720 (lane 0 of
    its group) and its second holds the other 16 rows -- calls 0, 1 and 2, 3.  Terms shifted by -1 and +7, and a negated
    shifted term of weight 2, whose fill is TRUE.  Sampled rows of every call match the oracle at (call, row - first
    row of the call), level 2 from the device's own level-1 rows."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 531)
    n, r = params.n, params.r
    G, inst = 8, 2736
    c = S.Circuit(3, group=G)
    fx, fy, fz = fresh = [c.refresh(w) for w in c.inputs]
    nodes = [[(2, fx), (1, fy.lane(-1)), (1, fz)],
             [(2, ~fx.lane(7)), (-1, fy), (2, fz.lane(-1)), (1, S.Circuit.TRUE)],
             [(-2, fx.lane(-7)), (1, ~fy.lane(1)), (2, ~fz.lane(-1)), (2, fx), (-1, fz.lane(7))]]
    outs = [w for terms in nodes for w in c.sum_node(terms)]
    c.output(*(fresh + outs))
    assert c.has_wsum and c.info() == dict(levels=2, nodes=6, widest=3, slots=12)
    assert 3 * inst == 8208 and (C.CALL_ROWS - 2 * inst) % G == 0
    bits = np.random.default_rng(532).integers(0, 2, size=(3, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 533)
    eng.set_random_flatten(True, 4321)
    got = eng.circuit_run(c, inputs)
    assert np.array_equal(_decrypt(S, params, sk, got), c.evaluate_plain(bits))

    def val(w):      # the referenced LWEs of every instance: lane shift, FALSE fill, then NOT
        src = np.zeros((inst, n + 1), np.uint64) if w.id == 0x7FFFFFFF else (inputs[w.id] if w.id < 3 else got[(w.id - 3) // 3])
        v = C.lane_shift(src, w.shift, G)
        return C.lwe_not(v, r) if w.negated else v

    def usum(terms):
        return (sum(wt * val(w).astype(np.int64) for wt, w in terms) % r).astype(np.uint64)

    level_u = [[usum([(1, w)]) for w in c.inputs], [usum(terms) for terms in nodes]]
    rows_0 = [0, 1, 7, 8, 2735, 2736, 2737, 2743, 5471, 5472, 5479, 8184, 8191]
    rows_1 = [8192, 8193, 8199, 8200, 8207]
    for level in (0, 1):
        for part, rows in enumerate((rows_0, rows_1)):
            rows = np.array(rows)
            call = 2 * level + part
            rank, t = rows // inst, rows % inst
            U = np.stack([level_u[level][k][i] for k, i in zip(rank, t)])
            Z = np.zeros_like(U)
            ref = o.bootstrap_batch(bkey, U[:, :n], U[:, n], Z[:, :n], Z[:, n],
                                    rnd=(4321, call, (rows - part * C.CALL_ROWS).astype(np.uint32)))
            for j, (k, i) in enumerate(zip(rank, t)):
                what = "level %d row %d (call %d)" % (level + 1, rows[j], call)
                if level == 0:
                    assert np.array_equal(got[k, i], ref[j, 1]), "refresh, " + what
                    continue
                assert np.array_equal(got[3 + 3 * k, i], ref[j, 0]), "HI, " + what
                assert np.array_equal(got[3 + 3 * k + 1, i], ref[j, 1]), "MID, " + what
                assert np.array_equal(got[3 + 3 * k + 2, i], (U[j] - np.uint64(2) * ref[j, 0]) & np.uint64(r - 1)), "LOW, " + what
    eng.close()


def test_fan_in_64(S, oc):
    """Sum nodes of 64 terms, mostly constants and repeated wires whose errors cancel (2 w - 2 w, w - w), around a few
    refreshed wires that count: against the oracle in both modes."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 541)
    c = S.Circuit(4)
    f = [c.refresh(w) for w in c.inputs]
    T, F = S.Circuit.TRUE, S.Circuit.FALSE
    n0 = [(2, f[0]), (-2, f[0])] * 12 + [(1, ~f[1]), (-1, ~f[1])] * 8 + [(1, T)] * 6 + [(2, T)] * 5 + [(-1, F)] * 5 + \
        [(-2, T)] * 4 + [(2, f[0]), (2, f[1]), (2, ~f[2]), (2, f[3])]
    n1 = [(1, f[2]), (2, ~f[3])] + [(2, T), (-2, T)] * 15 + [(1, f[0]), (-1, f[0])] * 15 + [(1, f[1]), (-2, F)]
    assert len(n0) == len(n1) == 64
    c.output(*(c.sum_node(n0) + c.sum_node(n1)))
    inst = 16
    bits = np.array([[(t >> i) & 1 for t in range(inst)] for i in range(4)], dtype=bool)
    plain = c.evaluate_plain(bits)
    s0 = (6 + 10 - 8 + 2 * (bits[0].astype(int) + bits[1] + ~bits[2] + bits[3])) % 4
    assert np.array_equal(plain[0], s0 >= 2) and np.array_equal(plain[0], ~(bits[0] ^ bits[1] ^ bits[2] ^ bits[3]))
    inputs = _encrypt(o, sk, bits, 542)
    _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain)
    eng.close()


def matvec_circuit(S, seed):
    """gf2_matvec of a random 8 x 8 matrix (inputs refreshed), with one more node 2 r0 + r1 whose LOW wire -- the bit
    of input 1, not bootstrapped -- is a ninth output."""
    M = np.random.default_rng(seed).integers(0, 2, size=(8, 8))
    M[3] = [1, 0, 0, 0, 0, 0, 0, 0]
    M[:, 0] |= M[:, 1] == 0                       # (inputs 0 and 1 are used: nodes 0 and 1 refresh them)
    c = S.gf2_matvec(M)
    assert c.n_gates == 16 and c.gates[0] == (0,) and c.gates[1] == (1,)
    r0, r1 = S.Wire(8 + 1), S.Wire(8 + 3 + 1)
    low = c.sum_node([(2, r0), (1, r1)])[2]
    c.output(*([S.Wire(ref) for ref in c.outputs] + [low]))
    return c, M


@pytest.mark.parametrize("N", ["n", "m"])
def test_gf2_matvec_ciphertext_form_refreshed_direct_and_lifted(S, oc, N):
    """Two blocks.  flags = 0 against replay_ct; PACK_DIRECT and PACK_DIRECT | PACK_LIFT against replay_ct_direct on a
    second ctx, with the calls each composition makes: the eight parities are direct, the LOW output is refreshed
    (one call of n rows) or lifted (no call); out_lwe is that of the flags = 0 run."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, 551, engines=2)
    n, blocks = params.n, 2
    c, M = matvec_circuit(S, 552)
    bits = np.random.default_rng(553).integers(0, 2, size=(8, blocks, n)).astype(bool)
    plain = c.evaluate_plain(bits.reshape(8, -1))
    assert np.array_equal(plain[:8], (M @ bits.reshape(8, -1)) % 2 == 1) and np.array_equal(plain[8], bits[1].reshape(-1))
    a, b = LR.craft_cts(S, params, sk, bits, 554)
    if N == "m":
        a, b = LR.widen_cts(a, b, params.m, 555)
    for key in (None, KEY32):
        what = "randomised" if key else "deterministic"
        _set_mode([eng, ref], key)
        (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
        calls = []
        (rw, rv), rlwe = C.replay_ct(c, a, b, params,
                                     lambda call, a1, b1, a2, b2: (calls.append(len(b1)), ref.bootstrap_batch(a1, b1, a2, b2))[1],
                                     lambda call, pa, pb: (calls.append(-len(pb)), ref.pack_encrypted_bits(pa, pb))[1])
        assert calls == [8 * blocks * n, 9 * blocks * n, -9 * blocks]
        assert np.array_equal(lwe, rlwe), "out_lwe differs from replay_ct (%s)" % what
        assert np.array_equal(w, rw) and np.array_equal(v, rv), "(w, v) differ from replay_ct (%s)" % what
        assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain) and np.array_equal(_decrypt(S, params, sk, lwe), plain)
        for lift in (False, True):
            _set_mode([eng, ref], key)
            (dw, dv), dlwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True, lift=lift)
            assert np.array_equal(dlwe, lwe), "direct out_lwe differs from the flags = 0 run (%s)" % what
            raw_calls, tails = [], []

            def boot_raw(call, a1, b1, a2, b2):
                raw_calls.append(len(b1))
                return ref.bootstrap_batch(a1, b1, a2, b2, raw=True)

            def tail(call, group):
                tails.append(len(group))
                return ref.pack_lwe_modq(group)

            (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, boot_raw, tail, lift=lift)
            assert raw_calls == [8 * blocks * n, 9 * blocks * n] + ([] if lift else [blocks * n]) and tails == [9 * blocks]
            assert np.array_equal(rlwe, lwe)
            assert np.array_equal(dw, rw) and np.array_equal(dv, rv), "(w, v) differ from replay_ct_direct (%s, lift %s)" % (what, lift)
            assert not np.array_equal(dw[0], w[0])                        # a parity took the direct path
            assert np.array_equal(_decrypt_ct(S, params, sk, dw, dv), plain), (what, lift)
            print("worst packed phase error (%s, lift %s, N = %s): parities %d, LOW %d, against Dr/2 = %d"
                  % (what, lift, N, max(R.phase_error(params, sk, dw[q, t], dv[q, t], plain[q, t * n:(t + 1) * n])
                                        for q in range(8) for t in range(blocks)),
                     max(R.phase_error(params, sk, dw[8, t], dv[8, t], plain[8, t * n:(t + 1) * n]) for t in range(blocks)),
                     params.Dr // 2))
    eng.close()
    ref.close()


def test_lanes_every_node_kind_and_the_pack_level_through_one_gather(S, oc):
    """G = 8, one block of PackedCiphertexts (64 instances): a classic node and a gate3 on the inputs share level 1, a
    sum node of five terms on their bootstrapped wires -- weights 2, -2, 1, -1, 1, lane shifts -1, +7, +1, -7 -- is
    level 2, and the outputs take every path of the pack stage: a negated, shifted gate wire, the LOW wire, the
    unshifted HI wire (direct), an input wire and TRUE.  Level calls and the pack stage's pseudo-level go through the
    one k_circ_gather.  flags = 0 against replay_ct, PACK_DIRECT and PACK_DIRECT | PACK_LIFT against replay_ct_direct on
    a second ctx with the calls each makes, in both flatten modes; every form decrypts to evaluate_plain.  Inputs are
    crafted with |e| <= Dr/16 = 16, so three of them stay below Dr/2 = 128; every node's input-sum error is measured
    from the replay with the secret key before anything is compared."""
    from sgfhe_jl_amd import circuit as C
    from sgfhe_jl_amd.scheme import split_ciphertext_array
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, 591, engines=2)
    n, G = params.n, 8
    c = S.Circuit(3, group=G)
    x, y, z = c.inputs
    g = c.gate(x, ~y.lane(1))
    m = c.gate3(x, y, z.lane(-1))
    hi, mid, low = c.sum_node([(2, g[0].lane(-1)), (-2, ~g[1].lane(7)), (1, m[0].lane(1)), (-1, m[1].lane(-7)), (1, ~g[2])])
    c.output(~g[1].lane(-1), low, hi, x, S.Circuit.TRUE)
    assert c.has_wsum and c.has_gate3 and c.schedule() == [[0, 1], [2]] and [c.kind(k) for k in range(3)] == ["classic", "gate3", "sum"]
    bits = np.random.default_rng(592).integers(0, 2, size=(3, 1, n)).astype(bool)
    plain = c.evaluate_plain(bits.reshape(3, -1))
    assert all(0 < plain[q].sum() < n for q in range(4)) and plain[4].all()
    a, b = LR.craft_cts(S, params, sk, bits, 593)
    inputs = split_ciphertext_array(a, b, n, params.r).reshape(3, n, n + 1)
    _set_mode([ref], None)
    worst = WR.input_sum_errors(S, params, sk, c, inputs, bits.reshape(3, -1),
                                lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2))
    print("largest input-sum error per node:", worst, "against Dr/2 =", params.Dr // 2)
    assert len(worst) == 3 and max(worst.values()) < params.Dr // 2, worst
    for key in (None, KEY32):
        what = "randomised" if key else "deterministic"
        _set_mode([eng, ref], key)
        (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
        calls = []
        (rw, rv), rlwe = C.replay_ct(c, a, b, params,
                                     lambda call, a1, b1, a2, b2: (calls.append(len(b1)), ref.bootstrap_batch(a1, b1, a2, b2))[1],
                                     lambda call, pa, pb: (calls.append(-len(pb)), ref.pack_encrypted_bits(pa, pb))[1])
        assert calls == [2 * n, n, -5]
        assert np.array_equal(lwe, rlwe), "out_lwe differs from replay_ct (%s)" % what
        assert np.array_equal(w, rw) and np.array_equal(v, rv), "(w, v) differ from replay_ct (%s)" % what
        assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain) and np.array_equal(_decrypt(S, params, sk, lwe), plain)
        for lift in (False, True):
            _set_mode([eng, ref], key)
            (dw, dv), dlwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True, lift=lift)
            assert np.array_equal(dlwe, lwe), "direct out_lwe differs from the flags = 0 run (%s)" % what
            raw_calls, tails = [], []

            def boot_raw(call, a1, b1, a2, b2):
                raw_calls.append(len(b1))
                return ref.bootstrap_batch(a1, b1, a2, b2, raw=True)

            def tail(call, group):
                tails.append(len(group))
                return ref.pack_lwe_modq(group)

            (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, boot_raw, tail, lift=lift)
            assert raw_calls == [2 * n, n] + ([] if lift else [4 * n]) and tails == [5]     # (HI alone is direct)
            assert np.array_equal(rlwe, lwe)
            assert np.array_equal(dw, rw) and np.array_equal(dv, rv), "(w, v) differ from replay_ct_direct (%s, lift %s)" % (what, lift)
            assert not np.array_equal(dw[2], w[2])                        # HI took the direct path
            assert np.array_equal(_decrypt_ct(S, params, sk, dw, dv), plain), (what, lift)
    eng.close()
    ref.close()


def test_probe_records_of_a_sum_node_run(S, oc):
    """The records of sgfhe_circuit_run_probe equal tests/noise_ref.py on the rows of a second run that outputs every
    wire; no row is wrong; the record of a LOW wire is the node's input-sum error (against s mod 2) up to 2 e_HI."""
    params, o, sk, bkey, (A, B) = _setup64(S, oc, 561, engines=2)
    c = S.Circuit(3)
    x, y, z = c.inputs
    f = [c.refresh(w) for w in c.inputs]                               # nodes 0 .. 2
    n3 = c.sum_node([(2, f[0]), (2, ~f[1]), (2, f[2])])                # a parity
    n4 = c.sum_node([(2, f[0]), (1, f[1]), (1, ~f[2])])
    n5 = c.gate(x, z)
    n6 = c.sum_node([(-1, n3[0]), (2, n4[1]), (1, n5[2]), (-2, n4[0]), (1, S.Circuit.TRUE)])
    c.output(n6[2], ~n6[0], n4[2], n3[0], n3[2])
    d, _ = WR.with_term_outputs(S, c)
    wires = list(range(c.n_inputs + 3 * c.n_gates))
    d.output(*[S.Wire(w) for w in wires])
    assert d.schedule() == c.schedule() == [[0, 1, 2, 5], [3, 4], [6]] and c.has_wsum
    inst = 24
    bits = np.random.default_rng(562).integers(0, 2, size=(3, inst)).astype(np.uint8)
    inputs = _encrypt(o, sk, bits, 563)
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
        # LOW of the parity node: U - 2 HI with U = 2 (f0 + ~f1 + f2): its error is the input-sum error less 2 e_HI
        mask = np.uint64(params.r - 1)
        nf1 = (np.uint64(params.r) - lwes[3 + 3 * 1 + 1]) & mask
        nf1[:, params.n] = (nf1[:, params.n] + np.uint64(params.Dr)) & mask
        U = (np.uint64(2) * (lwes[3 + 1] + nf1 + lwes[3 + 3 * 2 + 1])) & mask
        s = 2 * (plain[3 + 1].astype(np.int64) + ~plain[3 + 3 + 1] + plain[3 + 6 + 1])
        e_u = (NR.phases_zr(params, sk, U).astype(np.int64) - s * params.Dr) % params.r
        e_u = np.where(e_u > params.r // 2, e_u - params.r, e_u)
        e_hi = NR.errors_zr(params, sk, lwes[3 + 3 * 3], plain[3 + 3 * 3])
        e_low = NR.errors_zr(params, sk, lwes[3 + 3 * 3 + 2], plain[3 + 3 * 3 + 2])
        assert np.array_equal(e_low, e_u - 2 * e_hi) and stats[3 + 3 * 3 + 2].max_abs == int(np.abs(e_low).max())
        print("max |e|: inputs %s, refreshed %s, parity HI %d, parity LOW %d (input sum %d), Dr/2 = %d"
              % ([stats[i].max_abs for i in range(3)], [stats[3 + 3 * g + 1].max_abs for g in range(3)],
                 stats[3 + 9].max_abs, stats[3 + 11].max_abs, int(np.abs(e_u).max()), params.Dr // 2))
    kinds = {d_["wire"]: d_["kind"] for d_ in S.noise_report(c, stats)}
    assert kinds[3 + 9] == "HI" and kinds[3 + 10] == "MID" and kinds[3 + 11] == "LOW" and kinds[3 + 15] == "AND" and kinds[0] == "input"
    A.close()
    B.close()


def test_plans_without_sum_nodes_keep_their_entry_points_and_bytes(S, oc):
    """A circuit of classic and three-input nodes still takes sgfhe_circuit_create3 and gives the oracle's bytes; the
    same arrays restated through sgfhe_circuit_create_w -- classic nodes classic, three-input nodes three unit weights
    -- give those bytes too."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 571)
    rng = np.random.default_rng(572)
    c = S.Circuit(3)
    wires = list(c.inputs) + [S.Circuit.FALSE]
    for g in range(12):
        ins = [wires[int(rng.integers(min(len(wires), 10)))] for _ in range(3)]
        ins = [~w if rng.integers(2) else w for w in ins]
        new = c.gate3(*ins) if g % 2 else c.gate(*ins[:2])
        wires.extend(new[:2])                                   # (bootstrapped rows only are fed on)
    c.output(wires[-1], ~wires[-2], wires[-6], c.inputs[0], S.Circuit.TRUE, S.Wire(3 + 3 * 11 + 2), S.Wire(3 + 2))
    assert c.has_gate3 and not c.has_wsum and not c.gate_weights
    w = S.Circuit(3)
    w.gates, w.gate_shifts = list(c.gates), list(c.gate_shifts)
    w.outputs, w.output_shifts = list(c.outputs), list(c.output_shifts)
    L = S.lib()
    vp = lambda a_: np.ascontiguousarray(a_).ctypes.data_as(ctypes.c_void_p)
    kind = np.array([len(g) == 3 for g in c.gates], dtype=np.uint32)
    start = np.cumsum([0] + [len(g) for g in c.gates]).astype(np.uint32)
    refs = np.array([r_ for g in c.gates for r_ in g], dtype=np.uint32)
    ones = np.ones(len(refs), dtype=np.int32)
    outs = np.array(c.outputs, dtype=np.uint32)
    h = ctypes.c_void_p()
    assert L.sgfhe_circuit_create_w(3, vp(kind), vp(start), vp(refs), None, vp(ones), 12, vp(outs), None, len(outs), 1,
                                    ctypes.byref(h)) == 0
    w._L, w._plan = L, h                                             # (freed with the object, like its own plan)
    assert w.info() == c.info()
    inst = 16
    bits = np.random.default_rng(573).integers(0, 2, size=(3, inst)).astype(bool)
    inputs = _encrypt(o, sk, bits, 574)
    plain = c.evaluate_plain(bits)
    _both_modes_against_the_oracle(S, o, bkey, sk, params, eng, c, inputs, plain)
    for key in (None, KEY32):
        _set_mode([eng], key)
        x = eng.circuit_run(c, inputs)
        _set_mode([eng], key)
        y = eng.circuit_run(w, inputs)
        assert x.tobytes() == y.tobytes(), "randomised" if key else "deterministic"
    eng.close()


def test_parity_of_8_p1024(S, oc, gpu_keys):
    """Params(1024), 8 instances in the LWE form: 8 refreshes and one 8-term parity, against the levels replayed
    through the engine's own bootstrap_batch; the output decrypts to the parity."""
    from sgfhe_jl_amd import circuit as C
    params, o, sk, eng = gpu_keys.engine(1024)
    c = S.Circuit(8)
    c.output(c.xor(*[c.refresh(w) for w in c.inputs]))
    assert c.has_wsum and c.info() == dict(levels=2, nodes=9, widest=8, slots=c.info()["slots"])
    inst = 8
    bits = np.random.default_rng(581).integers(0, 2, size=(8, inst)).astype(bool)
    bits[:, 0], bits[:, 1] = 0, 1
    inputs = _encrypt(o, sk, bits, 582)
    got = eng.circuit_run(c, inputs)
    want = C.replay_levels(c, inputs, params.r, lambda call, a1, b1, a2, b2: eng.bootstrap_batch(a1, b1, a2, b2))
    assert np.array_equal(got, want)
    assert np.array_equal(_decrypt(S, params, sk, got)[0], np.bitwise_xor.reduce(bits))
