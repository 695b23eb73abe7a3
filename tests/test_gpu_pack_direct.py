"""Packing circuit outputs over Z_Q directly (sgfhe_pack_lwe_modq, sgfhe_circuit_run_ct_ex with
SGFHE_CIRCUIT_PACK_DIRECT): the tail against the big-int oracle in both flatten modes, its
identity with sgfhe_pack_encrypted_bits, the circuit run against the host composition `circuit.replay_ct_direct` on
the oracle and on a second ctx, the pack stage wider than one group, a Params(1024) adder, edge cases."""

import ctypes
import os
import sys

import numpy as np
import pytest

import pack_direct_ref as R

pytestmark = pytest.mark.gpu

KEY32 = R.KEY32
SENTINEL = 0xA5A5A5A5A5A5A5A5
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


def _decrypt_ct(S, params, sk, w, v):
    """(w, v) [outputs][blocks][m] -> bits [outputs][blocks * n]."""
    return np.stack([np.concatenate([S.host.decrypt_rlwe(params, sk, w[o, t], v[o, t]) for t in range(w.shape[1])])
                     for o in range(w.shape[0])])


def _worst_phase(params, sk, w, v, plain):
    n = params.n
    return max(R.phase_error(params, sk, w[o, t], v[o, t], plain[o, t * n:(t + 1) * n])
               for o in range(w.shape[0]) for t in range(w.shape[1]))


def _set_mode(engines, key):
    for e in engines:
        e.set_random_flatten(key is not None, key or 0)      # (the call counter starts again at 0)


def _engine_replay(c, a, b, params, ref):
    """The direct run composed from a second ctx's own primitives: un-reduced bootstrap calls, host ModRed,
    sgfhe_pack_lwe_modq (the ctx numbers its calls itself, in the order the composition makes them)."""
    from sgfhe_jl_amd import circuit as C
    return C.replay_ct_direct(c, a, b, params,
                              lambda call, a1, b1, a2, b2: ref.bootstrap_batch(a1, b1, a2, b2, raw=True),
                              lambda call, group: ref.pack_lwe_modq(group))


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_tail_equals_the_oracle(S, oc, mode):
    """sgfhe_pack_lwe_modq of three ciphertexts -- the un-reduced AND, OR and XOR rows of 192 oracle bootstraps --
    word for word against the big-int tail; randomised: as call 1 of the stream, ciphertext ct drawing with z = ct."""
    key = KEY32 if mode == "randomised" else None
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 101)
    n = params.n
    bits = np.random.default_rng(102).integers(0, 2, size=6 * n).astype(np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits, 103)
    raw = R.oracle_boot(o, bkey, None)(0, a[:3 * n], b[:3 * n], a[3 * n:], b[3 * n:])
    lwe = np.stack([raw[ct * n:(ct + 1) * n, ct] for ct in range(3)])
    call = 0
    if key:
        eng.set_random_flatten(True, key)
        eng.bootstrap_batch(a[:2], b[:2], a[2:4], b[2:4])                 # call 0
        call = 1
    w, v = eng.pack_lwe_modq(lwe)
    assert w.shape == v.shape == (3, params.m)
    fast = R.FastTail(R.bigint_params(params), R.key_lists(oc, bkey, n, params.m))
    x, y = bits[:3 * n], bits[3 * n:]
    for ct, fn in enumerate((np.bitwise_and, np.bitwise_or, np.bitwise_xor)):
        ow, ov = fast(lwe[ct], seed=key, ct=ct, call=call)
        assert np.array_equal(w[ct], ow) and np.array_equal(v[ct], ov), "ciphertext %d (%s)" % (ct, mode)
        sl = slice(ct * n, (ct + 1) * n)
        assert np.array_equal(S.host.decrypt_rlwe(params, sk, w[ct], v[ct]), fn(x[sl], y[sl]))
    if key:     # the call took one number, and no bootstrap draws: the next bootstrap call is call 2
        got = eng.bootstrap_batch(a[:2], b[:2], a[2:4], b[2:4])
        assert np.array_equal(got, o.bootstrap_batch(bkey, a[:2], b[:2], a[2:4], b[2:4], rnd=(key, 2)))
    eng.close()


def test_tail_after_raw_refresh_is_pack_encrypted_bits(S, oc):
    """Deterministic: sgfhe_pack_encrypted_bits(a, b) = sgfhe_pack_lwe_modq of the un-reduced AND rows of
    sgfhe_bootstrap_batch(0, Dr, a, b, SGFHE_FLAG_RAW_MODQ)."""
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 111)
    n = params.n
    bits = np.random.default_rng(112).integers(0, 2, size=2 * n).astype(np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits, 113)
    want = eng.pack_encrypted_bits(a.reshape(2, n, n), b.reshape(2, n))
    raw = eng.bootstrap_batch(np.zeros_like(a), np.full_like(b, params.Dr), a, b, raw=True)
    got = eng.pack_lwe_modq(raw[:, 0].reshape(2, n, n + 1, 2))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    eng.close()


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_circuit_direct_equals_the_oracle_replay(S, oc, mode):
    """The circuit of the host test (AND, ~OR, XOR, an input, a negated input, TRUE, one wire twice), two blocks:
    (w, v) word for word the oracle replay, out_lwe the bytes of the flags = 0 run, decryption the plain evaluation."""
    from sgfhe_jl_amd import circuit as C
    key = KEY32 if mode == "randomised" else None
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 121)
    n = params.n
    c = R.direct_circuit(S)
    blocks = 2
    bits = np.random.default_rng(122).integers(0, 2, size=(3, blocks, n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 123)
    plain = c.evaluate_plain(bits.reshape(3, -1))
    _set_mode([eng], key)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True)
    _set_mode([eng], key)
    (w0, v0), lwe0 = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
    assert np.array_equal(lwe, lwe0), "out_lwe differs from the flags = 0 run (%s)" % mode
    assert not np.array_equal(w, w0)
    bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
    (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, R.oracle_boot(o, bkey, key), R.oracle_tail(bp, bk, key))
    assert np.array_equal(lwe, rlwe)
    assert np.array_equal(w, rw) and np.array_equal(v, rv), "packed outputs differ from the oracle replay (%s)" % mode
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    assert np.array_equal(_decrypt_ct(S, params, sk, w0, v0), plain)
    print("worst packed phase error, %s: direct %d, refreshed %d, against Dr / 2 = %d"
          % (mode, _worst_phase(params, sk, w, v, plain), _worst_phase(params, sk, w0, v0, plain), params.Dr // 2))
    eng.close()


def test_pack_stage_wider_than_one_group_randomised(S, oc):
    """70 outputs x 2 blocks = 140 ciphertexts = groups of 128 and 12 at Params(64): the first all direct (no bootstrap
    call), the second with refreshed ciphertexts among direct ones; against the composition on a second ctx."""
    params, o, sk, bkey, (eng, ref) = _setup64(S, oc, 131, engines=2)
    n = params.n
    c = S.Circuit(2)
    x, y = c.inputs
    g1 = c.gate(x, y)
    g2 = c.gate(g1[0], ~g1[2])
    c.output(*([g2[0], g2[1], ~g2[2], g1[1]] * 16 + [x, g2[0], S.Circuit.TRUE, ~y, ~g1[2], S.Circuit.FALSE]))
    assert c.n_outputs == 70 and c.info()["levels"] == 2
    blocks = 2
    bits = np.random.default_rng(132).integers(0, 2, size=(2, blocks, n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 133)
    _set_mode([eng, ref], KEY32)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True)
    (rw, rv), rlwe = _engine_replay(c, a, b, params, ref)
    assert np.array_equal(lwe, rlwe)
    assert np.array_equal(w, rw) and np.array_equal(v, rv)
    plain = c.evaluate_plain(bits.reshape(2, -1))
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), plain)
    # two level calls, a tail (first group), a bootstrap call and a tail (second group): the next call is number 5
    x3, y3 = lwe[64, :3], lwe[67, :3]
    got = eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])
    assert np.array_equal(got, o.bootstrap_batch(bkey, x3[:, :n], x3[:, n], y3[:, :n], y3[:, n], rnd=(KEY32, 5)))
    eng.close()
    ref.close()


def test_adder_p1024_direct(S, oc, gpu_keys):
    """A 4-bit adder over one block at Params(1024), deterministic: bytes equal the composition of the engine's own
    primitives on a second ctx (un-reduced bootstrap calls, host ModRed, sgfhe_pack_lwe_modq); the sums decrypt to
    x + y from the packed outputs alone."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import encrypted_adder
    params, o, sk, eng = gpu_keys.engine(1024)
    ref = eng.clone()
    nbits, inst = 4, params.n
    c = encrypted_adder.adder_circuit(S, nbits)
    rng = np.random.default_rng(141)
    xs, ys = rng.integers(0, 16, size=inst), rng.integers(0, 16, size=inst)
    plain = np.array([(xs >> i) & 1 for i in range(nbits)] + [(ys >> i) & 1 for i in range(nbits)])
    a, b = _encrypt_cts(S, params, sk, plain[:, None, :], 142)
    try:
        _set_mode([eng, ref], None)
        w, v = eng.circuit_run_ct(c, a, b, direct=True)
        (rw, rv), _ = _engine_replay(c, a, b, params, ref)
        assert np.array_equal(w, rw) and np.array_equal(v, rv)
        dec = _decrypt_ct(S, params, sk, w, v).astype(np.int64)
        assert np.array_equal(sum(dec[i] << i for i in range(nbits + 1)), xs + ys)
    finally:
        ref.close()
        eng.set_random_flatten(False)
        eng.release_host_staging()


def test_edge_cases(S, oc):
    params, o, sk, bkey, (eng,) = _setup64(S, oc, 151)
    n, m = params.n, params.m
    L = S.lib()
    c = R.direct_circuit(S)
    blocks = 2
    bits = np.random.default_rng(152).integers(0, 2, size=(3, blocks, n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 153)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    ow = np.full((c.n_outputs, blocks, m), SENTINEL, dtype=np.uint64)
    ov, ol = ow.copy(), np.full((c.n_outputs, blocks * n, n + 1), SENTINEL, dtype=np.uint64)
    untouched = lambda: np.all(ow == SENTINEL) and np.all(ov == SENTINEL) and np.all(ol == SENTINEL)
    # an unknown flag bit
    for flags in (2, DIRECT | 0x80000000):
        assert L.sgfhe_circuit_run_ct_ex(eng._h, c.handle(), blocks, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol), flags) == -1
    assert untouched()
    # a residue that is not below Q: nothing written
    lwe = np.zeros((2, n, n + 1, 2), dtype=np.uint64)
    lwe[1, n - 1, n] = (params.Q & (2 ** 64 - 1), params.Q >> 64)
    assert L.sgfhe_pack_lwe_modq(eng._h, ptr(lwe), 2, ptr(ow), ptr(ov)) == -1 and untouched()
    lwe[1, n - 1, n] = ((params.Q - 1) & (2 ** 64 - 1), (params.Q - 1) >> 64)
    w2, v2 = eng.pack_lwe_modq(lwe)                                   # Q - 1 is a residue
    assert w2.shape == (2, m)
    assert eng.pack_lwe_modq(np.zeros((0, n, n + 1, 2), dtype=np.uint64))[0].shape == (0, m)
    # blocks = 0
    w0, v0 = eng.circuit_run_ct(c, np.zeros((3, 0, n), np.uint64), np.zeros((3, 0, n), np.uint64), direct=True)
    assert w0.shape == v0.shape == (c.n_outputs, 0, m)
    # a ctx without a key
    nokey = S.Engine(params)
    assert L.sgfhe_circuit_run_ct_ex(nokey._h, c.handle(), blocks, ptr(a), ptr(b), n, ptr(ow), ptr(ov), ptr(ol), DIRECT) == -5
    assert L.sgfhe_pack_lwe_modq(nokey._h, ptr(lwe), 2, ptr(ow), ptr(ov)) == -5 and untouched()
    nokey.close()
    # out_w NULL with the flag: the flags = 0 run (the LWE outputs; the level calls of the draw stream and no more)
    want = eng.circuit_run_ct(c, a, b, packed=False, lwe=True)
    assert np.array_equal(eng.circuit_run_ct(c, a, b, packed=False, lwe=True, direct=True), want)
    eng.set_random_flatten(True, KEY32)
    eng.circuit_run_ct(c, a, b, packed=False, lwe=True, direct=True)
    x3, y3 = want[0, :3], want[1, :3]
    got = eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])
    assert np.array_equal(got, o.bootstrap_batch(bkey, x3[:, :n], x3[:, n], y3[:, :n], y3[:, n], rnd=(KEY32, 2)))
    eng.set_random_flatten(False)
    # a clone runs direct with its parent's bytes; so does the ctx after release_host_staging, and the refreshed
    # run after a direct one is the refreshed run
    refreshed = eng.circuit_run_ct(c, a, b)
    w, v = eng.circuit_run_ct(c, a, b, direct=True)
    cl = eng.clone()
    wc, vc = cl.circuit_run_ct(c, a, b, direct=True)
    assert np.array_equal(wc, w) and np.array_equal(vc, v)
    cl.close()
    eng.release_host_staging()
    w3, v3 = eng.circuit_run_ct(c, a, b, direct=True)
    assert np.array_equal(w3, w) and np.array_equal(v3, v)
    again = eng.circuit_run_ct(c, a, b)
    assert np.array_equal(again[0], refreshed[0]) and np.array_equal(again[1], refreshed[1])
    assert np.array_equal(_decrypt_ct(S, params, sk, w, v), c.evaluate_plain(bits.reshape(3, -1)))
    eng.close()


@pytest.fixture(scope="module")
def straddle(S, oc):
    """Shared by the four cases below, built once and left unchanged: two ctxs under one key, the circuit, its
    encrypted inputs and its plain evaluation."""
    params, o, sk, bkey, engs = _setup64(S, oc, 161, engines=2)
    c = S.Circuit(2)
    x, y = c.inputs
    g0, g1, g2 = c.gate(x, y), c.gate(x, ~y), c.gate(~x, y)
    c.output(g2[1], g0[0], x, ~g1[2])
    blocks = 44
    bits = np.random.default_rng(162).integers(0, 2, size=(2, blocks, params.n)).astype(bool)
    a, b = _encrypt_cts(S, params, sk, bits, 163)
    yield dict(params=params, o=o, sk=sk, bkey=bkey, engs=engs, c=c, a=a, b=b,
               plain=c.evaluate_plain(bits.reshape(2, -1)))
    for e in engs:
        e.close()


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
@pytest.mark.parametrize("lift", [False, True], ids=["direct", "direct+lift"])
def test_unreduced_level_call_split_inside_a_producing_node(S, oc, straddle, mode, lift):
    """Params(64), 44 blocks = 2816 instances, one level of 3 nodes = 8448 rows: the level is two calls, both un-reduced,
    and call 0 ends at row 8192, inside node 2 (rows 5632 .. 8447), whose OR wire is output 0 -- its job belongs to both
    calls, each copying the rows it holds.  Outputs: OR of node 2, AND of node 0, input x, ~XOR of node 1: 176
    ciphertexts = groups of 128 and 48; the first ends with 40 refreshed (lifted) ciphertexts of x, the second opens
    with the other 4 and goes on with 44 direct ones.  (w, v) and out_lwe byte for byte against
    circuit.replay_ct_direct on a second ctx's own un-reduced bootstrap_batch and pack_lwe_modq, which number their
    calls themselves.  Call numbers consumed, by the closed form: 2 level calls (ceil(8448 / 8192)); direct: 2 per
    group (both refresh something), 6 in all; lifted: 1 per group, 4 in all.  The replay makes exactly that many
    calls; randomised, the next bootstrap on the run's ctx is the oracle's call of that number (deterministic runs draw
    nothing: every call is number 0 and the counter cannot be observed)."""
    from sgfhe_jl_amd import circuit as C
    key = KEY32 if mode == "randomised" else None
    K = straddle
    params, o, bkey, c, a, b = K["params"], K["o"], K["bkey"], K["c"], K["a"], K["b"]
    eng, ref = K["engs"]
    n, blocks = params.n, a.shape[1]
    assert blocks * n == 2816 and c.info()["levels"] == 1 and c.info()["nodes"] == 3
    assert 3 * blocks * n == 8448 and c.n_outputs * blocks == 176 and C.pack_calls(n) == 128
    level_calls = -(-3 * blocks * n // 8192)
    want_calls = level_calls + (2 if lift else 2 * 2)
    calls = []
    _set_mode([eng, ref], key)
    (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True, lift=lift)
    (rw, rv), rlwe = C.replay_ct_direct(
        c, a, b, params,
        lambda call, a1, b1, a2, b2: (calls.append(call), ref.bootstrap_batch(a1, b1, a2, b2, raw=True))[1],
        lambda call, group: (calls.append(call), ref.pack_lwe_modq(group))[1], lift=lift)
    # (what the REPLAY numbered, a property of replay_ct_direct: it says the composition the bytes are compared with
    # makes the closed-form number of calls, and is no evidence about the engine's own counter.  The engine's counter
    # is pinned below, in the randomised mode only: a deterministic run numbers every call 0 and the counter is not
    # exposed by the ABI.)
    assert calls == list(range(want_calls))
    assert np.array_equal(lwe, rlwe)
    assert np.array_equal(w, rw) and np.array_equal(v, rv), "packed outputs differ from the replay (%s)" % mode
    # (decryption of two ciphertexts per output, one of each group where the output has both)
    for q, t in ((0, 0), (0, 43), (1, 0), (2, 39), (2, 40), (3, 43)):
        assert np.array_equal(S.host.decrypt_rlwe(params, K["sk"], w[q, t], v[q, t]), K["plain"][q, t * n:(t + 1) * n])
    if key:     # the engine's counter: its next call draws as call number `want_calls` of the stream
        x3, y3 = lwe[0, :3], lwe[1, :3]
        got = eng.bootstrap_batch(x3[:, :n], x3[:, n], y3[:, :n], y3[:, n])
        assert np.array_equal(got, o.bootstrap_batch(bkey, x3[:, :n], x3[:, n], y3[:, :n], y3[:, n],
                                                     rnd=(key, want_calls)))
