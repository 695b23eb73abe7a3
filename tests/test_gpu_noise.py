"""The noise probe on the device (sgfhe_lwe_noise, sgfhe_circuit_run_probe) against its
restatement on the host (tests/noise_ref.py).  Every statistic is an integer: all comparisons are equalities.
Keys are generated on the device (sgfhe_bkey_generate)."""

import ctypes

import numpy as np
import pytest

import noise_ref as NR
from test_noise_host import _all_wires_circuit, _probe_circuit

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_NO_KEY = -1, -5
SENTINEL = 0xA5A5A5A5A5A5A5A5
KEY32 = bytes(range(7, 39))


def _rows(a, b):
    return np.concatenate([a, b[:, None]], axis=1)


def _gate_rows(o, sk, eng, pairs, seed, raw=False):
    """`pairs` bootstraps of fresh encryptions: (result [pairs][3][n + 1]([2]), plaintext bits [pairs][3])."""
    bits = np.random.default_rng(seed).integers(0, 2, size=2 * pairs).astype(np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits, seed + 1)
    out = eng.bootstrap_batch(a[:pairs], b[:pairs], a[pairs:], b[pairs:], raw=raw)
    x, y = bits[:pairs], bits[pairs:]
    return out, np.stack([x & y, x | y, x ^ y], axis=1)


def test_zr_primitive_params64(S, gpu_keys):
    """The 3 * 37 gate rows of one call in place; one gate through the stride; one row; none; five flipped
    bits; rows with hand-placed errors at every threshold of the record."""
    params, o, sk, eng = gpu_keys.engine(64)
    n = params.n
    out, exp = _gate_rows(o, sk, eng, 37, 300)
    rows, flat = out.reshape(-1, n + 1), exp.reshape(-1)
    ref = NR.record_zr(params, sk, rows, flat)
    assert ref[0] == 111 and ref[1] == 0
    assert eng.lwe_noise(sk, out, flat) == S.NoiseStats(*ref)
    assert eng.lwe_noise(sk, out, flat, stride=n + 1) == S.NoiseStats(*ref)
    for g in range(3):      # gate g of [batch][3][n + 1] in place
        got = eng.lwe_noise(sk, out.reshape(-1)[g * (n + 1):], exp[:, g], stride=3 * (n + 1))
        assert got == S.NoiseStats(*NR.record_zr(params, sk, out[:, g], exp[:, g])), g
    assert eng.lwe_noise(sk, rows[5], flat[5:6]) == S.NoiseStats(*NR.record_zr(params, sk, rows[5:6], flat[5:6]))
    assert eng.lwe_noise(sk, np.zeros(0, np.uint64), np.zeros(0, np.uint8)) == S.NoiseStats(0, 0, 0, 0, 0, 0)
    flipped = flat.copy()
    flipped[[0, 17, 50, 64, 110]] ^= 1
    got = eng.lwe_noise(sk, out, flipped)
    assert got.wrong == 5 and got == S.NoiseStats(*NR.record_zr(params, sk, rows, flipped))
    errs = NR.boundary_errors(params)
    for bit in (0, 1):
        hand = NR.handmade_zr(params, sk, np.random.default_rng(310 + bit), errs, [bit] * len(errs))
        for i, e in enumerate(errs):
            got = eng.lwe_noise(sk, hand[i], [bit])
            assert got == S.NoiseStats(*NR.record_zr(params, sk, hand[i:i + 1], [bit])), (e, bit)
            assert (got.max_abs, got.sum, got.sum_sq) == (abs(e), e, e * e)
        assert eng.lwe_noise(sk, hand, [bit] * len(errs)) == \
            S.NoiseStats(*NR.record_zr(params, sk, hand, [bit] * len(errs)))


def test_zr_primitive_params256_ragged_rows(S, gpu_keys):
    """n = 256: four words of a row per lane.  21 gate rows and 45 fresh encryptions: 66 rows, four workgroups
    of 16 and one of 2."""
    params, o, sk, eng = gpu_keys.engine(256)
    n = params.n
    out, exp = _gate_rows(o, sk, eng, 7, 320)
    bits = np.random.default_rng(322).integers(0, 2, size=45).astype(np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits, 323)
    rows = np.concatenate([out.reshape(-1, n + 1), _rows(a, b)])
    expected = np.concatenate([exp.reshape(-1), bits])
    assert len(rows) == 66
    ref = NR.record_zr(params, sk, rows, expected)
    assert ref[1] == 0 and ref[2] > 0
    assert eng.lwe_noise(sk, rows, expected) == S.NoiseStats(*ref)
    for count in (15, 16, 17):
        assert eng.lwe_noise(sk, rows[:count], expected[:count]) == \
            S.NoiseStats(*NR.record_zr(params, sk, rows[:count], expected[:count])), count


def _residue(row, j, value):
    row[j] = (value & (2 ** 64 - 1), value >> 64)


@pytest.mark.parametrize("n", [64, 256])
def test_zq_primitive(S, gpu_keys, n):
    """Un-reduced rows of a SGFHE_FLAG_RAW_MODQ call in both flatten modes against the Python-int record; an error
    placed at exactly DQ_tilde - 1 and at DQ_tilde; a residue equal to Q is refused."""
    params, o, sk, eng = gpu_keys.engine(n)
    Q, DQ = params.Q, params.DQ_tilde
    try:
        for key in (None, KEY32):
            eng.set_random_flatten(key is not None, key or 0)
            raw, exp = _gate_rows(o, sk, eng, 9, 330 + n, raw=True)          # 27 rows: a ragged last workgroup
            ref = NR.record_zq(params, sk, raw, exp)
            assert ref[0] == 27 and ref[1] == 0 and 0 < ref[2] < DQ
            assert eng.lwe_noise(sk, raw, exp.reshape(-1), raw=True) == S.NoiseStatsQ(*ref)
            g1 = eng.lwe_noise(sk, raw.reshape(-1)[2 * (n + 1):], exp[:, 1], raw=True, stride=6 * (n + 1))
            assert g1 == S.NoiseStatsQ(*NR.record_zq(params, sk, raw[:, 1], exp[:, 1]))
    finally:
        eng.set_random_flatten(False)
    row, bit = raw[4, 2].copy(), int(exp[4, 2])
    e = NR.errors_zq(params, sk, row, [bit])[0]
    b = int(row[n, 0]) | (int(row[n, 1]) << 64)
    for placed, wrong in ((DQ - 1, 0), (DQ, 1), (-DQ, 1), (-(DQ - 1), 0)):
        _residue(row, n, (b - e + placed) % Q)
        assert NR.errors_zq(params, sk, row, [bit]) == [placed]
        assert eng.lwe_noise(sk, row, [bit], raw=True) == S.NoiseStatsQ(1, wrong, abs(placed), abs(placed))
    assert eng.lwe_noise(sk, np.zeros(0, np.uint64), np.zeros(0, np.uint8), raw=True) == S.NoiseStatsQ(0, 0, 0, 0)
    bad = raw[:3, 0].copy()
    _residue(bad[2], 7, Q)
    with pytest.raises(S.SgfheError) as ei:
        eng.lwe_noise(sk, bad, exp[:3, 0], raw=True)
    assert ei.value.code == ERR_INVALID_ARG
    _residue(bad[2], 7, Q - 1)
    assert eng.lwe_noise(sk, bad, exp[:3, 0], raw=True).rows == 3


def _circuit_engines(S, gpu_keys):
    params, o, sk, _ = gpu_keys.engine(64)
    engs = []
    for _ in range(2):
        e = S.Engine(params)
        e.generate_key(sk, gpu_keys.KEY_SEED)
        engs.append(e)
    return params, o, sk, engs


def _check_probe(S, params, o, sk, engs, instances, key, seed):
    A, B = engs
    n = params.n
    c = _probe_circuit(S)
    d, wires = _all_wires_circuit(S, c)
    bits = np.random.default_rng(seed).integers(0, 2, size=(c.n_inputs, instances)).astype(np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits.reshape(-1), seed + 1)
    inputs = _rows(a, b).reshape(c.n_inputs, instances, n + 1)
    for e in engs:
        e.set_random_flatten(key is not None, key or 0)          # (the call counter starts again at 0)
    out, stats = A.circuit_probe(c, inputs, sk, bits)
    # (a) the bytes of sgfhe_circuit_run, and the same call number afterwards
    assert np.array_equal(out, B.circuit_run(c, inputs))
    nxt = [e.bootstrap_batch(a[:3], b[:3], a[3:6], b[3:6]) for e in engs]
    assert np.array_equal(nxt[0], nxt[1])
    # (b) every wire against the reference on the LWEs a run with every wire as an output returns
    B.set_random_flatten(key is not None, key or 0)
    lwes = B.circuit_run(d, inputs)
    plain = d.evaluate_plain(bits)
    assert len(stats) == c.n_inputs + 3 * c.n_gates
    for w, rows, exp in zip(wires, lwes, plain):
        assert stats[w] == S.NoiseStats(*NR.record_zr(params, sk, rows, exp)), (w, instances)
        assert stats[w].rows == instances and stats[w].wrong == 0          # (d)
    # (c) the pruned node (node 3) and nothing else
    for w in range(len(stats)):
        if w not in wires:
            assert (w - c.n_inputs) // 3 == 3 and stats[w] == S.NoiseStats(0, 0, 0, 0, 0, 0), w


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
@pytest.mark.parametrize("instances", [5, 70])
def test_circuit_probe(S, gpu_keys, instances, mode):
    """Three levels; AND, ~OR and XOR read; unread gate outputs; a pruned node; inputs read negated, twice and not
    at all; both constants.  70 instances: the two nodes of a level share workgroup-sized tiles unevenly."""
    params, o, sk, engs = _circuit_engines(S, gpu_keys)
    try:
        _check_probe(S, params, o, sk, engs, instances, KEY32 if mode == "randomised" else None, 340 + instances)
    finally:
        for e in engs:
            e.close()


def test_circuit_probe_level_wider_than_a_call(S, gpu_keys):
    """4200 instances: a level of two nodes is 8400 rows, two calls -- the first ends inside the second node, the
    second starts there -- and both add into the same records."""
    params, o, sk, engs = _circuit_engines(S, gpu_keys)
    try:
        _check_probe(S, params, o, sk, engs, 4200, None, 350)
    finally:
        for e in engs:
            e.close()


def test_argument_errors(S, gpu_keys):
    params, o, sk, _ = gpu_keys.engine(64)
    n = params.n
    L = S.lib()
    eng = S.Engine(params)                       # no key
    try:
        sk64 = np.ascontiguousarray(sk, dtype=np.uint64)
        rows = NR.handmade_zr(params, sk, np.random.default_rng(360), [3, -4], [0, 1])
        exp = np.array([0, 1], dtype=np.uint8)
        st = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        # the primitive needs no bootstrap key
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), p(rows), 2, n + 1, p(exp), 0, st) == 0
        assert list(st) == [2, 0, 4, (1 << 64) - 1, 25, 0, 0, 0]
        assert L.sgfhe_lwe_noise(eng._h, None, p(rows), 2, n + 1, p(exp), 0, st) == ERR_INVALID_ARG
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), None, 2, n + 1, p(exp), 0, st) == ERR_INVALID_ARG
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), p(rows), 2, n + 1, None, 0, st) == ERR_INVALID_ARG
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), p(rows), 2, n + 1, p(exp), 0, None) == ERR_INVALID_ARG
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), p(rows), 2, n, p(exp), 0, st) == ERR_INVALID_ARG        # short stride
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), p(rows), 2, n + 1, p(exp), 2, st) == ERR_INVALID_ARG    # RAW_RNS2
        assert L.sgfhe_lwe_noise(eng._h, p(sk64), p(rows), 1, 2 * n + 3, p(exp), 1, st) == ERR_INVALID_ARG  # odd, Z_Q
        c = _probe_circuit(S)
        inst = 3
        bits = np.zeros((c.n_inputs, inst), dtype=np.uint8)
        a, b = o.lwe_encrypt_bits(sk, bits.reshape(-1), 361)
        inputs = np.ascontiguousarray(_rows(a, b).reshape(c.n_inputs, inst, n + 1))
        out = np.full((c.n_outputs, inst, n + 1), SENTINEL, dtype=np.uint64)
        stats = np.zeros((c.n_inputs + 3 * c.n_gates, 8), dtype=np.uint64)
        run = lambda h, s, bi, stt: L.sgfhe_circuit_run_probe(h, c.handle(), inst, p(inputs), p(out), s, bi, stt)
        assert run(eng._h, p(sk64), p(bits), p(stats)) == ERR_NO_KEY
        assert (out == SENTINEL).all()
        eng.generate_key(sk, gpu_keys.KEY_SEED)
        assert run(eng._h, None, p(bits), p(stats)) == ERR_INVALID_ARG
        assert run(eng._h, p(sk64), None, p(stats)) == ERR_INVALID_ARG
        assert run(eng._h, p(sk64), p(bits), None) == ERR_INVALID_ARG
        assert (out == SENTINEL).all()
        assert run(eng._h, p(sk64), p(bits), p(stats)) == 0
        assert not (out == SENTINEL).any() and stats[0, 0] == inst
        eng.release_host_staging()               # the probe's tables go with the staging, and come back
        assert run(eng._h, p(sk64), p(bits), p(stats)) == 0 and stats[4, 0] == inst
    finally:
        eng.close()
