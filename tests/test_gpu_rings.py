"""Circuits, LUT bootstraps, the lift to Z_Q and the noise probe on every ring kind the ctx accepts (tests/ring_cases.py):
a Q below 2^24 on k_crt_acc2 / k_crt_acc, a single-limb Q just below 2^64, the wide base of MODE_WIDE under a 93-bit Q,
a composite Q keyed in limb form, and m = 128 -- at n = 8 and 16, where a wave spans several rows of n + 1 words, the
split has one ragged tile and the probe fewer key bits than lanes.  Every comparison is equality of every word, against
the project's C and big-integer oracles and Python integers; each case first holds kernel_names() to the ring table.

Decryption and "no wrong row" are asserted under the noise rules of include/sgfhe_hip.h only: the rule's condition is
measured first on the oracle's replay with the secret key (lut_ref.lut_input_sum_errors for LUT nodes; the replay's own
decryption for the others).  The key noise of ring_cases, crafted input errors of at most r/64 (LWE form) and Dr/16
(ciphertext form) and the key seeds below make the oracle replay alone satisfy it on all five rings in both flatten
modes: checked on the CPU, worst LUT input-sum error 2 of Dr/8 = 4 at n = 8 and 2 of Dr/8 = 8 at n = 16.  A case is never
skipped: where a ring has no randomised mode or no pack, the documented SGFHE_ERR_UNSUPPORTED is asserted, and that
nothing was written."""

import ctypes

import numpy as np
import pytest

import lut_ref as LR
import noise_ref as NR
import pack_direct_ref as R
import pack_lift_ref as PL
import ring_cases as RC

pytestmark = pytest.mark.gpu

KEY32 = RC.KEY32
SENTINEL = 0xA5A5A5A5A5A5A5A5
SMALL_BATCH_DEFAULT = 24
# secret-key seed per ring (the key seed is one more): at n = 8 a row's ModRed rounding alone is up to (1 + key bits) / 2
# of Dr/8 = 4, so the seeds are ones whose oracle replay keeps every LUT input sum inside the rule (module docstring)
SK_SEED = {"tiny": 401, "limb64": 411, "wide": 421, "composite": 431, "m128": 441}


class Case:
    """One ring: oracles, key, and (on first use) the keyed engine, for the module."""

    def __init__(self, S, oc, name):
        self.S, self.name = S, name
        self.rg = RC.ring(S, name)
        self.params = self.rg.params
        self.o, self.lo = RC.oracles(oc, self.rg)
        self.sk = self.o.private_key(SK_SEED[name])
        self.bkey = self.o.bootstrap_key(self.sk, SK_SEED[name] + 1, noise=self.rg.noise)
        self.khat = self.o.key_transform(self.bkey)
        self.bp = R.bigint_params(self.params)
        self.bk = R.key_lists(oc, self.bkey, self.params.n, self.params.m)
        self._eng = None

    @property
    def eng(self):
        if self._eng is None:
            self._eng = self.S.Engine(self.params)
            RC.upload(self._eng, self.rg, self.bkey)
        return self._eng

    def mode(self, rnd):
        """-> whether the mode exists (RC.set_mode asserts the kernel names, or the refusal)."""
        return RC.set_mode(self.S, self.eng, self.rg, rnd)

    def close(self):
        if self._eng is not None:
            self._eng.close()
            self._eng = None


_CASES = {}


@pytest.fixture(scope="module", params=RC.NAMES)
def case(S, oc, request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(S, oc, request.param)
    yield _CASES[request.param]
    _CASES[request.param].close()


def _key(rnd):
    return KEY32 if rnd else None


# ---- the lift ---------------------------------------------------------------------------------------------------------

def lift_rows(params):
    """All r words as rows of n + 1, the last row padded with 0 and r - 1 in turn."""
    n, r = params.n, params.r
    rows = -(-r // (n + 1))
    x = np.zeros(rows * (n + 1), dtype=np.uint64)
    x[:r] = np.arange(r)
    x[r:] = [(r - 1) * (i & 1) for i in range(len(x) - r)]
    return x.reshape(rows, n + 1)


def _check_lift(eng, params):
    x = lift_rows(params)
    got = eng.lwe_lift(x)
    Q, r = params.Q, params.r
    want = [(int(v) * Q + r // 2) // r for v in x.reshape(-1)]
    assert [int(lo) | (int(hi) << 64) for lo, hi in got.reshape(-1, 2)] == want


def test_lwe_lift_every_word(case):
    assert case.mode(False)
    _check_lift(case.eng, case.params)


def test_lwe_lift_every_word_params2048(S):
    """No key is needed: the one full-size ring, r = 32768 (16 rows of 2049 words)."""
    params = S.Params(2048)
    eng = S.Engine(params)
    try:
        _check_lift(eng, params)
    finally:
        eng.close()


# ---- the LUT primitive -------------------------------------------------------------------------------------------------

LUT_FEW = (0x96, 0xE8, 0xCA, 0xFF, 0x10)


def lut_rows(case):
    """256 rows: table t, sum (t + t div 8) mod 8 -- every sum under every residue of t mod 8 --, errors cycling through
    0, +-1 and +-(r/32 - 1), the last value inside the rule."""
    p = case.params
    lim = p.r // 32 - 1
    errs = (0, 1, -1, lim, -lim)
    t = np.arange(256)
    s = (t + t // 8) % 8
    e = np.array([errs[i % 5] for i in t])
    a, b = LR.rows_at(p, case.sk, s, e, np.random.default_rng(500 + p.n))
    return a, b, t.astype(np.uint8), (t >> s) & 1


def lut_reference(case, a, b, tables, rnd, call=0):
    """(reduced, raw) rows of lut_ref.rows_from_acc on the low-amplitude oracle, as call `call` of the draw stream."""
    z = np.zeros_like(a), np.zeros_like(b)
    _, acc = case.lo.bootstrap_batch(case.khat, a, b, z[0], z[1], want_acc=True, opt=True,
                                     rnd=(KEY32, call) if rnd else None)
    return LR.rows_from_acc(case.params, acc, tables), LR.rows_from_acc(case.params, acc, tables, raw=True)


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_lut_primitive(case, rnd):
    """All 256 tables in chunks of 64 on both lanes, then five rows in the small-batch form and again in the throughput
    form (set_small_batch_max(0): on `wide`, randomised, k_extprod<6, 3, true> then carries LUT rows); reduced and raw.
    The rows are inside the rule by construction and the oracle's rows decrypt at all three scales."""
    if not case.mode(rnd):
        return
    eng, p = case.eng, case.params
    a, b, tables, want = lut_rows(case)
    few = [int(np.flatnonzero(tables == t)[0]) for t in LUT_FEW]
    ref = lut_reference(case, a, b, tables, rnd)
    ref_few = lut_reference(case, a[few], b[few], tables[few], rnd)
    for k in range(3):
        assert np.array_equal(LR.decrypt_scaled(p, case.sk, ref[0][:, k], k), want), k
    try:
        for raw in (False, True):
            eng.set_chunk(64)
            case.mode(rnd)
            assert np.array_equal(eng.bootstrap_lut_batch(a, b, tables, raw=raw), ref[raw]), ("chunks", raw)
            eng.set_chunk(0)
            for small in (SMALL_BATCH_DEFAULT, 0):
                eng.set_small_batch_max(small)
                case.mode(rnd)
                got = eng.bootstrap_lut_batch(a[few], b[few], tables[few], raw=raw)
                assert np.array_equal(got, ref_few[raw]), ("five rows", small, raw)
    finally:
        eng.set_chunk(0)
        eng.set_small_batch_max(SMALL_BATCH_DEFAULT)
        eng.set_random_flatten(False)


# ---- the mixed circuit, LWE form -----------------------------------------------------------------------------------------

INSTANCES = 12                                   # a multiple of the group of 4, not of 8


def lwe_inputs(case):
    """bits [3][12] and their LWEs with |e| <= r/64, made from the secret key."""
    p = case.params
    rng = np.random.default_rng(510 + p.n)
    bits = rng.integers(0, 2, size=(3, INSTANCES)).astype(bool)
    e = rng.integers(-(p.r // 64), p.r // 64 + 1, size=bits.size)
    return bits, NR.handmade_zr(p, case.sk, rng, e, bits.reshape(-1)).reshape(3, INSTANCES, p.n + 1)


def lwe_reference(case, c, inputs, bits, rnd):
    """replay_levels on the two oracles, after the rule's condition: every LUT input sum inside Dr/8, and the replay
    itself decrypts to the plain evaluation."""
    from sgfhe_jl_amd import circuit as C
    p = case.params
    boot, boot_lut = LR.oracle_boots(case.o, case.lo, case.bkey, p, _key(rnd))
    worst = LR.lut_input_sum_errors(case.S, p, case.sk, c, inputs, bits, boot, boot_lut)
    assert len(worst) == 4 and max(worst.values()) < p.r // 32, worst
    ref = C.replay_levels(c, inputs, p.r, boot, boot_lut)
    assert np.array_equal(_decrypt(case, ref), c.evaluate_plain(bits))
    return ref


def _decrypt(case, lwe):
    return LR.decrypt_scaled(case.params, case.sk, lwe, 0).reshape(lwe.shape[:-1]).astype(bool)


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_mixed_circuit_lwe_form(case, rnd):
    if not case.mode(rnd):
        return
    c = RC.mixed_circuit(case.S, "lwe")
    bits, inputs = lwe_inputs(case)
    ref = lwe_reference(case, c, inputs, bits, rnd)
    try:
        got = case.eng.circuit_run(c, inputs)
    finally:
        case.eng.set_random_flatten(False)
    assert np.array_equal(got, ref)
    assert np.array_equal(_decrypt(case, got), c.evaluate_plain(bits))


# ---- the same circuit, ciphertext form -----------------------------------------------------------------------------------

BLOCKS = 2
FLAGS = ((False, False), (True, False), (True, True))          # (direct, lift)


def ct_inputs(case):
    """bits [3][2][n]; ciphertexts of length n with errors up to Dr/16, and the length-m form of the same LWEs."""
    p = case.params
    bits = np.random.default_rng(520 + p.n).integers(0, 2, size=(3, BLOCKS, p.n)).astype(bool)
    a, b = PL.craft_cts(case.S, p, case.sk, bits, 521)
    return bits, (a, b), PL.widen_cts(a, b, p.m, 522)


def ct_reference(case, c, a, b, rnd, direct, lift):
    from conftest import oracle_threads
    from sgfhe_jl_amd import circuit as C
    p, o, key = case.params, case.o, _key(rnd)
    if not direct:
        T = oracle_threads()                            # (the default is every core of the machine, quota or not)
        boot, boot_lut = LR.oracle_boots(o, case.lo, case.bkey, p, key)
        khat = case.khat if o.uses_ntt else None        # (the limb-wise oracle packs from the canonical key)
        pack = lambda call, pa, pb: tuple(np.stack(x) for x in zip(*[
            o.pack_encrypted_bits(case.bkey, pa[i], pb[i], khat=khat, threads=T, rnd=(key, i, call) if key else None)
            for i in range(len(pa))]))
        return C.replay_ct(c, a, b, p, boot, pack, boot_lut)
    braw, braw_lut = LR.oracle_boots(o, case.lo, case.bkey, p, key, raw=True)
    return C.replay_ct_direct(c, a, b, p, braw, R.oracle_tail(case.bp, case.bk, key), lift=lift, boot_lut_raw=braw_lut)


def _run_ct_raw(case, c, a, b, flags):
    """sgfhe_circuit_run_ct_ex through the C ABI on sentinel-filled outputs -> (rc, w, v, lwe)."""
    p = case.params
    L = case.S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    w = np.full((c.n_outputs, BLOCKS, p.m), SENTINEL, dtype=np.uint64)
    v = np.full_like(w, SENTINEL)
    lwe = np.full((c.n_outputs, BLOCKS * p.n, p.n + 1), SENTINEL, dtype=np.uint64)
    rc = L.sgfhe_circuit_run_ct_ex(case.eng._h, c.handle(), BLOCKS, ptr(a), ptr(b), a.shape[2], ptr(w), ptr(v), ptr(lwe), flags)
    return rc, w, v, lwe


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_mixed_circuit_ciphertext_form(case, rnd):
    """Two blocks, the inputs once of length n and once of length m (the same LWEs: one reference), flags 0, PACK_DIRECT
    and PACK_DIRECT | PACK_LIFT.  The LWE outputs are the bytes of the flags = 0 replay under every flag, every packed
    ciphertext equals the oracle's and decrypts to the plain evaluation."""
    if not case.mode(rnd):
        return
    S, p, eng = case.S, case.params, case.eng
    c = RC.mixed_circuit(S, "ct")
    bits, short, wide = ct_inputs(case)
    plain = c.evaluate_plain(bits.reshape(3, -1)).reshape(c.n_outputs, BLOCKS, p.n)
    try:
        lwe0 = None
        for direct, lift in FLAGS:
            flags = (1 if direct else 0) | (2 if lift else 0)
            if not case.rg.pack[bool(rnd)]:
                case.mode(rnd)
                rc, w, v, lwe = _run_ct_raw(case, c, short[0], short[1], flags)
                assert rc == RC.ERR_UNSUPPORTED
                assert (w == SENTINEL).all() and (v == SENTINEL).all() and (lwe == SENTINEL).all()
                continue
            (rw, rv), rlwe = ct_reference(case, c, short[0], short[1], rnd, direct, lift)
            if lwe0 is None:                       # the rule's condition, on the oracle's replay
                lwe0 = rlwe
                assert np.array_equal(_decrypt(case, rlwe), plain.reshape(c.n_outputs, -1))
            assert np.array_equal(rlwe, lwe0)
            for q in range(c.n_outputs * BLOCKS):
                assert np.array_equal(S.host.decrypt_rlwe(p, case.sk, rw.reshape(-1, p.m)[q], rv.reshape(-1, p.m)[q]),
                                      plain.reshape(-1, p.n)[q]), (direct, lift, q)
            for a, b in (short, wide):
                case.mode(rnd)
                (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=direct, lift=lift)
                where = (direct, lift, a.shape[2])
                assert np.array_equal(lwe, rlwe), where
                assert np.array_equal(w, rw) and np.array_equal(v, rv), where
    finally:
        eng.set_random_flatten(False)


# ---- noise ---------------------------------------------------------------------------------------------------------------

def _zq_rows(case, errors, bits, rng):
    """Rows [count][n + 1][2] over Z_Q with phase bit 2 DQ_tilde + e exactly; a holds uniform residues, 0 and Q - 1."""
    p = case.params
    n, Q = p.n, p.Q
    s = [int(x) & 1 for x in case.sk]
    out = np.zeros((len(errors), n + 1, 2), dtype=np.uint64)
    for t, (e, bit) in enumerate(zip(errors, bits)):
        a = [int.from_bytes(rng.bytes(16), "little") % Q for _ in range(n)]
        a[t % n], a[(t + 3) % n] = Q - 1, 0
        vals = a + [(sum(x for x, k in zip(a, s) if k) + int(bit) * 2 * p.DQ_tilde + e) % Q]
        out[t, :, 0] = [x & 0xFFFFFFFFFFFFFFFF for x in vals]
        out[t, :, 1] = [x >> 64 for x in vals]
    return out


def test_lwe_noise_primitive(case):
    """17 rows (one full tile of 16 and a ragged one) with chosen errors, over Z_r and over Z_Q: 0, +-1, the margin and
    wrong thresholds, the wrap -- over Z_Q the neighbours of +-Q/2 and +-DQ_tilde exactly -- against Python integers."""
    S, p, eng = case.S, case.params, case.eng
    assert case.mode(False)
    Dr, r, Q, DQ = p.r // 4, p.r, p.Q, p.DQ_tilde
    rng = np.random.default_rng(530 + p.n)
    bits = rng.integers(0, 2, size=17).astype(np.uint8)
    errs = NR.boundary_errors(p) + [r // 2 - 1, -(r // 2 - 1), Dr // 4 + 1, 2, -2, -(Dr // 4 - 1)]
    assert len(errs) == 17
    rows = NR.handmade_zr(p, case.sk, rng, errs, bits)
    want = NR.record_zr(p, case.sk, rows, bits)
    assert want[2] == r // 2 and want[3] == sum(errs) and want[4] == sum(e * e for e in errs)
    assert eng.lwe_noise(case.sk, rows, bits) == S.NoiseStats(*want)
    assert eng.lwe_noise(case.sk, rows[:16], bits[:16]) == S.NoiseStats(*NR.record_zr(p, case.sk, rows[:16], bits[:16]))
    half = Q // 2
    assert Q % 2 == 1                             # (so -(Q - 1) / 2 .. (Q - 1) / 2 are the centred errors)
    errs_q = [0, 1, -1, DQ, -DQ, DQ - 1, -(DQ - 1), DQ + 1, half, half - 1, -half, -(half - 1), 2 * DQ, DQ // 2,
              -(DQ // 2), 3, -3]
    assert len(errs_q) == 17
    raw = _zq_rows(case, errs_q, bits, rng)
    assert NR.errors_zq(p, case.sk, raw, bits) == errs_q
    want = NR.record_zq(p, case.sk, raw, bits)
    assert want == (17, sum(abs(e) >= DQ for e in errs_q), half, sum(abs(e) for e in errs_q))
    assert eng.lwe_noise(case.sk, raw, bits, raw=True) == S.NoiseStatsQ(*want)
    for t in (4, 8, 10):                          # +-DQ_tilde, +Q/2 and -Q/2 as single rows
        assert eng.lwe_noise(case.sk, raw[t], bits[t:t + 1], raw=True) == \
            S.NoiseStatsQ(*NR.record_zq(p, case.sk, raw[t:t + 1], bits[t:t + 1])), t


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_circuit_probe_every_wire(case, rnd):
    """sgfhe_circuit_run_probe of the mixed circuit: `out` has the bytes of the oracle replay, and the record of every wire
    -- the inputs, all three wires of every node, read or not -- equals the statistics of the replay's rows in Python
    integers, a scaled wire against its own codeword.  No row is wrong (the rule's condition holds: lwe_reference)."""
    from sgfhe_jl_amd import circuit as C
    if not case.mode(rnd):
        return
    S, p = case.S, case.params
    c = RC.mixed_circuit(S, "lwe")
    bits, inputs = lwe_inputs(case)
    ref = lwe_reference(case, c, inputs, bits, rnd)
    # every wire at once: the same nodes (all live in `c` too, so rows and calls are the same) with every wire an output
    d = S.Circuit(3, group=4)
    d.gates, d.gate_shifts = list(c.gates), list(c.gate_shifts)
    d.gate_weights, d.gate_tables = dict(c.gate_weights), dict(c.gate_tables)
    d.outputs = list(range(3 + 3 * c.n_gates))
    d.output_shifts = [0] * len(d.outputs)
    assert d.schedule() == c.schedule() and sum(len(level) for level in c.schedule()) == c.n_gates
    boot, boot_lut = LR.oracle_boots(case.o, case.lo, case.bkey, p, _key(rnd))
    wires = C.replay_levels(d, inputs, p.r, boot, boot_lut)
    plain = d.evaluate_plain(bits)
    try:
        out, stats = case.eng.circuit_probe(c, inputs, case.sk, bits)
    finally:
        case.eng.set_random_flatten(False)
    assert np.array_equal(out, ref)
    assert len(stats) == len(d.outputs)
    Dr = p.r // 4
    for w in d.outputs:
        g, k = divmod(w - 3, 3)
        scale = k if w >= 3 and c.kind(g) == "lut" else 0
        if scale == 0:
            want = NR.record_zr(p, case.sk, wires[w], plain[w])
        else:
            e = [int(x) for x in LR.phase_errors(p, case.sk, wires[w], plain[w], scale)]
            Cw = Dr >> scale
            want = (len(e), sum(abs(x) >= Cw // 2 for x in e), max(abs(x) for x in e), sum(e), sum(x * x for x in e),
                    sum(abs(x) >= Cw // 4 for x in e))
        assert stats[w] == S.NoiseStats(*want), (w, stats[w], want)
        assert stats[w].rows == INSTANCES and stats[w].wrong == 0, w


# ---- NOT over Z_Q with the codeword past Q -------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["just past Q/2", "Q - 1"])
def test_direct_not_reduces_the_codeword(S, oc, where):
    """The ctx accepts any DQ_tilde < Q, so the codeword 2 DQ_tilde of NOT over Z_Q may be past Q.  k_circ_scatter_raw
    subtracts from its residue, as k_lwe_noise_q and circuit.lwe_not_modq do: on the `tiny` ring at DQ_tilde =
    floor(Q/2) + 1 (un-reduced, only b in {0, 1, 2} would leave the residues) and at DQ_tilde = Q - 1 (un-reduced, every
    b but Q - 1 would) the negated direct outputs pack to the oracle's ciphertexts.  Bytes only: such a ring decrypts
    nothing."""
    from sgfhe_jl_amd import circuit as C
    base = RC.ring(S, "tiny")
    Q = base.params.Q
    params = S.Params.custom(base.params.n, Q, base.params.B, DQ_tilde=Q // 2 + 1 if where == "just past Q/2" else Q - 1)
    assert Q <= 2 * params.DQ_tilde and params.DQ_tilde < Q
    n = params.n
    o = oc.Oracle.from_params(params)
    sk = o.private_key(451)
    bkey = o.bootstrap_key(sk, 452, noise=base.noise)
    c = S.Circuit(2)
    g = c.gate(*c.inputs)
    c.output(~g[0], g[1], ~g[2])
    rng = np.random.default_rng(453)
    a = rng.integers(0, params.r, size=(2, 1, n), dtype=np.uint64)
    b = rng.integers(0, params.r, size=(2, 1, n), dtype=np.uint64)
    (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, R.oracle_boot(o, bkey, None),
                                        R.oracle_tail(R.bigint_params(params), R.key_lists(oc, bkey, n, params.m), None))
    eng = S.Engine(params)
    try:
        eng.upload_key(bkey)
        assert eng.kernel_names() == base.kernels[False]
        (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True)
        assert np.array_equal(lwe, rlwe)
        assert np.array_equal(w, rw) and np.array_equal(v, rv)
    finally:
        eng.close()
