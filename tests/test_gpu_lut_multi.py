"""LUT families on the device: several truth tables on one bootstrap's accumulator (sgfhe_bootstrap_lut_multi_batch,
include/sgfhe_hip.h).  Every word of out[:, j] against `lut_ref.rows_from_acc` on the accumulators of the low-amplitude
C oracle for tables[:, j] -- an independent reference --, in both flatten modes, reduced and un-reduced, in every
chunk, lane and small-batch form; against the single-table call of the same ctx; the call numbering of the draw
stream; the argument errors; Params(1024); the other ring kinds of tests/ring_cases.py.  The rows are those of
tests/test_gpu_lut.py: made from the secret key with sums s = 0..7 and errors up to +-(Dr/8 - 1).
Circuits (sgfhe_circuit_create_lut_multi): circuit_run against circuit.replay_levels driven by a second ctx's
single-table primitives, which the tests above and tests/test_gpu_lut.py hold to the oracles (deterministic: the
replay makes several primitive calls per level call, so only there do a second ctx's call numbers fit), and by the
oracles themselves in the randomised mode -- families of 2, 8 and 256 members with dead siblings, a level cut by a call
boundary inside a leader's rows, a lane-shifted family, the ciphertext form under all three flag sets, the probe, the
plan with one LUT node per table, the PRESENT S-box through circuit.shannon, Params(1024) on a clone."""

import ctypes

import numpy as np
import pytest

import lut_ref as LR
import ring_cases as RC

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5
RAW_MODQ, RAW_RNS2 = 1, 2
SEED = 0x5EED
NAMED = (0x00, 0xFF, 0x96, 0xE8, 0xCA, 0xF0, 0x10, 0xAA)
# batch -> tables per row: 5 x 256 is every table on every row in the small-batch form; 40 is above the small-batch
# maximum and no multiple of 8; 264 runs with set_chunk(64) as several chunks on both lanes
SHAPES = {5: 256, 40: 3, 264: 8}


def family_tables(batch, T):
    """[batch][T]: all 256 tables on every row, rotated by the row, at T = 256; else the named tables (the constants,
    parity, majority, the mux among them) rotated by the row in the first columns and random ones behind them -- a row
    may hold a table twice."""
    t = np.arange(batch)[:, None]
    j = np.arange(T)[None, :]
    if T == 256:
        return ((t + j) % 256).astype(np.uint8)
    rnd = np.random.default_rng(600 + batch).integers(0, 256, size=(batch, T))
    named = np.array(NAMED)[(t + j) % 8]
    return np.where(j < min(T, 4), named, rnd).astype(np.uint8)


def reference_rows(params, acc, tables):
    """What lut_ref.rows_from_acc gives column by column, reduced and raw from one pass over its own arithmetic
    (lut_ref.base_lwe, then 4, 2, 1 times the base word mod Q and lut_ref.modred): ([batch][T][3][n + 1],
    [batch][T][3][n + 1][2])."""
    n, Q = params.n, params.Q
    batch, T = tables.shape
    red = np.zeros((batch, T, 3, n + 1), dtype=np.uint64)
    raw = np.zeros((batch, T, 3, n + 1, 2), dtype=np.uint64)
    for t in range(batch):
        pa = [int(lo) | (int(hi) << 64) for lo, hi in acc[t, 0]]
        pb = [int(lo) | (int(hi) << 64) for lo, hi in acc[t, 1]]
        for j in range(T):
            alpha, beta = LR.base_lwe(params, pa, pb, int(tables[t, j]))
            for k in range(3):
                vs = [(w << (2 - k)) % Q for w in alpha + [beta]]
                red[t, j, k] = [LR.modred(v, params) for v in vs]
                raw[t, j, k, :, 0] = [v & 0xFFFFFFFFFFFFFFFF for v in vs]
                raw[t, j, k, :, 1] = [v >> 64 for v in vs]
    return red, raw


class _Case:
    """Params(64): key, engine and the low-amplitude oracle, once for the module."""

    def __init__(self, S, oc):
        self.params = S.Params(64)
        self.o = oc.Oracle.from_params(self.params)
        self.lo = LR.low_oracle(oc, self.params)
        self.sk = self.o.private_key(301)
        self.bkey = self.o.bootstrap_key(self.sk, 302)
        self.eng = S.Engine(self.params)
        self.eng.upload_key(self.bkey)
        self._ref = {}

    def rows(self, batch):
        """The rows of test_gpu_lut's _Case.rows: sum (t + t div 8) mod 8, error cycling through 0, +-(Dr/8 - 1) and
        values between.  -> a, b, tables [batch][T], the wanted bits [batch][T]."""
        lim = self.params.r // 32 - 1
        errs = (lim, -lim, 0, 1, -1, lim // 2, -(lim // 3))
        t = np.arange(batch)
        s = (t + t // 8) % 8
        e = np.array([errs[i % len(errs)] for i in t])
        a, b = LR.rows_at(self.params, self.sk, s, e, np.random.default_rng(310 + batch))
        tables = family_tables(batch, SHAPES[batch])
        want = (tables.astype(np.int64) >> s[:, None]) & 1
        return a, b, tables, want

    def acc(self, batch, rnd, call=0):
        a, b, _, _ = self.rows(batch)
        _, acc = self.lo.bootstrap_batch(self.bkey, a, b, np.zeros_like(a), np.zeros_like(b), want_acc=True,
                                         rnd=(SEED, call) if rnd else None)
        return acc

    def reference(self, batch, rnd, raw):
        """As call 0 of the draw stream: computed once, shared."""
        key = (batch, rnd)
        if key not in self._ref:
            self._ref[key] = reference_rows(self.params, self.acc(batch, rnd), self.rows(batch)[2])
        return self._ref[key][1 if raw else 0]


_CASE = []


@pytest.fixture(scope="module")
def case(S, oc):
    if not _CASE:
        _CASE.append(_Case(S, oc))
    yield _CASE[0]


def _mode(eng, rnd):
    eng.set_random_flatten(bool(rnd), SEED)       # (the call counter starts again at 0)


@pytest.mark.parametrize("batch", sorted(SHAPES))
@pytest.mark.parametrize("rnd", [False, True], ids=["deterministic", "randomised"])
def test_primitive_equals_rows_from_acc(case, batch, rnd):
    """Reduced and raw, every word of every table; every row decrypts to its table entry at all three scales."""
    eng, params = case.eng, case.params
    a, b, tables, want = case.rows(batch)
    eng.set_chunk(64 if batch == 264 else 0)
    try:
        for raw in (False, True):
            _mode(eng, rnd)
            got = eng.bootstrap_lut_multi_batch(a, b, tables, raw=raw)
            assert got.shape == (batch, SHAPES[batch], 3, params.n + 1) + ((2,) if raw else ())
            assert np.array_equal(got, case.reference(batch, rnd, raw)), (batch, rnd, raw)
            if not raw:
                for k in range(3):
                    bits = LR.decrypt_scaled(params, case.sk, got[:, :, k], k).reshape(want.shape)
                    assert np.array_equal(bits, want), k
    finally:
        eng.set_chunk(0)
        eng.set_random_flatten(False)


@pytest.mark.parametrize("rnd", [False, True], ids=["deterministic", "randomised"])
def test_equals_the_single_table_call(case, rnd):
    """T = 1 is bootstrap_lut_batch; column j of a family call is bootstrap_lut_batch of tables[:, j] at the same call
    number of the same stream (the 40 x 3 rows, reduced and raw)."""
    eng = case.eng
    a, b, tables, _ = case.rows(40)
    try:
        for raw in (False, True):
            _mode(eng, rnd)
            multi = eng.bootstrap_lut_multi_batch(a, b, tables, raw=raw)
            for j in range(tables.shape[1]):
                _mode(eng, rnd)
                single = eng.bootstrap_lut_batch(a, b, tables[:, j], raw=raw)
                assert np.array_equal(multi[:, j], single), (j, raw)
                _mode(eng, rnd)
                one = eng.bootstrap_lut_multi_batch(a, b, tables[:, j:j + 1], raw=raw)
                assert np.array_equal(one[:, 0], single), (j, raw)
    finally:
        eng.set_random_flatten(False)


@pytest.mark.parametrize("rnd", [False, True], ids=["deterministic", "randomised"])
def test_chunk_lane_and_small_batch_forms_give_the_same_bytes(S, case, rnd):
    """The 264 x 8 rows on a second ctx under set_lanes(1), set_chunk(8) and set_small_batch_max(0), each alone."""
    a, b, tables, _ = case.rows(264)
    eng = S.Engine(case.params)
    eng.upload_key(case.bkey)
    try:
        for raw in (False, True):
            ref = case.reference(264, rnd, raw)
            for knob, on, off in ((eng.set_lanes, 1, 2), (eng.set_chunk, 8, 0)):
                knob(on)
                _mode(eng, rnd)
                assert np.array_equal(eng.bootstrap_lut_multi_batch(a, b, tables, raw=raw), ref), (knob.__name__, raw)
                knob(off)
        eng.set_small_batch_max(0)                 # (last: the ctx is closed below)
        for raw in (False, True):
            _mode(eng, rnd)
            assert np.array_equal(eng.bootstrap_lut_multi_batch(a, b, tables, raw=raw), case.reference(264, rnd, raw))
            _mode(eng, rnd)
            assert np.array_equal(eng.bootstrap_lut_multi_batch(a[:5], b[:5], tables[:5], raw=raw),
                                  case.reference(264, rnd, raw)[:5])
    finally:
        eng.close()


def test_one_call_number_per_call(case):
    """Randomised mode: a family call of 256 tables is call 0, the bootstrap_batch call after it the oracle's call 1,
    the family call after that call 2 of the stream."""
    eng, params, o, lo = case.eng, case.params, case.o, case.lo
    a, b, tables, _ = case.rows(5)
    bits = np.array([0, 1, 1, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    ga, gb = o.lwe_encrypt_bits(case.sk, bits, 320)
    _mode(eng, True)
    try:
        first = eng.bootstrap_lut_multi_batch(a, b, tables)
        gate = eng.bootstrap_batch(ga[0::2], gb[0::2], ga[1::2], gb[1::2])
        third = eng.bootstrap_lut_multi_batch(a, b, tables[:, :8])
    finally:
        eng.set_random_flatten(False)
    assert np.array_equal(first, case.reference(5, True, False))
    assert np.array_equal(gate, o.bootstrap_batch(case.bkey, ga[0::2], gb[0::2], ga[1::2], gb[1::2], rnd=(SEED, 1)))
    assert np.array_equal(third, reference_rows(params, case.acc(5, True, call=2), tables[:, :8])[0])
    assert not np.array_equal(third, first[:, :8])


def test_argument_errors_write_nothing(S, case):
    params, n, r = case.params, case.params.n, case.params.r
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    a, b, tables, _ = case.rows(5)
    T = tables.shape[1]
    out = np.full((5, T + 1, 3, n + 1, 2), SENTINEL, dtype=np.uint64)
    h = case.eng._h
    INVALID, NO_KEY = -1, -5                   # SGFHE_ERR_INVALID_ARG, SGFHE_ERR_NO_KEY
    assert L.sgfhe_bootstrap_lut_multi_batch(None, None, None, None, 1, 0, None, 0) == INVALID      # (a NULL ctx)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[4, n - 1] = r
    bad_b[2] = r
    calls = [(bad_a, b, tables, T, out, 0), (a, bad_b, tables, T, out, RAW_MODQ), (None, b, tables, T, out, 0),
             (a, None, tables, T, out, 0), (a, b, None, T, out, 0), (a, b, tables, T, None, 0),
             (a, b, tables, T, out, RAW_MODQ | RAW_RNS2), (a, b, tables, T, out, RAW_RNS2), (a, b, tables, T, out, 4),
             (a, b, tables, T, out, 0x80000000), (a, b, tables, 0, out, 0), (a, b, tables, 257, out, 0),
             (a, b, tables, 257, out, RAW_MODQ)]
    for xa, xb, xt, nt, xo, flags in calls:
        rc = L.sgfhe_bootstrap_lut_multi_batch(h, ptr(xa) if xa is not None else None, ptr(xb) if xb is not None else None,
                                               ptr(xt) if xt is not None else None, nt, 5,
                                               ptr(xo) if xo is not None else None, flags)
        assert rc == INVALID and np.all(out == SENTINEL), (nt, flags)
    assert L.sgfhe_bootstrap_lut_multi_batch(h, ptr(bad_a), ptr(b), ptr(tables), T, 0, ptr(out), 0) == 0
    assert np.all(out == SENTINEL)
    fresh = S.Engine(params)
    try:
        rc = L.sgfhe_bootstrap_lut_multi_batch(fresh._h, ptr(a), ptr(b), ptr(tables), T, 5, ptr(out), 0)
        assert rc == NO_KEY and np.all(out == SENTINEL)
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        case.eng.bootstrap_lut_multi_batch(a, b, np.zeros((5, 257), dtype=np.uint8))
    with pytest.raises(ValueError):
        case.eng.bootstrap_lut_multi_batch(a, b, tables[:, 0])
    # the ctx is as it was: the next call is the reference's
    _mode(case.eng, False)
    assert np.array_equal(case.eng.bootstrap_lut_multi_batch(a, b, tables), case.reference(5, False, False))


def test_params_1024(S, oc, gpu_keys):
    """8 rows x 8 tables at Params(1024) in both modes against the oracle's accumulators, as test_gpu_lut's
    test_params_1024: row t carries the eight tables rotated by t."""
    from conftest import oracle_threads
    params, o, sk, eng = gpu_keys.engine(1024)
    khat = gpu_keys.khat(1024)
    lo = LR.low_oracle(oc, params)
    T = oracle_threads()
    lim = params.r // 32 - 1
    s = np.arange(8)
    e = np.array([lim, -lim, 0, 1, -1, lim // 2, -(lim // 3), lim])
    eight = np.array([0x96, 0xE8, 0xCA, 0x10, 0xFF, 0x00, 0x55, 0x7F], dtype=np.uint8)
    tables = eight[(np.arange(8)[:, None] + np.arange(8)[None, :]) % 8]
    want = (tables.astype(np.int64) >> s[:, None]) & 1
    a, b = LR.rows_at(params, sk, s, e, np.random.default_rng(330))
    z = np.zeros_like(a), np.zeros_like(b)
    try:
        for rnd in (False, True):
            _, acc = lo.bootstrap_batch(khat, a, b, z[0], z[1], want_acc=True, opt=True, threads=T,
                                        rnd=(SEED, 0) if rnd else None)
            ref = reference_rows(params, acc, tables)
            for raw in (False, True):
                _mode(eng, rnd)
                got = eng.bootstrap_lut_multi_batch(a, b, tables, raw=raw)
                assert np.array_equal(got, ref[1 if raw else 0]), (rnd, raw)
                if not raw:
                    for k in range(3):
                        bits = LR.decrypt_scaled(params, sk, got[:, :, k], k).reshape(want.shape)
                        assert np.array_equal(bits, want), (rnd, k)
    finally:
        eng.set_random_flatten(False)


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_other_ring_kinds(S, oc, name, rnd):
    """Twelve rows x 8 tables on every other ring kind (the two-limb and the four-limb moduli, the composite one with
    its key as limb pairs, m = 128) against the single-table call of the same ctx, which tests/test_gpu_rings.py holds
    to the oracle: the small-batch form and, with set_small_batch_max(0), the throughput form; reduced and raw."""
    rg = RC.ring(S, name)
    p = rg.params
    o, _ = RC.oracles(oc, rg)
    sk = o.private_key(701)
    bkey = o.bootstrap_key(sk, 702, noise=rg.noise)
    eng = S.Engine(p)
    try:
        RC.upload(eng, rg, bkey)
        if not RC.set_mode(S, eng, rg, rnd):
            return
        lim = p.r // 32 - 1
        t = np.arange(12)
        s = (t + t // 8) % 8
        e = np.array([(0, 1, -1, lim, -lim)[i % 5] for i in t])
        a, b = LR.rows_at(p, sk, s, e, np.random.default_rng(710 + p.n))
        tables = family_tables(12, 8)
        for small in (24, 0):
            eng.set_small_batch_max(small)
            for raw in (False, True):
                RC.set_mode(S, eng, rg, rnd)
                got = eng.bootstrap_lut_multi_batch(a, b, tables, raw=raw)
                for j in range(8):
                    RC.set_mode(S, eng, rg, rnd)
                    assert np.array_equal(got[:, j], eng.bootstrap_lut_batch(a, b, tables[:, j], raw=raw)), (small, raw, j)
    finally:
        eng.close()


# ---- LUT families in circuits (sgfhe_circuit_create_lut_multi) ------------------------------------------------------

KEY32 = bytes(range(1, 33))
PRESENT = (0xC, 5, 6, 0xB, 9, 0, 0xA, 0xD, 3, 0xE, 0xF, 8, 4, 7, 1, 2)


def _circuit_setup(S, oc, seed, engines=1):
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
    import noise_ref as NR
    rng = np.random.default_rng(seed)
    flat = np.asarray(bits).reshape(-1)
    e = rng.integers(-(params.r // 64), params.r // 64 + 1, size=flat.size)
    return NR.handmade_zr(params, sk, rng, e, flat).reshape(np.asarray(bits).shape + (params.n + 1,))


def _decrypt0(params, sk, lwe):
    return LR.decrypt_scaled(params, sk, lwe, 0).reshape(lwe.shape[:-1]).astype(bool)


def _second_ctx(ref):
    """(boot, boot_lut) of replay_levels on a second ctx's primitives, deterministic mode."""
    return (lambda call, *lwe: ref.bootstrap_batch(*lwe),
            lambda call, a, b, t, idx: ref.bootstrap_lut_batch(a, b, t))


def _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits, rnd_instances=None):
    """Deterministic: circuit_run equals replay_levels on the second ctx's single-table primitives.  Randomised: on the
    two oracles, over the first rnd_instances instances (all by default, none at 0).  Both decrypt to evaluate_plain."""
    from sgfhe_jl_amd import circuit as C
    plain = c.evaluate_plain(bits)
    eng.set_random_flatten(False)
    ref.set_random_flatten(False)
    got = eng.circuit_run(c, inputs)
    assert np.array_equal(got, C.replay_levels(c, inputs, params.r, *_second_ctx(ref))), "deterministic"
    assert np.array_equal(_decrypt0(params, sk, got), plain)
    ri = inputs.shape[1] if rnd_instances is None else rnd_instances
    if not ri:
        return got
    boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, KEY32)
    want = C.replay_levels(c, inputs[:, :ri], params.r, boot, boot_lut)
    eng.set_random_flatten(True, KEY32)
    try:
        rnd = eng.circuit_run(c, inputs[:, :ri])
    finally:
        eng.set_random_flatten(False)
    assert np.array_equal(rnd, want), "randomised"
    assert np.array_equal(_decrypt0(params, sk, rnd), plain[:, :ri])
    return got


def _family_circuit(S):
    """Three inputs through refresh, then fan; families of 2, 8 and 256 members on the fanned wires (with a NOT on a
    different position each); a second LUT level reads sibling wires at all three scales, one of its nodes a family
    again; a classic gate beside the fans.  Of the 256 only four siblings are live, of the 8 three; the leader of the
    family of 2 is live through its sibling alone."""
    c = S.Circuit(3)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    g2 = c.gate(rx, ~ry)
    A = c.lut_multi([0x96, 0xE8], fx[2], fy[1], fz[0])
    t8 = [int(t) for t in np.random.default_rng(801).integers(0, 256, size=8)]
    B = c.lut_multi(t8, ~fx[2], fy[1], fz[0])
    t256 = [(t + 77) % 256 for t in range(256)]
    Cc = c.lut_multi(t256, fx[2], ~fy[1], fz[0])
    D = c.lut(0xCA, A[1][2], B[3][1], Cc[200][0])
    E = c.lut_multi([0x96, 0x17], Cc[17][2], ~Cc[255][1], B[7][0])
    c.output(D[0], E[0][0], E[1][0], A[1][0], ~B[5][0], Cc[3][0], g2[0], ~E[1][0])
    return c


def test_family_circuit(S, oc):
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 811, engines=2)
    try:
        c = _family_circuit(S)
        assert c.n_gates == 7 + 2 + 8 + 256 + 1 + 2
        # bootstraps: 3 refreshes, 3 fans and a gate, three leaders, a LUT node and a leader
        assert [len(l) for l in c.schedule()] == [3, 4, 3, 2]
        assert c.info() == dict(levels=4, nodes=12, widest=4, slots=c.info()["slots"])
        assert len(c.live_siblings(9)) == 3 and len(c.live_siblings(17)) == 4 and c.live_siblings(7) == [8]
        bits = np.array([[(i >> k) & 1 for i in range(8)] for k in range(3)], dtype=bool)
        inputs = _inputs(params, sk, bits, 812)
        _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits)
    finally:
        eng.close()
        ref.close()


def test_all_256_siblings_live(S, oc):
    """Every member of a family of 256 is an output: the bits of all 256 tables at once, from three bootstrap levels
    (deterministic; test_family_circuit holds a family of 256 to the oracles in the randomised mode)."""
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 821, engines=2)
    try:
        c = S.Circuit(3)
        fx, fy, fz = (c.fan(c.refresh(w)) for w in c.inputs)
        fam = c.lut_multi(list(range(256)), fx[2], fy[1], fz[0])
        c.output(*[t[0] for t in fam])
        assert c.info()["nodes"] == 7 and c.info()["levels"] == 3
        bits = np.array([[(i >> k) & 1 for i in range(8)] for k in range(3)], dtype=bool)
        inputs = _inputs(params, sk, bits, 822)
        got = _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits, rnd_instances=0)
        want = np.array([[(t >> s) & 1 for s in range(8)] for t in range(256)], dtype=bool)
        assert np.array_equal(_decrypt0(params, sk, got), want)
    finally:
        eng.close()
        ref.close()


def test_call_boundary_inside_a_family_leader(S, oc):
    """42 row-taking nodes x 200 instances = 8400 rows in one level, above SGFHE_CIRCUIT_CALL_ROWS = 8192: the boundary
    falls inside rank 40, the leader of a family of three; rank 17 is a plain LUT node, every fifth other node a sum
    node, the rest classic.  Deterministic: every word against replay_levels on a second
    ctx's primitives.  Randomised: a row's draws depend on its call and its index in the call alone, so the oracles run
    every LUT row and every sibling's, every row of the second call and every 16th row of the first, at their own
    indices, and those rows are compared."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 831, engines=2)
    n = params.n
    try:
        inst = 200
        fams = {17: [0xCA], 40: [0x1B, 0xE8, 0x69]}
        c = S.Circuit(2)
        x, y = c.inputs
        outs, full = [], []          # full: outputs whose every row the randomised check compares
        for k in range(42):
            if k in fams:            # (inputs straight into a LUT node: bytes are compared, not bits)
                for t in c.lut_multi(fams[k], S.Circuit.FALSE, S.Circuit.FALSE, ~x if k == 17 else y):
                    full.append(len(outs))
                    outs.append(t[0])
            elif k % 5 == 0:
                outs.append(c.sum_node([(1, x), (1, y if k % 2 else ~y)])[0])
            else:
                outs.append(c.gate(x, ~y if k % 2 else y)[k % 3])
        c.output(*outs)
        ranks = c.schedule()[0]
        assert len(c.schedule()) == 1 and len(ranks) == 42 and c.info()["nodes"] == 42 and c.n_gates == 44
        assert c.kind(ranks[40]) == "lut" and len(c.siblings(ranks[40])) == 2
        assert 40 * inst < C.CALL_ROWS < 41 * inst
        bits = np.random.default_rng(832).integers(0, 2, size=(2, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 833)
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(got, C.replay_levels(c, inputs, params.r, *_second_ctx(ref)))
        # randomised
        khat = o.key_transform(bkey)
        _, boot_lut = LR.oracle_boots(o, lo, bkey, params, KEY32)
        picked = np.zeros(42 * inst, dtype=bool)

        def boot(call, a1, b1, a2, b2):
            rows = np.arange(len(b1))
            sel = rows[(rows % 16 == 5) | (call == 1)]
            picked[call * C.CALL_ROWS + sel] = True
            res = np.zeros((len(b1), 3, n + 1), dtype=np.uint64)
            res[sel] = o.bootstrap_batch(khat, a1[sel], b1[sel], a2[sel], b2[sel], opt=True,
                                         rnd=(KEY32, call, sel.astype(np.uint32)))
            return res

        want = C.replay_levels(c, inputs, params.r, boot, boot_lut)
        picked = picked.reshape(42, inst)
        # by output: the rows of its producing rank, every row where the output is a LUT or sibling wire
        rank_of_output = []
        for k in range(42):
            rank_of_output += [k] * (len(fams[k]) if k in fams else 1)
        sel = np.stack([picked[k] for k in rank_of_output])
        sel[full] = True
        assert sel[full].all() and sel.sum() > 1300 and not sel.all()
        eng.set_random_flatten(True, KEY32)
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(got[sel], want[sel])
    finally:
        eng.set_random_flatten(False)
        eng.close()
        ref.close()


def test_lane_shifted_family(S, oc):
    """group = 4: a family reads lane-shifted scaled wires (a negated scale-1 reference that leaves the group fills with
    TRUE at scale 1), and a later node reads lane-shifted sibling wires."""
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 841, engines=2)
    try:
        c = S.Circuit(2, group=4)
        fx, fy = (c.fan(c.refresh(w)) for w in c.inputs)
        fam = c.lut_multi([0xCA, 0x96, 0x2D], fx[2].lane(1), ~fy[1].lane(-1), fx[0].lane(2))
        b = c.lut(0x96, ~fam[1][2].lane(-3), fam[2][1], ~fam[0][0].lane(3))
        c.output(fam[1][0], b[0], ~fam[2][0].lane(1))
        assert c.info()["nodes"] == 6
        bits = np.random.default_rng(842).integers(0, 2, size=(2, 8)).astype(bool)
        inputs = _inputs(params, sk, bits, 843)
        _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits)
    finally:
        eng.close()
        ref.close()


def test_ciphertext_form(S, oc):
    """One block; outputs: sibling wires +0 (one negated) and a classic gate wire.  flags 0 (randomised) against
    replay_ct, PACK_DIRECT (deterministic) and PACK_DIRECT | PACK_LIFT (randomised) against
    replay_ct_direct: the family's outputs are refreshed or lifted, the gate output is direct -- so the call of level 2,
    which holds the family, runs un-reduced, and the siblings' wires reach the wire table as ModRed words all the same;
    all decrypt."""
    import pack_direct_ref as R
    import pack_lift_ref as PL
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 851)
    n = params.n
    try:
        c = S.Circuit(2)
        x, y = c.inputs
        fx, fy = c.fan(x), c.fan(y)
        g = c.gate(x, ~y)
        fam = c.lut_multi([0xCA, 0x96, 0x53], fx[2], ~fy[1], fx[0])
        g2 = c.gate(x, y)
        g3 = c.gate(g[0], ~g2[1])                  # level 2, beside the family: its direct output leaves the call raw
        c.output(fam[1][0], ~fam[2][0], g3[0])     # (the leader is live through its siblings alone)
        assert [len(l) for l in c.schedule()] == [4, 2]
        bits = np.random.default_rng(852).integers(0, 2, size=(2, 1, n)).astype(bool)
        plain = c.evaluate_plain(bits.reshape(2, -1))
        a, b = PL.craft_cts(S, params, sk, bits, 853)
        bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
        khat = o.key_transform(bkey)

        def dec(w, v):
            return np.stack([S.host.decrypt_rlwe(params, sk, w[q, 0], v[q, 0]) for q in range(w.shape[0])])

        for key in (None, KEY32):
            boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, key)
            pack = lambda call, pa, pb: tuple(np.stack(x) for x in zip(*[
                o.pack_encrypted_bits(bkey, pa[i], pb[i], khat=khat, rnd=(key, i, call) if key else None)
                for i in range(len(pa))]))
            eng.set_random_flatten(key is not None, key or 0)
            lwe = eng.circuit_run_ct(c, a, b, packed=False, lwe=True)
            if key is not None:
                (rw, rv), rlwe = C.replay_ct(c, a, b, params, boot, pack, boot_lut)
                eng.set_random_flatten(True, key)
                (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True)
                assert np.array_equal(lwe, rlwe) and np.array_equal(w, rw) and np.array_equal(v, rv), key
                assert np.array_equal(dec(w, v), plain)
            braw, braw_lut = LR.oracle_boots(o, lo, bkey, params, key, raw=True)
            for lift in ((False,) if key is None else (True,)):    # (direct deterministic, lifted randomised)
                (rw, rv), rlwe = C.replay_ct_direct(c, a, b, params, braw, R.oracle_tail(bp, bk, key), lift=lift,
                                                    boot_lut_raw=braw_lut)
                eng.set_random_flatten(key is not None, key or 0)
                (dw, dv), dlwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=True, lift=lift)
                assert np.array_equal(dlwe, lwe) and np.array_equal(rlwe, lwe), (key, lift)
                assert np.array_equal(dw, rw) and np.array_equal(dv, rv), (key, lift)
                assert np.array_equal(dec(dw, dv), plain)
        eng.set_random_flatten(False)
    finally:
        eng.close()


def _probe_circuit(S, tables):
    """A family on three fanned inputs.  Member 1 is read at every scale (an output, and two positions of a later LUT
    node), member 2 only through its wire +0 (an output), member 3 is dead; the leader is an output."""
    c = S.Circuit(3)
    fx, fy, fz = (c.fan(c.refresh(w)) for w in c.inputs)
    fam = c.lut_multi(tables, fx[2], ~fy[1], fz[0])
    later = c.lut(0xE8, fam[1][2], fam[1][1], fz[0])
    c.output(fam[0][0], fam[1][0], fam[2][0], later[0])
    return c, fam


def test_probe_measures_sibling_wires_that_have_a_slot(S, oc):
    """The record of a read sibling wire equals the record of the leader's wire in the circuit where that table is the
    leader's (exact integers, the same rows in the deterministic mode); a sibling wire nothing reads, and every wire of a
    dead sibling, has an all-zero record; `out` has the bytes of circuit_run."""
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 861)
    try:
        t = [0xCA, 0x96, 0x1B, 0xE8]
        c, fam = _probe_circuit(S, t)
        inst = 40
        bits = np.random.default_rng(862).integers(0, 2, size=(3, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 863)
        run = eng.circuit_run(c, inputs)
        out, stats = eng.circuit_probe(c, inputs, sk, bits)
        assert np.array_equal(out, run)
        assert np.array_equal(_decrypt0(params, sk, out), c.evaluate_plain(bits))
        zero = lambda st: (st.rows, st.wrong, st.max_abs, st.sum, st.sum_sq, st.margin) == (0,) * 6
        for member in (1, 2):
            # the same circuit with this member's table as the leader's: its leader's records
            order = [t[member]] + [x for i, x in enumerate(t) if i != member]
            d, dfam = _probe_circuit(S, order)
            _, dstats = eng.circuit_probe(d, inputs, sk, bits)
            for w in range(3):
                st, lead = stats[fam[member][w].id], dstats[dfam[0][w].id]
                assert lead.rows == inst and lead.wrong == 0
                if member == 1 or w == 0:
                    assert st == lead, (member, w, st, lead)
                else:
                    assert zero(st), (member, w, st)           # live sibling, wire unread: no slot, no rows
        assert all(zero(stats[fam[3][w].id]) for w in range(3))   # a dead sibling
        assert all(stats[fam[0][w].id].rows == inst for w in range(3))   # the leader: every wire, read or not
    finally:
        eng.close()


def _sbox_circuit(S, family):
    c = S.Circuit(4)
    tables = [sum(((PRESENT[x] >> bit) & 1) << x for x in range(16)) for bit in range(4)]
    c.output(*S.shannon(c, tables, c.inputs, refresh=True, family=family))
    return c


def test_family_plan_gives_the_bytes_of_one_node_per_table(S, oc):
    """Deterministic mode: the PRESENT S-box through shannon as one family and as one LUT node per cofactor -- the same
    bytes, 11 bootstraps per input against 18; all 16 inputs twice over, decrypted to the table."""
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 871)
    try:
        shared, single = _sbox_circuit(S, True), _sbox_circuit(S, False)
        assert shared.info()["nodes"] == 11 and single.info()["nodes"] == 18
        assert shared.info()["levels"] == single.info()["levels"] == 4
        xs = np.arange(32) % 16
        bits = np.array([(xs >> k) & 1 for k in range(4)], dtype=bool)
        inputs = _inputs(params, sk, bits, 872)
        got = eng.circuit_run(shared, inputs)
        assert np.array_equal(got, eng.circuit_run(single, inputs))
        dec = _decrypt0(params, sk, got)
        assert np.array_equal(sum(dec[k].astype(int) << k for k in range(4)), np.array(PRESENT)[xs])
        eng.set_random_flatten(True, KEY32)
        dec = _decrypt0(params, sk, eng.circuit_run(shared, inputs))
        assert np.array_equal(sum(dec[k].astype(int) << k for k in range(4)), np.array(PRESENT)[xs])
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_params_1024_sbox_on_a_clone(S, gpu_keys):
    """The PRESENT S-box through shannon at Params(1024), 16 instances, on a clone: the bytes of the original ctx, and
    the table."""
    params, o, sk, eng = gpu_keys.engine(1024)
    c = _sbox_circuit(S, True)
    xs = np.arange(16)
    bits = np.array([(xs >> k) & 1 for k in range(4)], dtype=bool)
    inputs = _inputs(params, sk, bits, 881)
    eng.set_random_flatten(False)
    want = eng.circuit_run(c, inputs)
    dec = _decrypt0(params, sk, want)
    assert np.array_equal(sum(dec[k].astype(int) << k for k in range(4)), np.array(PRESENT)[xs])
    clone = eng.clone()
    try:
        assert np.array_equal(clone.circuit_run(c, inputs), want)
    finally:
        clone.close()
