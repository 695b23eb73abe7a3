"""LUT bootstraps and LUT nodes on the device (sgfhe_bootstrap_lut_batch, sgfhe_circuit_create_lut;
include/sgfhe_hip.h).  The primitive: every word against `lut_ref.rows_from_acc` on the
accumulators of the low-amplitude C oracle, in both flatten modes, reduced and un-reduced, in every chunk, lane and
small-batch form; the call numbering of the draw stream; the argument errors; Params(1024).  Circuits: circuit_run
against circuit.replay_levels driven by the standard and the low-amplitude oracle -- a truth-table circuit, a level cut
by a call boundary, lane-shifted scaled wires, the ciphertext form, the probe, a plan on a clone.  The input rows are
made from the secret key with chosen sums s and errors |e| <= Dr/8 - 1."""

import ctypes

import numpy as np
import pytest

import lut_ref as LR

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5
RAW_MODQ, RAW_RNS2 = 1, 2
SEED = 0x5EED


class _Case:
    """Params(64): key, engine and the two oracles, once for the module."""

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
        """Row t: table t mod 256 (all 256 tables from batch 256 on, the named ones first below that), sum
        (t + t div 8) mod 8, error cycling through 0, +-(Dr/8 - 1) and values between."""
        lim = self.params.r // 32 - 1
        errs = (lim, -lim, 0, 1, -1, lim // 2, -(lim // 3))
        named = (0x00, 0xFF, 0x96, 0xE8, 0xCA, 0xF0, 0x10, 0xAA)
        t = np.arange(batch)
        tables = (t % 256).astype(np.uint8) if batch >= 256 else np.array([named[i % 8] for i in t], dtype=np.uint8)
        s = (t + t // 8) % 8
        e = np.array([errs[i % len(errs)] for i in t])
        a, b = LR.rows_at(self.params, self.sk, s, e, np.random.default_rng(310 + batch))
        want = (tables.astype(np.int64) >> s) & 1
        return a, b, tables, want

    def reference(self, batch, rnd, raw):
        """rows_from_acc of the low-amplitude oracle, as call 0 of the draw stream: computed once, shared."""
        key = (batch, rnd)
        if key not in self._ref:
            a, b, tables, _ = self.rows(batch)
            _, acc = self.lo.bootstrap_batch(self.bkey, a, b, np.zeros_like(a), np.zeros_like(b), want_acc=True,
                                             rnd=(SEED, 0) if rnd else None)
            self._ref[key] = (LR.rows_from_acc(self.params, acc, tables), LR.rows_from_acc(self.params, acc, tables, raw=True))
        return self._ref[key][1 if raw else 0]


_CASE = []


@pytest.fixture(scope="module")
def case(S, oc):
    if not _CASE:
        _CASE.append(_Case(S, oc))
    yield _CASE[0]


def _mode(eng, rnd):
    eng.set_random_flatten(bool(rnd), SEED)       # (the call counter starts again at 0)


@pytest.mark.parametrize("batch", [5, 40, 264])
@pytest.mark.parametrize("rnd", [False, True], ids=["deterministic", "randomised"])
def test_primitive_equals_rows_from_acc(case, batch, rnd):
    """Batch 5 runs in the small-batch form, 40 is above its maximum and no multiple of 8, 264 carries all 256 tables
    plus 8 and runs with set_chunk(64) as several chunks on both lanes.  Reduced and raw, every word; every row
    decrypts to its table entry at all three scales."""
    eng, params = case.eng, case.params
    a, b, tables, want = case.rows(batch)
    eng.set_chunk(64 if batch == 264 else 0)
    try:
        for raw in (False, True):
            _mode(eng, rnd)
            got = eng.bootstrap_lut_batch(a, b, tables, raw=raw)
            assert np.array_equal(got, case.reference(batch, rnd, raw)), (batch, rnd, raw)
            if not raw:
                for k in range(3):
                    assert np.array_equal(LR.decrypt_scaled(params, case.sk, got[:, k], k), want), k
    finally:
        eng.set_chunk(0)
        eng.set_random_flatten(False)


@pytest.mark.parametrize("rnd", [False, True], ids=["deterministic", "randomised"])
def test_chunk_lane_and_small_batch_forms_give_the_same_bytes(S, case, rnd):
    """The 264 rows on a second ctx under set_lanes(1), set_chunk(8) and set_small_batch_max(0), each alone."""
    a, b, tables, _ = case.rows(264)
    eng = S.Engine(case.params)
    eng.upload_key(case.bkey)
    try:
        for raw in (False, True):
            ref = case.reference(264, rnd, raw)
            for knob, on, off in ((eng.set_lanes, 1, 2), (eng.set_chunk, 8, 0)):
                knob(on)
                _mode(eng, rnd)
                assert np.array_equal(eng.bootstrap_lut_batch(a, b, tables, raw=raw), ref), (knob.__name__, raw)
                knob(off)
        eng.set_small_batch_max(0)                 # (last: the ctx is closed below)
        for raw in (False, True):
            _mode(eng, rnd)
            assert np.array_equal(eng.bootstrap_lut_batch(a, b, tables, raw=raw), case.reference(264, rnd, raw))
            _mode(eng, rnd)
            assert np.array_equal(eng.bootstrap_lut_batch(a[:5], b[:5], tables[:5], raw=raw),
                                  case.reference(264, rnd, raw)[:5])
    finally:
        eng.close()


def test_one_call_number_per_call(case):
    """Randomised mode: a LUT call is call 0, the bootstrap_batch call after it the oracle's call 1, the LUT call after
    that call 2 of the stream."""
    eng, params, o, lo = case.eng, case.params, case.o, case.lo
    a, b, tables, _ = case.rows(5)
    z = np.zeros_like(a), np.zeros_like(b)
    bits = np.array([0, 1, 1, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    ga, gb = o.lwe_encrypt_bits(case.sk, bits, 320)
    _mode(eng, True)
    try:
        first = eng.bootstrap_lut_batch(a, b, tables)
        gate = eng.bootstrap_batch(ga[0::2], gb[0::2], ga[1::2], gb[1::2])
        third = eng.bootstrap_lut_batch(a, b, tables)
    finally:
        eng.set_random_flatten(False)
    assert np.array_equal(first, case.reference(5, True, False))
    assert np.array_equal(gate, o.bootstrap_batch(case.bkey, ga[0::2], gb[0::2], ga[1::2], gb[1::2], rnd=(SEED, 1)))
    _, acc = lo.bootstrap_batch(case.bkey, a, b, z[0], z[1], want_acc=True, rnd=(SEED, 2))
    assert np.array_equal(third, LR.rows_from_acc(params, acc, tables))
    assert not np.array_equal(third, first)


def test_argument_errors_write_nothing(S, case):
    params, n, r = case.params, case.params.n, case.params.r
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    a, b, tables, _ = case.rows(5)
    out = np.full((5, 3, n + 1, 2), SENTINEL, dtype=np.uint64)
    h = case.eng._h
    INVALID, NO_KEY = -1, -5                   # SGFHE_ERR_INVALID_ARG, SGFHE_ERR_NO_KEY
    assert L.sgfhe_bootstrap_lut_batch(None, None, None, None, 0, None, 0) == INVALID      # (a NULL ctx)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[4, n - 1] = r
    bad_b[2] = r
    calls = [(bad_a, b, tables, out, 0), (a, bad_b, tables, out, RAW_MODQ), (None, b, tables, out, 0),
             (a, None, tables, out, 0), (a, b, None, out, 0), (a, b, tables, None, 0),
             (a, b, tables, out, RAW_MODQ | RAW_RNS2), (a, b, tables, out, RAW_RNS2), (a, b, tables, out, 4),
             (a, b, tables, out, 0x80000000)]
    for xa, xb, xt, xo, flags in calls:
        rc = L.sgfhe_bootstrap_lut_batch(h, ptr(xa) if xa is not None else None, ptr(xb) if xb is not None else None,
                                         ptr(xt) if xt is not None else None, 5, ptr(xo) if xo is not None else None, flags)
        assert rc == INVALID and np.all(out == SENTINEL), flags
    assert L.sgfhe_bootstrap_lut_batch(h, ptr(bad_a), ptr(b), ptr(tables), 0, ptr(out), 0) == 0 and np.all(out == SENTINEL)
    fresh = S.Engine(params)
    try:
        rc = L.sgfhe_bootstrap_lut_batch(fresh._h, ptr(a), ptr(b), ptr(tables), 5, ptr(out), 0)
        assert rc == NO_KEY and np.all(out == SENTINEL)
    finally:
        fresh.close()
    # the ctx is as it was: the next call is the reference's
    _mode(case.eng, False)
    assert np.array_equal(case.eng.bootstrap_lut_batch(a, b, tables), case.reference(5, False, False))


def test_params_1024(S, oc, gpu_keys):
    """8 rows at Params(1024) in both modes against the oracle (A0 and the digit pairs of +-A0 differ per parameter
    set); the standard oracle's NTT-domain key serves the low-amplitude oracle unchanged."""
    from conftest import oracle_threads
    params, o, sk, eng = gpu_keys.engine(1024)
    khat = gpu_keys.khat(1024)
    lo = LR.low_oracle(oc, params)
    T = oracle_threads()
    lim = params.r // 32 - 1
    s = np.arange(8)
    e = np.array([lim, -lim, 0, 1, -1, lim // 2, -(lim // 3), lim])
    tables = np.array([0x96, 0xE8, 0xCA, 0x10, 0xFF, 0x00, 0x55, 0x7F], dtype=np.uint8)
    want = (tables.astype(np.int64) >> s) & 1
    a, b = LR.rows_at(params, sk, s, e, np.random.default_rng(330))
    z = np.zeros_like(a), np.zeros_like(b)
    try:
        for rnd in (False, True):
            _, acc = lo.bootstrap_batch(khat, a, b, z[0], z[1], want_acc=True, opt=True, threads=T,
                                        rnd=(SEED, 0) if rnd else None)
            for raw in (False, True):
                _mode(eng, rnd)
                got = eng.bootstrap_lut_batch(a, b, tables, raw=raw)
                assert np.array_equal(got, LR.rows_from_acc(params, acc, tables, raw=raw)), (rnd, raw)
                if not raw:
                    for k in range(3):
                        assert np.array_equal(LR.decrypt_scaled(params, sk, got[:, k], k), want), (rnd, k)
    finally:
        eng.set_random_flatten(False)


# ---- LUT nodes in circuits (sgfhe_circuit_create_lut) ------------------------------------------------------------

KEY32 = bytes(range(1, 33))


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


def _against_the_oracles(S, params, o, lo, sk, bkey, eng, c, inputs, bits, precondition=True):
    """circuit_run equals replay_levels driven by the two oracles in both modes and decrypts to evaluate_plain; first,
    from the oracle replay with the secret key: every LUT node's input-sum error is below Dr/8."""
    from sgfhe_jl_amd import circuit as C
    plain = c.evaluate_plain(bits)
    for key in (None, KEY32):
        boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, key)
        if precondition:
            worst = LR.lut_input_sum_errors(S, params, sk, c, inputs, bits, boot, boot_lut)
            live = {g for nodes in c.schedule() for g in nodes if c.kind(g) == "lut"}
            assert set(worst) == live and max(worst.values()) < params.r // 32, worst
        ref = C.replay_levels(c, inputs, params.r, boot, boot_lut)
        eng.set_random_flatten(key is not None, key or 0)
        try:
            got = eng.circuit_run(c, inputs)
        finally:
            eng.set_random_flatten(False)
        assert np.array_equal(got, ref), "circuit_run differs from the oracle replay (%s)" % ("randomised" if key else "deterministic")
        assert np.array_equal(_decrypt0(params, sk, got), plain)
    return got


def _truth_table_circuit(S):
    """Three inputs through refresh, then fan; 32 LUT nodes -- the NOT pattern rotating over the positions, one
    position FALSE in one node and TRUE in another --; a classic gate and a sum node in the level of the fans and in the
    level of the tables."""
    c = S.Circuit(3)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    g2 = c.gate(rx, ~ry)                       # level 2, beside the fans
    s2 = c.sum_node([(1, rx), (1, ry), (1, rz)])
    tables = [0x00, 0xFF, 0x96, 0xE8, 0xCA] + [int(t) for t in np.random.default_rng(340).integers(0, 256, size=27)]
    outs = []
    for i, t in enumerate(tables):
        x = [fx[2], fy[1], fz[0]]
        if i % 4 < 3:
            x[i % 4] = ~x[i % 4]
        if i == 5:
            x[0] = S.Circuit.FALSE
        if i == 6:
            x[1] = S.Circuit.TRUE
        if i == 7:
            x[2] = S.Circuit.TRUE
        outs.append(c.lut(t, *x)[0])
    g3 = c.gate(g2[2], s2[0])                  # level 3, beside the tables
    s3 = c.sum_node([(2, g2[0]), (2, s2[1])])
    c.output(*(outs + [g3[1], s3[0], ~outs[2]]))
    return c


def test_truth_table_circuit(S, oc):
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 341)
    try:
        c = _truth_table_circuit(S)
        assert [len(l) for l in c.schedule()] == [3, 5, 34] and c.info()["levels"] == 3
        bits = np.array([[(i >> k) & 1 for i in range(8)] for k in range(3)], dtype=bool)
        inputs = _inputs(params, sk, bits, 342)
        _against_the_oracles(S, params, o, lo, sk, bkey, eng, c, inputs, bits)
    finally:
        eng.close()


def test_call_boundary_inside_a_mixed_level(S, oc):
    """42 nodes x 200 instances = 8400 rows in one level, above SGFHE_CIRCUIT_CALL_ROWS = 8192: the boundary falls
    inside node 40, a LUT node; nodes 1 and 17 are LUT nodes too, the others classic.  Deterministic: every word
    against replay_levels on a second ctx's primitives (which the tests above hold against the oracle).  Randomised:
    a row's draws depend on its call and its index in the call alone, so the oracles run every LUT row, every row of
    the second call and every 16th row of the first, at their own indices, and those rows are compared."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 351, engines=2)
    n = params.n
    try:
        inst, luts = 200, {1: 0x96, 17: 0xCA, 40: 0x1B}
        c = S.Circuit(2)
        x, y = c.inputs
        outs = []
        for k in range(42):
            if k in luts:          # (inputs straight into a LUT node: bytes are compared, not bits)
                outs.append(c.lut(luts[k], S.Circuit.FALSE, S.Circuit.FALSE, ~x if k == 17 else y)[0])
            else:
                outs.append(c.gate(x, ~y if k % 2 else y)[k % 3])
        c.output(*outs)
        assert [len(l) for l in c.schedule()] == [42] and 40 * inst < C.CALL_ROWS < 41 * inst
        bits = np.random.default_rng(352).integers(0, 2, size=(2, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 353)
        want = C.replay_levels(c, inputs, params.r, lambda call, *lwe: ref.bootstrap_batch(*lwe),
                               lambda call, a, b, t, idx: ref.bootstrap_lut_batch(a, b, t))
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(got, want)
        assert np.array_equal(_decrypt0(params, sk, got)[[0, 2, 3]], c.evaluate_plain(bits)[[0, 2, 3]])   # (classic nodes)
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
        for k in luts:
            picked[k * inst:(k + 1) * inst] = True
        picked = picked.reshape(42, inst)
        assert picked[40].all() and picked[41].all() and picked.sum() > 1000
        eng.set_random_flatten(True, KEY32)
        got = eng.circuit_run(c, inputs)
        assert np.array_equal(got[picked], want[picked])
    finally:
        eng.set_random_flatten(False)
        eng.close()
        ref.close()


def test_lane_shifted_scaled_wires(S, oc):
    """group = 4: a LUT node reads lane-shifted scaled wires; a negated scale-1 reference that leaves the group fills
    with TRUE at scale 1, b = Dr/2 (the table then sees x1 = 1 there)."""
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 361)
    try:
        c = S.Circuit(2, group=4)
        fx, fy = (c.fan(c.refresh(w)) for w in c.inputs)
        a = c.lut(0xCA, fx[2].lane(1), ~fy[1].lane(-1), fx[0].lane(2))
        b = c.lut(0x96, ~fy[2].lane(-3), fx[1], ~fy[0].lane(3))
        c.output(a[0], b[0], ~a[0].lane(1))
        bits = np.random.default_rng(362).integers(0, 2, size=(2, 8)).astype(bool)
        inputs = _inputs(params, sk, bits, 363)
        got = _against_the_oracles(S, params, o, lo, sk, bkey, eng, c, inputs, bits)
        # lane 0 of each group: ~fy[1].lane(-1) left the group and reads TRUE, so node a is table 0xCA at x1 = 1
        x0 = np.roll(bits[0], -1)
        x2 = np.roll(bits[0], -2)
        for t in (0, 4):
            s = int(x0[t]) + 2 + 4 * (int(x2[t]) if t % 4 + 2 < 4 else 0)
            assert _decrypt0(params, sk, got)[0, t] == bool((0xCA >> s) & 1)
    finally:
        eng.close()


def test_ciphertext_form(S, oc):
    """One block; outputs: LUT wires +0 (one negated) and a classic gate wire.  flags 0 against replay_ct in both modes,
    PACK_DIRECT (deterministic) and PACK_DIRECT | PACK_LIFT (randomised) against replay_ct_direct: the LUT outputs are
    refreshed or lifted, the gate output is direct; all decrypt."""
    import pack_direct_ref as R
    import pack_lift_ref as PL
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 371)
    n = params.n
    try:
        # (the inputs are crafted with |e| <= Dr/16, inside the Dr/8 of a fan's single input)
        c = S.Circuit(2)
        x, y = c.inputs
        fx, fy = c.fan(x), c.fan(y)
        g = c.gate(x, ~y)                          # level 1 with the fans: an un-reduced mixed call when direct
        mux = c.lut(0xCA, fx[2], ~fy[1], fx[0])
        c.output(mux[0], ~fy[0], g[1])
        bits = np.random.default_rng(372).integers(0, 2, size=(2, 1, n)).astype(bool)
        plain = c.evaluate_plain(bits.reshape(2, -1))
        a, b = PL.craft_cts(S, params, sk, bits, 373)
        bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
        khat = o.key_transform(bkey)

        def dec(w, v):
            return np.stack([S.host.decrypt_rlwe(params, sk, w[q, 0], v[q, 0]) for q in range(w.shape[0])])

        for key in (None, KEY32):
            boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, key)
            pack = lambda call, pa, pb: tuple(np.stack(x) for x in zip(*[
                o.pack_encrypted_bits(bkey, pa[i], pb[i], khat=khat, rnd=(key, i, call) if key else None)
                for i in range(len(pa))]))
            (rw, rv), rlwe = C.replay_ct(c, a, b, params, boot, pack, boot_lut)
            eng.set_random_flatten(key is not None, key or 0)
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


def test_probe_records_each_wire_against_its_own_codeword(S, oc):
    """The records of scale-0, scale-1 and scale-2 wires equal the numpy statistics, each against its own codeword
    C = Dr >> k (wrong: |e| >= C/2, margin: |e| >= C/4); `out` has the bytes of circuit_run."""
    import noise_ref as NR
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 381)
    try:
        c = S.Circuit(3)
        rx, ry, rz = (c.refresh(w) for w in c.inputs)
        fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
        mux = c.lut(0xCA, fx[2], ~fy[1], fz[0])
        g = c.gate(rx, ry)
        c.output(mux[0], g[2])
        inst = 40
        bits = np.random.default_rng(382).integers(0, 2, size=(3, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 383)
        run = eng.circuit_run(c, inputs)
        out, stats = eng.circuit_probe(c, inputs, sk, bits)
        assert np.array_equal(out, run)
        # every wire's rows from a circuit whose plain evaluation and replay give them: the engine replay of one ctx
        wires, plain = {}, {}
        boot = lambda call, a1, b1, a2, b2: eng.bootstrap_batch(a1, b1, a2, b2)
        boot_lut = lambda call, a_, b_, t_, idx: eng.bootstrap_lut_batch(a_, b_, t_)
        for gnode in range(c.n_gates):
            for k in range(3):
                d = S.Circuit(3)
                d.gates, d.gate_shifts = list(c.gates), list(c.gate_shifts)
                d.gate_weights, d.gate_tables = dict(c.gate_weights), dict(c.gate_tables)
                d.outputs, d.output_shifts = [3 + 3 * gnode + k], [0]
                wires[(gnode, k)] = C.replay_levels(d, inputs, params.r, boot, boot_lut)[0]
                plain[(gnode, k)] = d.evaluate_plain(bits)[0]
        Dr = params.r // 4
        for gnode in range(c.n_gates):
            for k in range(3):
                st = stats[3 + 3 * gnode + k]
                scale = k if c.kind(gnode) == "lut" else 0
                if scale == 0:
                    want = NR.record_zr(params, sk, wires[(gnode, k)], plain[(gnode, k)])
                else:
                    e = [int(x) for x in LR.phase_errors(params, sk, wires[(gnode, k)], plain[(gnode, k)], scale)]
                    Cw = Dr >> scale
                    want = (len(e), sum(abs(x) >= Cw // 2 for x in e), max(abs(x) for x in e), sum(e),
                            sum(x * x for x in e), sum(abs(x) >= Cw // 4 for x in e))
                got = (st.rows, st.wrong, st.max_abs, st.sum, st.sum_sq, st.margin)
                assert got == want, (gnode, k, got, want)
                assert st.wrong == 0 and st.rows == inst
    finally:
        eng.close()


def test_params_1024_plan_on_a_clone(S, gpu_keys):
    """A plan with LUT nodes on a clone gives the bytes of the original ctx (Params(1024))."""
    params, o, sk, eng = gpu_keys.engine(1024)
    c = S.Circuit(3)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    mux = c.lut(0xCA, fx[2], fy[1], fz[0])
    c.output(mux[0], c.lut(0x96, mux[2], ~fy[1], fz[0])[0])
    bits = np.array([[(i >> k) & 1 for i in range(8)] for k in range(3)], dtype=bool)
    inputs = _inputs(params, sk, bits, 391)
    eng.set_random_flatten(False)
    want = eng.circuit_run(c, inputs)
    assert np.array_equal(_decrypt0(params, sk, want), c.evaluate_plain(bits))
    clone = eng.clone()
    try:
        assert np.array_equal(clone.circuit_run(c, inputs), want)
    finally:
        clone.close()
