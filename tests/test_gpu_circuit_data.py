"""Data planes on the device: LUT nodes and LUT siblings whose truth table is a byte of the run's data at every instance
(sgfhe_circuit_create_data, sgfhe_circuit_run_data / _run_ct_data / _run_probe_data, include/sgfhe_hip.h).  The contract is
that such a run is, byte for byte, the run of the constant-table plan with each row under its own table.  So: planes that
hold one table throughout against the sgfhe_circuit_create_lut_multi plan of those tables -- LWE form in both flatten
modes, ciphertext form under all three flag sets, the probe's records; random per-instance tables against
circuit.replay_levels on a second ctx's single-table primitives (deterministic) and on the two oracles (randomised), and row
by row against the constant-table runs of the byte values that occur; a level cut by a call boundary inside a data leader,
in every chunk, lane and small-batch form; a lane-shifted data family; the argument errors; circuit.lookup at Params(1024)
on a clone; the other ring kinds of tests/ring_cases.py.  Helpers and style: tests/test_gpu_lut_multi.py."""

import ctypes

import numpy as np
import pytest

import lut_ref as LR
import ring_cases as RC

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5
KEY32 = bytes(range(1, 33))
INVALID, NO_KEY = -1, -5                   # SGFHE_ERR_INVALID_ARG, SGFHE_ERR_NO_KEY
DIRECT, LIFT = 1, 2                        # SGFHE_CIRCUIT_PACK_DIRECT, SGFHE_CIRCUIT_PACK_LIFT


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
    """(boot, boot_lut) of replay_levels on a second ctx's primitives, deterministic mode: the single-table call takes
    one table per row."""
    return (lambda call, *lwe: ref.bootstrap_batch(*lwe),
            lambda call, a, b, t, idx: ref.bootstrap_lut_batch(a, b, t))


def _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits, data):
    """Deterministic: circuit_run equals replay_levels on the second ctx's single-table primitives.  Randomised: on the
    two oracles.  Both decrypt to evaluate_plain(bits, data)."""
    from sgfhe_jl_amd import circuit as C
    plain = c.evaluate_plain(bits, data)
    eng.set_random_flatten(False)
    ref.set_random_flatten(False)
    got = eng.circuit_run(c, inputs, data=data)
    assert np.array_equal(got, C.replay_levels(c, inputs, params.r, *_second_ctx(ref), data=data)), "deterministic"
    assert np.array_equal(_decrypt0(params, sk, got), plain)
    boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, KEY32)
    want = C.replay_levels(c, inputs, params.r, boot, boot_lut, data=data)
    eng.set_random_flatten(True, KEY32)
    try:
        rnd = eng.circuit_run(c, inputs, data=data)
    finally:
        eng.set_random_flatten(False)
    assert np.array_equal(rnd, want), "randomised"
    assert np.array_equal(_decrypt0(params, sk, rnd), plain)
    return got


PLANES = 13


def _family_circuit(S, const=None):
    """Three inputs through refresh, then fan; families of 2, 8 and 256 members that mix constant and data tables on the
    fanned wires (with a NOT on a different position each); a second LUT level reads data-sibling wires at all three
    scales -- one of its nodes a family again, one a single data node with the NOT on position 2; classic gates beside the
    fans and beside the families (a direct output of the ciphertext form in a level call that holds data rows).  Of the 256
    only four siblings are live, of the 8 four; plane 1 is named twice, plane 5 .. by many dead siblings.
    const = None: the data form, 13 planes.  const = [13 tables]: the same nodes with plane p replaced by the table
    const[p] -- the sgfhe_circuit_create_lut_multi plan."""
    P = (lambda p: S.Circuit.plane(p)) if const is None else (lambda p: int(const[p]))
    c = S.Circuit(3, planes=PLANES if const is None else 0)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    g2 = c.gate(rx, ~ry)
    A = c.lut_multi([P(0), 0xE8], fx[2], fy[1], fz[0])
    B = c.lut_multi([0x35, P(1), 0xD2, P(2), P(1), 0x6A, P(11), P(12)], ~fx[2], fy[1], fz[0])
    Cc = c.lut_multi([P(3 + i % 5) if i % 2 else (i + 77) % 256 for i in range(256)], fx[2], ~fy[1], fz[0])
    g3 = c.gate(g2[0], rz)
    D = c.lut(0xCA, A[1][2], B[3][1], Cc[201][0])
    E = c.lut_multi([P(8), 0x17, P(9)], Cc[17][2], ~Cc[255][1], B[7][0])
    F = c.lut_multi([P(10)], B[1][2], Cc[3][1], ~A[0][0])
    c.output(D[0], E[0][0], E[1][0], ~E[2][0], A[1][0], ~B[5][0], Cc[3][0], g2[0], F[0][0], g3[1])
    return c


def _constant_data(const, instances):
    return np.repeat(np.asarray(const, dtype=np.uint8)[:, None], instances, axis=1)


CONST = [int(t) for t in np.random.default_rng(1001).integers(0, 256, size=PLANES)]


def test_constant_planes_equal_the_constant_table_plan(S, oc):
    """data[p][:] = a table: every byte of circuit_run, of circuit_run_ct under flags 0, DIRECT and DIRECT | LIFT, and
    every record of the probe equals the run of the plan that has those tables."""
    import pack_lift_ref as PL
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1011)
    n = params.n
    try:
        c, k = _family_circuit(S), _family_circuit(S, CONST)
        assert c.planes == PLANES and k.planes == 0 and c.n_gates == k.n_gates == 7 + 2 + 8 + 256 + 1 + 1 + 3 + 1
        assert [len(l) for l in c.schedule()] == [len(l) for l in k.schedule()] == [3, 4, 4, 3]
        assert c.info() == k.info() and c.info()["nodes"] == 14
        assert c.kind(7) == "data" and c.kind(8) == "sibling" and c.kind(10) == "data_sibling" and c.kind(9) == "lut"
        assert len(c.live_siblings(9)) == 4 and len(c.live_siblings(17)) == 4 and c.live_siblings(7) == [8]
        inst = 16
        bits = np.random.default_rng(1012).integers(0, 2, size=(3, inst)).astype(bool)
        bits[:, :8] = [[(i >> j) & 1 for i in range(8)] for j in range(3)]
        inputs = _inputs(params, sk, bits, 1013)
        data = _constant_data(CONST, inst)
        runs = {}
        for key in (None, KEY32):
            eng.set_random_flatten(key is not None, key or 0)
            want = eng.circuit_run(k, inputs)
            eng.set_random_flatten(key is not None, key or 0)
            runs[key] = eng.circuit_run(c, inputs, data=data)
            assert np.array_equal(runs[key], want), key
            assert np.array_equal(_decrypt0(params, sk, runs[key]), k.evaluate_plain(bits))
        assert not np.array_equal(runs[None], runs[KEY32])
        # the probe: the same output bytes, and the records of corresponding wires (the wire ids are the same)
        eng.set_random_flatten(False)
        kout, kstats = eng.circuit_probe(k, inputs, sk, bits)
        cout, cstats = eng.circuit_probe(c, inputs, sk, bits, data=data)
        assert np.array_equal(cout, kout) and np.array_equal(cout, runs[None])
        assert len(cstats) == len(kstats) == 3 + 3 * c.n_gates and cstats == kstats
        assert sum(st.rows == inst for st in cstats) > 3 * 14 and all(st.wrong == 0 for st in cstats)
        # the ciphertext form, one block
        cbits = np.random.default_rng(1014).integers(0, 2, size=(3, 1, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, cbits, 1015)
        cdata = _constant_data(CONST, n)
        plain = k.evaluate_plain(cbits.reshape(3, -1))
        # (flags 0 and the lifted run randomised, the direct run deterministic)
        for key, direct, lift in ((KEY32, False, False), (None, True, False), (KEY32, True, True)):
            eng.set_random_flatten(key is not None, key or 0)
            (kw, kv), klwe = eng.circuit_run_ct(k, a, b, packed=True, lwe=True, direct=direct, lift=lift)
            eng.set_random_flatten(key is not None, key or 0)
            (w, v), lwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=direct, lift=lift, data=cdata)
            where = (key is not None, direct, lift)
            assert np.array_equal(lwe, klwe) and np.array_equal(w, kw) and np.array_equal(v, kv), where
            dec = np.stack([S.host.decrypt_rlwe(params, sk, w[q, 0], v[q, 0]) for q in range(w.shape[0])])
            assert np.array_equal(dec, plain), where
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_random_per_instance_tables(S, oc):
    """A different random byte in every plane at every instance: deterministic against the replay on a second ctx's
    single-table primitives, randomised against the two oracles, both decrypting to evaluate_plain(bits, data)."""
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1021, engines=2)
    try:
        c = _family_circuit(S)
        inst = 24
        rng = np.random.default_rng(1022)
        bits = rng.integers(0, 2, size=(3, inst)).astype(bool)
        data = rng.integers(0, 256, size=(PLANES, inst), dtype=np.uint8)
        inputs = _inputs(params, sk, bits, 1023)
        _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits, data)
        with pytest.raises(ValueError):
            eng.circuit_run(c, inputs)                               # planes and no data
        with pytest.raises(ValueError):
            eng.circuit_run(c, inputs, data=data[:, :-1])
        with pytest.raises(ValueError):
            eng.circuit_run(c, inputs, data=data.astype(np.uint32))
    finally:
        eng.close()
        ref.close()


def test_rows_of_a_byte_value_have_the_bytes_of_its_constant_run(S, oc):
    """Deterministic mode: where a plane holds the byte v, the wires of its node are those of the plan whose table is v
    -- for the leader's plane and for the sibling's (a sibling's wires are the leader's under the sibling's byte)."""
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1031)
    try:
        def build(tables):
            c = S.Circuit(3, planes=sum(isinstance(t, S.Plane) for t in tables))
            fx, fy, fz = (c.fan(c.refresh(w)) for w in c.inputs)
            fam = c.lut_multi(tables, fx[2], ~fy[1], fz[0])
            c.output(*[t[0] for t in fam])
            return c

        inst = 40
        rng = np.random.default_rng(1032)
        bits = rng.integers(0, 2, size=(3, inst)).astype(bool)
        inputs = _inputs(params, sk, bits, 1033)
        values = np.array([[0x96, 0x00, 0xE8, 0x1B], [0xFF, 0xCA, 0x96, 0x01]], dtype=np.uint8)
        data = np.stack([values[p][rng.integers(0, 4, size=inst)] for p in range(2)])
        got = eng.circuit_run(build([S.Circuit.plane(0), S.Circuit.plane(1)]), inputs, data=data)
        assert np.array_equal(_decrypt0(params, sk, got),
                              build([S.Circuit.plane(0), S.Circuit.plane(1)]).evaluate_plain(bits, data))
        seen = 0
        for p in range(2):
            for v in np.unique(data[p]):
                const = eng.circuit_run(build([int(v)]), inputs)
                rows = data[p] == v
                assert rows.any() and np.array_equal(got[p][rows], const[0][rows]), (p, v)
                seen += rows.sum()
        assert seen == 2 * inst
    finally:
        eng.close()


def test_call_boundary_inside_a_data_leader(S, oc):
    """42 row-taking nodes x 200 instances = 8400 rows in one level, above SGFHE_CIRCUIT_CALL_ROWS = 8192: the boundary
    falls inside rank 40, a data leader with two data siblings; rank 17 is a single data node, every fifth other node a sum
    node, the rest classic.  Deterministic: every word against replay_levels on a second ctx's primitives, and the same
    bytes under set_lanes(1), set_chunk(8) and set_small_batch_max(0).  Randomised: a row's draws depend on its call and
    its index in the call alone, so the oracles run every LUT row and every sibling's, every row of the second call and
    every 16th row of the first, at their own indices, and those rows are compared."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1041, engines=2)
    n = params.n
    try:
        inst = 200
        fams = {17: [0], 40: [1, 2, 3]}
        c = S.Circuit(2, planes=4)
        x, y = c.inputs
        outs, full = [], []          # full: outputs whose every row the randomised check compares
        for k in range(42):
            if k in fams:            # (inputs straight into a LUT node: bytes are compared, not bits)
                members = [S.Circuit.plane(p) for p in fams[k]]
                for t in c.lut_multi(members, S.Circuit.FALSE, S.Circuit.FALSE, ~x if k == 17 else y):
                    full.append(len(outs))
                    outs.append(t[0])
            elif k % 5 == 0:
                outs.append(c.sum_node([(1, x), (1, y if k % 2 else ~y)])[0])
            else:
                outs.append(c.gate(x, ~y if k % 2 else y)[k % 3])
        c.output(*outs)
        ranks = c.schedule()[0]
        assert len(c.schedule()) == 1 and len(ranks) == 42 and c.info()["nodes"] == 42 and c.n_gates == 44
        assert c.kind(ranks[40]) == "data" and [c.kind(h) for h in c.siblings(ranks[40])] == ["data_sibling"] * 2
        assert 40 * inst < C.CALL_ROWS < 41 * inst
        rng = np.random.default_rng(1042)
        bits = rng.integers(0, 2, size=(2, inst)).astype(bool)
        data = rng.integers(0, 256, size=(4, inst), dtype=np.uint8)
        inputs = _inputs(params, sk, bits, 1043)
        det = eng.circuit_run(c, inputs, data=data)
        assert np.array_equal(det, C.replay_levels(c, inputs, params.r, *_second_ctx(ref), data=data))
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

        want = C.replay_levels(c, inputs, params.r, boot, boot_lut, data=data)
        picked = picked.reshape(42, inst)
        rank_of_output = []
        for k in range(42):
            rank_of_output += [k] * (len(fams[k]) if k in fams else 1)
        sel = np.stack([picked[k] for k in rank_of_output])
        sel[full] = True
        assert sel[full].all() and sel.sum() > 1300 and not sel.all()
        eng.set_random_flatten(True, KEY32)
        got = eng.circuit_run(c, inputs, data=data)
        assert np.array_equal(got[sel], want[sel])
        # the chunk, lane and small-batch forms, deterministic
        eng.set_random_flatten(False)
        for knob, on, off in ((eng.set_lanes, 1, 2), (eng.set_chunk, 8, 0)):
            knob(on)
            assert np.array_equal(eng.circuit_run(c, inputs, data=data), det), knob.__name__
            knob(off)
        eng.set_small_batch_max(0)                 # (last: the ctx is closed below)
        assert np.array_equal(eng.circuit_run(c, inputs, data=data), det)
    finally:
        eng.set_random_flatten(False)
        eng.close()
        ref.close()


def test_lane_shifted_data_family(S, oc):
    """group = 4: a data family reads lane-shifted scaled wires (a negated scale-1 reference that leaves the group fills
    with TRUE at scale 1), a later data node reads lane-shifted data-sibling wires; the table is the byte of the node's
    OWN instance whatever the shifts -- evaluate_plain reads it there, and the replay hands it to the primitive there."""
    from sgfhe_jl_amd.circuit import lane_shift
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1051, engines=2)
    try:
        c = S.Circuit(2, group=4, planes=3)
        fx, fy = (c.fan(c.refresh(w)) for w in c.inputs)
        fam = c.lut_multi([S.Circuit.plane(0), 0x96, S.Circuit.plane(1)], fx[2].lane(1), ~fy[1].lane(-1), fx[0].lane(2))
        b = c.lut_data(2, ~fam[1][2].lane(-3), fam[2][1], ~fam[0][0].lane(3))
        c.output(fam[0][0], b[0], ~fam[2][0].lane(1))
        assert c.info()["nodes"] == 6
        rng = np.random.default_rng(1052)
        bits = rng.integers(0, 2, size=(2, 8)).astype(bool)
        data = rng.integers(0, 256, size=(3, 8), dtype=np.uint8)
        inputs = _inputs(params, sk, bits, 1053)
        got = _check_run(S, params, o, lo, sk, bkey, eng, ref, c, inputs, bits, data)
        # by hand: the family's inputs are shifted, its tables are not
        x0 = lane_shift(bits[0], 1, 4).astype(int)
        x1 = (~lane_shift(bits[1], -1, 4)).astype(int)
        x2 = lane_shift(bits[0], 2, 4).astype(int)
        s = x0 + 2 * x1 + 4 * x2
        dec = _decrypt0(params, sk, got)
        assert np.array_equal(dec[0], ((data[0] >> s) & 1).astype(bool))
        assert np.array_equal(dec[2], ~lane_shift(((data[1] >> s) & 1).astype(bool), 1, 4))
    finally:
        eng.close()
        ref.close()


def test_errors(S, oc):
    """The four entries without data refuse a plan with planes, write nothing and consume no call number; NULL data;
    no key; a plan without planes through the _data entries with NULL data is the old entry."""
    import pack_lift_ref as PL
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1061)
    n, m = params.n, params.m
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    try:
        c = S.Circuit(2, planes=2)
        fx, fy = c.fan(c.inputs[0]), c.fan(c.inputs[1])
        fam = c.lut_multi([S.Circuit.plane(1), S.Circuit.plane(0)], fx[2], fy[1], fx[0])
        c.output(fam[0][0], ~fam[1][0])
        k = S.Circuit(2)
        fx, fy = k.fan(k.inputs[0]), k.fan(k.inputs[1])
        fam = k.lut_multi([0xCA, 0x96], fx[2], fy[1], fx[0])
        k.output(fam[0][0], ~fam[1][0])
        inst = 8
        rng = np.random.default_rng(1062)
        bits = rng.integers(0, 2, size=(2, inst)).astype(bool)
        inputs = np.ascontiguousarray(_inputs(params, sk, bits, 1063))
        data = rng.integers(0, 256, size=(2, inst), dtype=np.uint8)
        cbits = rng.integers(0, 2, size=(2, 1, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, cbits, 1064)
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        cdata = rng.integers(0, 256, size=(2, n), dtype=np.uint8)
        skw = np.ascontiguousarray(sk, dtype=np.uint64)
        pbits = np.ascontiguousarray(bits.astype(np.uint8))
        h, plan = eng._h, c.handle()
        eng.set_random_flatten(True, KEY32)
        want = eng.circuit_run(c, inputs, data=data)                 # call numbers 0 and 1
        want_ct = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, data=cdata)
        out = np.full((2, inst, n + 1), SENTINEL, dtype=np.uint64)
        w = np.full((2, 1, m), SENTINEL, dtype=np.uint64)
        v, lwe = np.full_like(w, SENTINEL), np.full((2, n, n + 1), SENTINEL, dtype=np.uint64)
        stats = np.full((2 + 3 * c.n_gates, 8), SENTINEL, dtype=np.uint64)
        untouched = lambda: all((x == SENTINEL).all() for x in (out, w, v, lwe, stats))
        eng.set_random_flatten(True, KEY32)
        refused = [
            L.sgfhe_circuit_run(h, plan, inst, ptr(inputs), ptr(out)),
            L.sgfhe_circuit_run_ct(h, plan, 1, ptr(a), ptr(b), n, ptr(w), ptr(v), ptr(lwe)),
            L.sgfhe_circuit_run_ct_ex(h, plan, 1, ptr(a), ptr(b), n, ptr(w), ptr(v), ptr(lwe), 0),
            L.sgfhe_circuit_run_ct_ex(h, plan, 1, ptr(a), ptr(b), n, ptr(w), ptr(v), ptr(lwe), DIRECT | LIFT),
            L.sgfhe_circuit_run_probe(h, plan, inst, ptr(inputs), ptr(out), ptr(skw), ptr(pbits), ptr(stats)),
            # NULL data, and what the entries without data reject too
            L.sgfhe_circuit_run_data(h, plan, inst, ptr(inputs), None, ptr(out)),
            L.sgfhe_circuit_run_ct_data(h, plan, 1, ptr(a), ptr(b), n, None, ptr(w), ptr(v), ptr(lwe), 0),
            L.sgfhe_circuit_run_probe_data(h, plan, inst, ptr(inputs), None, ptr(out), ptr(skw), ptr(pbits), ptr(stats)),
            L.sgfhe_circuit_run_ct_data(h, plan, 1, ptr(a), ptr(b), n, ptr(cdata), ptr(w), ptr(v), ptr(lwe), 4),
            L.sgfhe_circuit_run_ct_data(h, plan, 1, ptr(a), ptr(b), n, ptr(cdata), ptr(w), ptr(v), ptr(lwe), LIFT),
            L.sgfhe_circuit_run_ct_data(h, plan, 1, ptr(a), ptr(b), n + 1, ptr(cdata), ptr(w), ptr(v), ptr(lwe), 0),
            L.sgfhe_circuit_run_ct_data(h, plan, 1, ptr(a), ptr(b), n, ptr(cdata), ptr(w), None, ptr(lwe), 0),
            L.sgfhe_circuit_run_data(h, plan, inst, None, ptr(data), ptr(out)),
            L.sgfhe_circuit_run_data(h, plan, inst, ptr(inputs), ptr(data), None),
            L.sgfhe_circuit_run_data(h, None, inst, ptr(inputs), ptr(data), ptr(out)),
            L.sgfhe_circuit_run_probe_data(h, plan, inst, ptr(inputs), ptr(data), ptr(out), None, ptr(pbits), ptr(stats)),
        ]
        assert refused == [INVALID] * len(refused) and untouched()
        assert L.sgfhe_circuit_run_data(None, plan, inst, ptr(inputs), ptr(data), ptr(out)) == INVALID
        # no instances: nothing to read, nothing written
        assert L.sgfhe_circuit_run_data(h, plan, 0, ptr(inputs), None, ptr(out)) == 0 and untouched()
        # no call number was consumed: the next runs are calls 0 and 1 again
        assert np.array_equal(eng.circuit_run(c, inputs, data=data), want)
        (gw, gv), glwe = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, data=cdata)
        assert np.array_equal(gw, want_ct[0][0]) and np.array_equal(gv, want_ct[0][1]) and np.array_equal(glwe, want_ct[1])
        fresh = S.Engine(params)
        try:
            rcs = [L.sgfhe_circuit_run_data(fresh._h, plan, inst, ptr(inputs), ptr(data), ptr(out)),
                   L.sgfhe_circuit_run_ct_data(fresh._h, plan, 1, ptr(a), ptr(b), n, ptr(cdata), ptr(w), ptr(v), ptr(lwe), 0),
                   L.sgfhe_circuit_run_probe_data(fresh._h, plan, inst, ptr(inputs), ptr(data), ptr(out), ptr(skw),
                                                  ptr(pbits), ptr(stats))]
            assert rcs == [NO_KEY] * 3 and untouched()
        finally:
            fresh.close()
        # a plan without planes through the _data entries, data NULL: the old entries
        kplan = k.handle()
        for key in (None, KEY32):
            eng.set_random_flatten(key is not None, key or 0)
            old = eng.circuit_run(k, inputs)
            (ow, ov), olwe = eng.circuit_run_ct(k, a, b, packed=True, lwe=True, direct=True)
            oout, ostats = eng.circuit_probe(k, inputs, sk, bits)
            eng.set_random_flatten(key is not None, key or 0)
            assert L.sgfhe_circuit_run_data(h, kplan, inst, ptr(inputs), None, ptr(out)) == 0
            assert np.array_equal(out, old)
            assert L.sgfhe_circuit_run_ct_data(h, kplan, 1, ptr(a), ptr(b), n, None, ptr(w), ptr(v), ptr(lwe), DIRECT) == 0
            assert np.array_equal(w, ow) and np.array_equal(v, ov) and np.array_equal(lwe, olwe)
            kstats = np.zeros((2 + 3 * k.n_gates, 8), dtype=np.uint64)
            assert L.sgfhe_circuit_run_probe_data(h, kplan, inst, ptr(inputs), None, ptr(out), ptr(skw), ptr(pbits),
                                                  ptr(kstats)) == 0
            assert np.array_equal(out, oout) and [S.engine.noise_record(rec) for rec in kstats] == ostats
        with pytest.raises(ValueError):
            eng.circuit_run(k, inputs, data=data)                    # data for a circuit without planes
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_params_1024_lookup_on_a_clone(S, gpu_keys):
    """circuit.lookup at Params(1024), 16 instances: every instance has its own random table of 16 entries of 4 bits and
    an encrypted 4-bit index; both modes decrypt to table_t[x_t], and a clone gives the original's bytes."""
    params, o, sk, eng = gpu_keys.engine(1024)
    k, count, inst = 4, 4, 16
    c = S.Circuit(k, planes=count << (k - 3))
    c.output(*S.lookup(c, c.inputs, count=count, refresh=True))
    assert c.info() == dict(levels=4, nodes=4 + 2 + 1 + 4, widest=4, slots=c.info()["slots"])
    rng = np.random.default_rng(1071)
    entries = rng.integers(0, 16, size=(inst, 16))                  # table_t[x]
    tables = [[sum(((int(entries[t][x]) >> f) & 1) << x for x in range(16)) for t in range(inst)] for f in range(count)]
    data = S.lookup_data(tables, k)
    assert data.shape == (8, inst)
    xs = (np.arange(inst) * 7 + 3) % 16
    bits = np.array([(xs >> j) & 1 for j in range(k)], dtype=bool)
    inputs = _inputs(params, sk, bits, 1072)
    value = lambda lwe: sum(_decrypt0(params, sk, lwe)[f].astype(int) << f for f in range(count))
    try:
        eng.set_random_flatten(False)
        want = eng.circuit_run(c, inputs, data=data)
        assert np.array_equal(value(want), entries[np.arange(inst), xs])
        clone = eng.clone()
        try:
            assert np.array_equal(clone.circuit_run(c, inputs, data=data), want)
        finally:
            clone.close()
        eng.set_random_flatten(True, KEY32)
        assert np.array_equal(value(eng.circuit_run(c, inputs, data=data)), entries[np.arange(inst), xs])
    finally:
        eng.set_random_flatten(False)


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_other_ring_kinds(S, oc, name, rnd):
    """A fan, a mixed family of three and a data node that reads its data siblings, on every other ring kind: with planes
    that hold one table throughout, circuit_run has the bytes of the constant-table plan; with random planes, where a
    plane holds a table's byte the leader's rows are the constant plan's."""
    rg = RC.ring(S, name)
    p = rg.params
    o, _ = RC.oracles(oc, rg)
    sk = o.private_key(1081)
    bkey = o.bootstrap_key(sk, 1082, noise=rg.noise)

    def build(const=None):
        P = (lambda q: S.Circuit.plane(q)) if const is None else (lambda q: const[q])
        c = S.Circuit(2, planes=3 if const is None else 0)
        f = c.fan(c.inputs[0])
        fam = c.lut_multi([P(0), 0x96, P(1)], f[2], ~f[1], c.inputs[1])
        top = c.lut_multi([P(2)], fam[2][2], fam[2][1], ~fam[1][0])
        c.output(fam[0][0], ~fam[2][0], top[0][0])
        return c

    eng = S.Engine(p)
    try:
        RC.upload(eng, rg, bkey)
        if not RC.set_mode(S, eng, rg, rnd):
            return
        inst = 12
        rng = np.random.default_rng(1083 + p.n)
        bits = rng.integers(0, 2, size=(2, inst)).astype(bool)
        inputs = _inputs(p, sk, bits, 1084)
        const = [0xCA, 0x1B, 0xE8]
        c, k = build(), build(const)
        assert [len(l) for l in c.schedule()] == [1, 1, 1] and c.info() == k.info()
        RC.set_mode(S, eng, rg, rnd)
        want = eng.circuit_run(k, inputs)
        RC.set_mode(S, eng, rg, rnd)
        assert np.array_equal(eng.circuit_run(c, inputs, data=_constant_data(const, inst)), want)
        data = _constant_data(const, inst)
        data[0, ::2] = 0x35                                          # the leader's plane: another table at every other instance
        RC.set_mode(S, eng, rg, rnd)
        got = eng.circuit_run(c, inputs, data=data)
        assert np.array_equal(got[0][1::2], want[0][1::2]) and np.array_equal(got[1:], want[1:])
        assert not np.array_equal(got[0][::2], want[0][::2])
    finally:
        eng.close()
