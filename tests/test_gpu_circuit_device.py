"""Device-resident circuit runs (sgfhe_circuit_run_device, _run_ct_device, _run_steps_device, _run_steps_ct_device,
include/sgfhe_hip.h): every array a torch tensor on the engine's device, the work queued on a stream and left in flight.
The contract is that every output word is the word the host entry writes for the same arguments on the same ctx state
and that the same call numbers are consumed, so the reference throughout is the HOST entry on a second ctx with the same
key and the same draw stream (as tests/test_gpu_circuit_steps.py compares the stepped run with a host loop): one-shot
over every node kind; two runs chained through a torch NOT on one stream without a host wait; a run that regrows the
ctx's buffers while the one before it is in flight; the stepped run fed in two chunks through one state tensor; the
ciphertext forms under every flag set; refusals that take no call number; one gate at Params(1024)."""

import ctypes

import numpy as np
import pytest

import lut_ref as LR

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5
KEY32 = bytes(range(1, 33))
INVALID, NO_KEY = -1, -5                   # SGFHE_ERR_INVALID_ARG, SGFHE_ERR_NO_KEY
MODES = pytest.mark.parametrize("key", [None, KEY32], ids=["deterministic", "randomised"])


@pytest.fixture(scope="module")
def duo(S, oc):
    """(params, secret key, eng, ref): two ctxs at Params(64) with one uploaded key; `ref` runs the host entries."""
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(2301)
    bkey = o.bootstrap_key(sk, 2302)
    eng, ref = S.Engine(params), S.Engine(params)
    eng.upload_key(bkey)
    ref.upload_key(bkey)
    yield params, sk, eng, ref
    eng.close()
    ref.close()


def _both(eng, ref, key):
    for e in (eng, ref):
        e.set_random_flatten(key is not None, key or 0)


def _inputs(params, sk, bits, seed):
    """bits [...] -> LWEs [...][n + 1] with |e| <= Dr/16, made from the secret key."""
    import noise_ref as NR
    rng = np.random.default_rng(seed)
    flat = np.asarray(bits).reshape(-1)
    e = rng.integers(-(params.r // 64), params.r // 64 + 1, size=flat.size)
    return np.ascontiguousarray(NR.handmade_zr(params, sk, rng, e, flat).reshape(np.asarray(bits).shape + (params.n + 1,)))


def _t(arr, dtype=None):
    """A numpy array of words (uint64) or planes (uint8) as a tensor on the device, the upload complete."""
    import torch
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint8:
        t = torch.from_numpy(a).cuda()
    else:
        t = torch.from_numpy(a.astype(np.uint64).view(np.int64)).cuda()
        if dtype is not None:
            t = t.view(dtype)
    torch.cuda.synchronize()
    return t


def _np(t):
    """The words of a tensor as uint64 (the caller has waited for the work that writes it)."""
    import torch
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


def _oneshot_circuit(S):
    """Every node kind, no register: classic (one input lane-shifted), three-input, sum, fan, a LUT family with a plane
    member, a data LUT; a routed and a lane-shifted output; group 4, two planes."""
    c = S.Circuit(5, group=4, planes=2)
    x0, x1, x2, x3, x4 = c.inputs
    a = c.gate(x0, x1.lane(1))
    m = c.gate3(x2, x3, a[2])
    s = c.sum_node([(1, x4), (2, a[1])])
    fx, fy, fz = c.fan(a[0]), c.fan(m[0]), c.fan(s[1])
    fam = c.lut_multi([0x96, S.Circuit.plane(0), 0xE8], fx[2], ~fy[1], fz[0])
    d = c.lut_data(1, fam[1][2], fam[2][1], fam[0][0])
    c.output(d[0], m[2], ~fam[1][0], c.reverse(a[2]), ~m[1].lane(-2), x3, S.Circuit.TRUE)
    return c


def _steps_circuit(S):
    """The circuit of every node kind of tests/test_gpu_circuit_steps.py: four registers, two stream inputs, two planes."""
    c = S.Circuit(6, planes=2, registers=4)
    reg, (x, y) = c.registers, c.stream_inputs
    a = c.gate(reg[0], x)
    m = c.gate3(reg[1], y, a[2])
    s = c.sum_node([(1, reg[2]), (2, a[1])])
    fx, fy, fz = c.fan(a[0]), c.fan(m[0]), c.fan(s[1])
    fam = c.lut_multi([0x96, S.Circuit.plane(0), 0xE8], fx[2], ~fy[1], fz[0])
    d = c.lut_data(1, fam[1][2], fam[2][1], fam[0][0])
    c.output(d[0], m[2], ~fam[1][0], a[2])
    c.next_state(a[1], s[1], ~m[0], reg[3])
    return c


@MODES
def test_one_shot_every_node_kind(S, duo, key):
    import torch
    params, sk, eng, ref = duo
    n = params.n
    c = _oneshot_circuit(S)
    assert c.route_tables and c.info()["nodes"] == 8
    inst = 12                                                            # three groups of 4
    rng = np.random.default_rng(2311)
    x = _inputs(params, sk, rng.integers(0, 2, size=(5, inst)).astype(bool), 2312)
    data = rng.integers(0, 256, size=(2, inst), dtype=np.uint8)
    try:
        _both(eng, ref, key)
        for dtype in (torch.int64, torch.uint64):                        # (each pair of runs: the next call numbers)
            xt, dt = _t(x, dtype), _t(data)
            big = _t(np.full((c.n_outputs + 1, inst, n + 1), SENTINEL, dtype=np.uint64), dtype)
            want = ref.circuit_run(c, x, data=data)
            got = eng.circuit_run_device(c, xt, data=dt, out=big[:c.n_outputs])
            eng.sync()
            assert got.dtype == dtype and got.data_ptr() == big.data_ptr()
            assert np.array_equal(_np(got), want), dtype
            assert (_np(big)[c.n_outputs] == SENTINEL).all()             # the row past the outputs
            assert np.array_equal(_np(xt), x) and np.array_equal(dt.cpu().numpy(), data)
            want = ref.circuit_run(c, x, data=data)
            fresh = eng.circuit_run_device(c, xt, data=dt)               # the result tensor is the method's own
            eng.sync()
            assert fresh.dtype == dtype and fresh.shape == (c.n_outputs, inst, n + 1)
            assert np.array_equal(_np(fresh), want), dtype
        with pytest.raises(ValueError):
            eng.circuit_run_device(c, xt)                                # planes and no data
        with pytest.raises(ValueError):
            eng.circuit_run_device(c, xt, data=dt, out=big)              # one row too long
    finally:
        _both(eng, ref, None)


@MODES
def test_chain_without_a_host_wait(S, duo, key):
    """ripple_adder(4), a torch NOT of its carry-out, a comparator of the sum word against the inputs: both runs and the
    torch kernels between them on one torch stream, nothing waited for until the end."""
    import torch
    from sgfhe_jl_amd.circuit import lwe_not
    params, sk, eng, ref = duo
    n, r, Dr = params.n, params.r, params.r // 4
    ca = S.ripple_adder(4)
    cb = S.Circuit(5)
    e = [c_ for c_ in cb.inputs]
    g0, g1 = cb.gate(e[0], e[1]), cb.gate(e[2], e[3])
    g2 = cb.gate(g0[2], g1[1])
    cb.output(cb.gate(g2[0], e[4])[1], g2[2], ~e[4])
    inst = 8
    rng = np.random.default_rng(2321)
    x = _inputs(params, sk, rng.integers(0, 2, size=(8, inst)).astype(bool), 2322)
    try:
        _both(eng, ref, key)
        ha = ref.circuit_run(ca, x)
        hx = np.ascontiguousarray(np.concatenate([ha[:4], lwe_not(ha[4], r)[None]]))
        want = ref.circuit_run(cb, hx)                                   # call numbers continue across A and B
        xt = _t(x)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            oa = eng.circuit_run_device(ca, xt, hip_stream=st)
            w = oa[4]
            neg = torch.cat([(r - w[:, :n]) % r, (Dr - w[:, n:]) % r], dim=1)
            xb = torch.cat([oa[:4], neg[None]]).contiguous()
            ob = eng.circuit_run_device(cb, xb, hip_stream=st)
        st.synchronize()
        assert np.array_equal(_np(oa), ha) and np.array_equal(_np(xb), hx)
        assert np.array_equal(_np(ob), want)
        # the draw stream stands where the reference's does: one more pair of runs
        oa2 = eng.circuit_run_device(ca, xt, hip_stream=st)
        eng.sync()
        assert np.array_equal(_np(oa2), ref.circuit_run(ca, x))
        if key is not None:
            assert not np.array_equal(_np(oa2), ha)
    finally:
        _both(eng, ref, None)


def test_growth_while_work_is_queued(S, duo):
    """A clone's buffers start empty: a run at 8 instances on the ctx's own stream sizes them, the run at 16 queued at
    once on another stream must regrow them -- after the first run has finished with them."""
    import torch
    params, sk, eng, ref = duo
    c = S.ripple_adder(3)
    rng = np.random.default_rng(2331)
    x8 = _inputs(params, sk, rng.integers(0, 2, size=(6, 8)).astype(bool), 2332)
    x16 = _inputs(params, sk, rng.integers(0, 2, size=(6, 16)).astype(bool), 2333)
    clone = eng.clone()
    try:
        _both(clone, ref, KEY32)
        want8, want16, want8b = ref.circuit_run(c, x8), ref.circuit_run(c, x16), ref.circuit_run(c, x8)
        t8, t16 = _t(x8), _t(x16)
        st = torch.cuda.Stream()
        got8 = clone.circuit_run_device(c, t8)
        got16 = clone.circuit_run_device(c, t16, hip_stream=st)
        got8b = clone.circuit_run_device(c, t8)                          # (no regrowth: queued behind the run on `st`)
        clone.sync()
        assert np.array_equal(_np(got8), want8)
        assert np.array_equal(_np(got16), want16)
        assert np.array_equal(_np(got8b), want8b)
    finally:
        clone.close()
        ref.set_random_flatten(False)


@MODES
def test_stepped_state_in_place(S, duo, key):
    import torch
    params, sk, eng, ref = duo
    c = _steps_circuit(S)
    inst, steps = 16, 5
    emit = [1, 0, 1, 1, 0]
    rng = np.random.default_rng(2341)
    state = _inputs(params, sk, rng.integers(0, 2, size=(4, inst)).astype(bool), 2342)
    stream = _inputs(params, sk, rng.integers(0, 2, size=(steps, 2, inst)).astype(bool), 2343)
    data = rng.integers(0, 256, size=(steps, 2, inst), dtype=np.uint8)
    try:
        _both(eng, ref, key)
        want, want_end = ref.circuit_run_steps(c, state, stream, data=data, emit=emit)
        assert want.shape[0] == 3
        st, xs, ds = _t(state), _t(stream), _t(data)
        first = st.clone()
        torch.cuda.synchronize()
        a, s1 = eng.circuit_run_steps_device(c, st, xs[:2], data=ds[:2], emit=emit[:2], state_out=st)
        b, s2 = eng.circuit_run_steps_device(c, st, xs[2:], data=ds[2:], emit=emit[2:], state_out=st)
        eng.sync()
        assert s1 is st and s2 is st and a.shape[0] == 1 and b.shape[0] == 2
        assert np.array_equal(np.concatenate([_np(a), _np(b)]), want)
        assert np.array_equal(_np(st), want_end) and not np.array_equal(_np(st), _np(first))
        assert np.array_equal(_np(xs), stream)
        # registers that start FALSE, results of the method's own
        want0, want0_end = ref.circuit_run_steps(c, None, stream[:2], data=data[:2])
        got0, end0 = eng.circuit_run_steps_device(c, None, xs[:2], data=ds[:2])
        eng.sync()
        assert np.array_equal(_np(got0), want0) and np.array_equal(_np(end0), want0_end)
    finally:
        _both(eng, ref, None)


@pytest.mark.parametrize("wide", [False, True], ids=["N=n", "N=m"])
def test_ciphertext_forms(S, duo, wide):
    """(w, v) and out_lwe under flags 0, DIRECT and DIRECT | LIFT against sgfhe_circuit_run_ct[_ex] on the reference ctx,
    in both modes; the input ciphertexts are split where they lie and stay as they were."""
    import pack_lift_ref as PL
    params, sk, eng, ref = duo
    n, m = params.n, params.m
    c, _lifted = PL.lift_circuit(S)
    blocks = 2
    rng = np.random.default_rng(2351)
    a, b = PL.craft_cts(S, params, sk, rng.integers(0, 2, size=(c.n_inputs, blocks, n)).astype(bool), 2352)
    if wide:
        a, b = PL.widen_cts(a, b, m, 2353)
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    at, bt = _t(a), _t(b)
    try:
        for key in (None, KEY32):
            _both(eng, ref, key)
            for direct, lift in ((False, False), (True, False), (True, True)):
                (hw, hv), hl = ref.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=direct, lift=lift)
                (w, v), lwe = eng.circuit_run_ct_device(c, at, bt, packed=True, lwe=True, direct=direct, lift=lift)
                eng.sync()
                where = (key is not None, direct, lift)
                assert w.shape == (c.n_outputs, blocks, m) and lwe.shape == (c.n_outputs, blocks * n, n + 1)
                assert np.array_equal(_np(w), hw) and np.array_equal(_np(v), hv), where
                assert np.array_equal(_np(lwe), hl), where
            hw, hv = ref.circuit_run_ct(c, a, b)                         # the packed outputs alone
            w, v = eng.circuit_run_ct_device(c, at, bt)
            hl = ref.circuit_run_ct(c, a, b, packed=False, lwe=True)     # the LWE outputs alone
            lwe = eng.circuit_run_ct_device(c, at, bt, packed=False, lwe=True)
            eng.sync()
            assert np.array_equal(_np(w), hw) and np.array_equal(_np(v), hv) and np.array_equal(_np(lwe), hl), key
        assert np.array_equal(_np(at), a) and np.array_equal(_np(bt), b)
    finally:
        _both(eng, ref, None)


def test_stepped_ciphertext_form(S, duo):
    """crc16_stream(8) with state ciphertexts over 3 steps, the last two emitted, DIRECT, randomised."""
    import pack_lift_ref as PL
    params, sk, eng, ref = duo
    n = params.n
    c = S.crc16_stream(8)
    blocks, steps = 1, 3
    rng = np.random.default_rng(2361)
    a, b = PL.craft_cts(S, params, sk, rng.integers(0, 2, size=(steps * 8, blocks, n)).astype(bool), 2362)
    sa, sb = PL.craft_cts(S, params, sk, rng.integers(0, 2, size=(16, blocks, n)).astype(bool), 2363, bound=1)
    a = np.ascontiguousarray(a.reshape(steps, 8, blocks, n), dtype=np.uint64)
    b = np.ascontiguousarray(b.reshape(steps, 8, blocks, n), dtype=np.uint64)
    sa, sb = np.ascontiguousarray(sa, dtype=np.uint64), np.ascontiguousarray(sb, dtype=np.uint64)
    try:
        _both(eng, ref, KEY32)
        ((hw, hv), hl), hend = ref.circuit_run_steps_ct(c, sa, sb, a, b, packed=True, lwe=True, direct=True, emit=[0, 1, 1])
        ((w, v), lwe), end = eng.circuit_run_steps_ct_device(c, _t(sa), _t(sb), _t(a), _t(b), packed=True, lwe=True,
                                                            direct=True, emit=[0, 1, 1])
        eng.sync()
        assert w.shape[0] == 2 and np.array_equal(_np(w), hw) and np.array_equal(_np(v), hv)
        assert np.array_equal(_np(lwe), hl) and np.array_equal(_np(end), hend)
        # registers that start FALSE: no state ciphertexts
        hl0, hend0 = ref.circuit_run_steps_ct(c, None, None, a, b, packed=False, lwe=True)
        lwe0, end0 = eng.circuit_run_steps_ct_device(c, None, None, _t(a), _t(b), packed=False, lwe=True)
        eng.sync()
        assert np.array_equal(_np(lwe0), hl0) and np.array_equal(_np(end0), hend0)
    finally:
        _both(eng, ref, None)


def test_errors_queue_nothing(S, duo):
    """Each refusal leaves the sentinels and the draw stream alone: the randomised run after it is still the reference
    ctx's next run."""
    params, sk, eng, ref = duo
    n = params.n
    L = S.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    plain = S.Circuit(2, group=4)
    plain.output(plain.gate(plain.inputs[0], plain.inputs[1].lane(1))[0])
    seq = S.Circuit(2, registers=1)
    g = seq.gate(seq.registers[0], seq.stream_inputs[0])
    seq.output(g[0])
    seq.next_state(g[1])
    inst = 8
    rng = np.random.default_rng(2371)
    x = _inputs(params, sk, rng.integers(0, 2, size=(2, inst)).astype(bool), 2372)
    xt = _t(x)
    out = _t(np.full((1, inst, n + 1), SENTINEL, dtype=np.uint64))
    run = L.sgfhe_circuit_run_device
    fresh = S.Engine(params)                                              # a ctx without a key
    try:
        _both(eng, ref, KEY32)
        refusals = [
            (lambda: run(eng._h, seq.handle(), inst, p(xt), None, p(out), None), INVALID),      # a plan with registers
            (lambda: run(eng._h, plain.handle(), inst, p(xt), None, None, None), INVALID),      # NULL out
            (lambda: run(eng._h, plain.handle(), inst - 2, p(xt), None, p(out), None), INVALID),    # group = 4
            (lambda: run(fresh._h, plain.handle(), inst, p(xt), None, p(out), None), NO_KEY),
        ]
        for i, (call, code) in enumerate(refusals):
            assert call() == code, i
            eng.sync()
            assert (_np(out) == SENTINEL).all(), i
            got = eng.circuit_run_device(plain, xt)
            eng.sync()
            assert np.array_equal(_np(got), ref.circuit_run(plain, x)), i
        with pytest.raises(S.SgfheError) as ei:
            eng.circuit_run_device(seq, xt)                              # the same refusal through the method
        assert ei.value.code == INVALID
        # no instances: nothing done, no call number taken
        assert run(eng._h, plain.handle(), 0, p(xt), None, p(out), None) == 0
        got = eng.circuit_run_device(plain, xt)
        eng.sync()
        assert (_np(out) == SENTINEL).all() and np.array_equal(_np(got), ref.circuit_run(plain, x))
    finally:
        fresh.close()
        _both(eng, ref, None)


def test_params_1024_one_gate_on_a_clone(S, gpu_keys):
    params, o, sk, eng = gpu_keys.engine(1024)
    c = S.Circuit(2)
    c.output(*c.gate(*c.inputs))
    inst = 8
    rng = np.random.default_rng(2381)
    x = _inputs(params, sk, rng.integers(0, 2, size=(2, inst)).astype(bool), 2382)
    try:
        eng.set_random_flatten(False)
        want = eng.circuit_run(c, x)
        assert np.array_equal(LR.decrypt_scaled(params, sk, want[0], 0).astype(bool),
                              LR.decrypt_scaled(params, sk, x[0], 0).astype(bool) & LR.decrypt_scaled(params, sk, x[1], 0).astype(bool))
        clone = eng.clone()
        try:
            got = clone.circuit_run_device(c, _t(x))
            clone.sync()
            res = _np(got)
        finally:
            clone.close()
        assert np.array_equal(res, want)
    finally:
        eng.set_random_flatten(False)
