"""Registers and stepped runs on the device (sgfhe_circuit_create_seq, sgfhe_circuit_run_steps, sgfhe_circuit_run_steps_ct,
include/sgfhe_hip.h).  The contract is that step s is, byte for byte, sgfhe_circuit_run_data of the step plan -- the same
nodes, no registers, outputs ++ next states -- on (the registers at the start of step s) ++ in[s], the level calls of
successive steps taking consecutive call numbers.  So: pure feedback with no bootstrap against numpy, word for word; a
circuit of every node kind against a host loop of Engine.circuit_run(step_plan) on a second ctx with the same key, in
both flatten modes; serial_adder against circuit.replay_steps on the two CPU oracles; scaled registers against
replay_steps on a second ctx's bootstrap_lut_batch; a level cut by a call boundary, in every chunk, lane and small-batch
form; resume through state_out and emit; no accumulation over 64 steps; the ciphertext form under all three flag sets;
the argument errors; one run at Params(1024) on a clone.  Helpers and style: tests/test_gpu_circuit_data.py."""

import ctypes

import numpy as np
import pytest

import lut_ref as LR

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
    """bits [...] -> LWEs [...][n + 1] with |e| <= Dr/16, made from the secret key."""
    import noise_ref as NR
    rng = np.random.default_rng(seed)
    flat = np.asarray(bits).reshape(-1)
    e = rng.integers(-(params.r // 64), params.r // 64 + 1, size=flat.size)
    return NR.handmade_zr(params, sk, rng, e, flat).reshape(np.asarray(bits).shape + (params.n + 1,))


def _decrypt0(params, sk, lwe):
    return LR.decrypt_scaled(params, sk, lwe, 0).reshape(lwe.shape[:-1]).astype(bool)


def _host_loop(ref, c, state, stream, data=None):
    """The stepped run as a host loop of the one-shot entry on the step plan, the state pulled down and pushed up again
    each step: (outputs [steps][n_outputs][instances][n + 1], the state after the last step)."""
    sp, outs = c.step_plan(), []
    for s in range(stream.shape[0]):
        res = ref.circuit_run(sp, np.concatenate([state, stream[s]]), data=None if data is None else data[s])
        outs.append(res[:c.n_outputs])
        state = res[c.n_outputs:]
    return np.stack(outs), state


def _both(eng, ref, key):
    for e in (eng, ref):
        e.set_random_flatten(key is not None, key or 0)


def test_pure_feedback_no_bootstrap(S, oc):
    """No live node: a step is the state load, the collect and the next-state gather.  Every word of out and state_out
    against numpy: a swap, a register holding itself, NOT, a lane-shifted stream input (FALSE at the group's edge), TRUE;
    an output that negates a lane-shifted register (TRUE at the edge: NOT after the fill)."""
    from sgfhe_jl_amd.circuit import lane_shift, lwe_not
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1911)
    n, r = params.n, params.r
    try:
        c = S.Circuit(6, group=4, registers=5)
        reg, (x,) = c.registers, c.stream_inputs
        c.output(*(reg + [~reg[3].lane(2)]))
        c.next_state(reg[1], reg[0], ~reg[2], x.lane(1), S.Circuit.TRUE)
        assert c.info()["nodes"] == 0 and c.info()["levels"] == 0
        inst, steps = 8, 4
        rng = np.random.default_rng(1912)
        state = rng.integers(0, r, size=(5, inst, n + 1), dtype=np.uint64)
        stream = rng.integers(0, r, size=(steps, 1, inst, n + 1), dtype=np.uint64)
        out, end = eng.circuit_run_steps(c, state, stream)
        true = lwe_not(np.zeros((inst, n + 1), dtype=np.uint64), r)
        cur = state
        for s in range(steps):
            want = np.concatenate([cur, lwe_not(lane_shift(cur[3], 2, 4), r)[None]])
            assert np.array_equal(out[s], want), s
            cur = np.stack([cur[1], cur[0], lwe_not(cur[2], r), lane_shift(stream[s, 0], 1, 4), true])
        assert np.array_equal(end, cur)
        assert not out[1, 3, 3].any() and out[1, 3, 2].any()        # lane 3 of x.lane(1) is the fill
        assert np.array_equal(out[1, 5, 2], true[0])                # NOT after the fill
        # registers that start FALSE
        out0, _ = eng.circuit_run_steps(c, None, stream)
        assert not out0[0, :5].any() and np.array_equal(out0[1, 4], true)
    finally:
        eng.close()


def _contract_circuit(S):
    """Classic, three-input, sum, LUT, family and data nodes; registers fed by a gate row, by a MID wire and by NOT of a
    gate row, and one that nothing reads but its own next state."""
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


@pytest.mark.parametrize("key", [None, KEY32], ids=["deterministic", "randomised"])
def test_contract_against_the_host_loop(S, oc, key):
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1921, engines=2)
    try:
        c = _contract_circuit(S)
        assert c.info() == c.step_plan().info() and c.info()["nodes"] == 8 and c.info()["levels"] == 5
        inst, steps = 16, 4
        rng = np.random.default_rng(1922)
        sbits = rng.integers(0, 2, size=(4, inst)).astype(bool)
        xbits = rng.integers(0, 2, size=(steps, 2, inst)).astype(bool)
        data = rng.integers(0, 256, size=(steps, 2, inst), dtype=np.uint8)
        state, stream = _inputs(params, sk, sbits, 1923), _inputs(params, sk, xbits, 1924)
        pout, pend = c.evaluate_plain_steps(sbits, xbits, data=data)
        _both(eng, ref, key)
        want, want_end = _host_loop(ref, c, state, stream, data)
        got, end = eng.circuit_run_steps(c, state, stream, data=data)
        assert np.array_equal(got, want) and np.array_equal(end, want_end)
        assert np.array_equal(_decrypt0(params, sk, got), pout) and np.array_equal(_decrypt0(params, sk, end), pend)
        assert np.array_equal(end[3], state[3])                      # the register that holds itself: the same words
    finally:
        _both(eng, ref, None)
        eng.close()
        ref.close()


def test_serial_adder_against_the_oracles(S, oc):
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1931)
    try:
        c = S.serial_adder()
        inst, steps = 16, 3
        rng = np.random.default_rng(1932)
        xbits = rng.integers(0, 2, size=(steps, 2, inst)).astype(bool)
        cbits = rng.integers(0, 2, size=(1, inst)).astype(bool)
        state, stream = _inputs(params, sk, cbits, 1933), _inputs(params, sk, xbits, 1934)
        pout, pend = c.evaluate_plain_steps(cbits, xbits)
        for key in (None, KEY32):
            boot, boot_lut = LR.oracle_boots(o, lo, bkey, params, key)
            want, want_end = C.replay_steps(c, state, stream, params.r, boot, boot_lut)
            eng.set_random_flatten(key is not None, key or 0)
            got, end = eng.circuit_run_steps(c, state, stream)
            assert np.array_equal(got, want) and np.array_equal(end, want_end), key
            assert np.array_equal(_decrypt0(params, sk, got), pout) and np.array_equal(_decrypt0(params, sk, end), pend)
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_scaled_registers(S, oc):
    """A LUT node's wires +0, +1, +2 feed registers of scales 0, 1, 2, which it reads back at positions 2, 1, 0; the
    scale-1 next state is negated, at the codeword Dr/2."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1941, engines=2)
    n, r = params.n, params.r
    try:
        c = S.Circuit(3, registers=3, reg_scales=[2, 1, 0])
        f = c.lut(0xCA, *c.registers)
        c.output(f[0])
        c.next_state(f[2], ~f[1], f[0])
        inst, steps = 16, 3
        rng = np.random.default_rng(1942)
        sbits = rng.integers(0, 2, size=(3, inst)).astype(bool)
        sbits[:, :8] = [[(i >> j) & 1 for i in range(8)] for j in range(3)]
        state = np.zeros((3, inst, n + 1), dtype=np.uint64)
        for i, k in enumerate((2, 1, 0)):                            # register i at the codeword Dr >> k, |e| <= Dr/64
            a, b = LR.rows_at(params, sk, sbits[i].astype(np.int64) * (4 >> k),
                              rng.integers(-(r // 256), r // 256 + 1, size=inst), rng)
            state[i, :, :n], state[i, :, n] = a, b
        stream = np.zeros((steps, 0, inst, n + 1), dtype=np.uint64)
        pout, pend = c.evaluate_plain_steps(sbits, np.zeros((steps, 0, inst), dtype=bool))
        want, want_end = C.replay_steps(c, state, stream, r, lambda call, *lwe: ref.bootstrap_batch(*lwe),
                                        lambda call, a, b, t, idx: ref.bootstrap_lut_batch(a, b, t))
        got, end = eng.circuit_run_steps(c, state, stream)
        assert np.array_equal(got, want) and np.array_equal(end, want_end)
        assert np.array_equal(_decrypt0(params, sk, got), pout)
        for i, k in enumerate((2, 1, 0)):
            assert np.array_equal(LR.decrypt_scaled(params, sk, end[i], k).astype(bool), pend[i]), i
    finally:
        eng.close()
        ref.close()


def test_call_boundary(S, oc):
    """Two nodes in one level over 4100 instances: 8200 rows, every level call cut at 8192."""
    from sgfhe_jl_amd import circuit as C
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1951, engines=2)
    try:
        c = S.Circuit(3, registers=2)
        reg, (x,) = c.registers, c.stream_inputs
        g0, g1 = c.gate(reg[0], x), c.gate(reg[1], ~x)
        c.output(g0[2], g1[0])
        c.next_state(g1[1], ~g0[0])
        inst, steps = 4100, 3
        assert len(c.schedule()) == 1 and inst < C.CALL_ROWS < 2 * inst
        rng = np.random.default_rng(1952)
        sbits = rng.integers(0, 2, size=(2, inst)).astype(bool)
        xbits = rng.integers(0, 2, size=(steps, 1, inst)).astype(bool)
        state, stream = _inputs(params, sk, sbits, 1953), _inputs(params, sk, xbits, 1954)
        pout, pend = c.evaluate_plain_steps(sbits, xbits)
        for key in (KEY32, None):
            _both(eng, ref, key)
            det, det_end = _host_loop(ref, c, state, stream)
            got, end = eng.circuit_run_steps(c, state, stream)
            assert np.array_equal(got, det) and np.array_equal(end, det_end), key
            assert np.array_equal(_decrypt0(params, sk, got), pout) and np.array_equal(_decrypt0(params, sk, end), pend)
        # the chunk, lane and small-batch forms, deterministic
        for knob, on, off in ((eng.set_lanes, 1, 2), (eng.set_chunk, 8, 0)):
            knob(on)
            got, end = eng.circuit_run_steps(c, state, stream)
            assert np.array_equal(got, det) and np.array_equal(end, det_end), knob.__name__
            knob(off)
        eng.set_small_batch_max(0)                 # (last: the ctx is closed below)
        got, end = eng.circuit_run_steps(c, state, stream)
        assert np.array_equal(got, det) and np.array_equal(end, det_end)
    finally:
        _both(eng, ref, None)
        eng.close()
        ref.close()


def test_resume_and_emit(S, oc):
    """5 steps = 2 steps, then 3 from the first run's state_out, on the same draw stream; emit = [0, 1, 0, 0, 1] gives
    the emitted steps' bytes of the full run and the same state; rows of `out` past the emitted count are not written."""
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1961)
    n = params.n
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    try:
        c = S.Circuit(4, registers=2)
        reg, (x, y) = c.registers, c.stream_inputs
        s, carry = c.full_adder(x, y, reg[0])
        g = c.gate(reg[1], s)
        c.output(s, g[2], reg[1])
        c.next_state(carry, g[1])
        inst, steps = 8, 5
        rng = np.random.default_rng(1962)
        sbits = rng.integers(0, 2, size=(2, inst)).astype(bool)
        xbits = rng.integers(0, 2, size=(steps, 2, inst)).astype(bool)
        state, stream = _inputs(params, sk, sbits, 1963), np.ascontiguousarray(_inputs(params, sk, xbits, 1964))
        pout, pend = c.evaluate_plain_steps(sbits, xbits)
        for key in (None, KEY32):
            eng.set_random_flatten(key is not None, key or 0)
            full, full_end = eng.circuit_run_steps(c, state, stream)
            assert np.array_equal(_decrypt0(params, sk, full), pout) and np.array_equal(_decrypt0(params, sk, full_end), pend)
            eng.set_random_flatten(key is not None, key or 0)
            a, a_end = eng.circuit_run_steps(c, state, stream[:2])
            b, b_end = eng.circuit_run_steps(c, a_end, stream[2:])
            assert np.array_equal(np.concatenate([a, b]), full) and np.array_equal(b_end, full_end), key
            eng.set_random_flatten(key is not None, key or 0)
            emit = [0, 1, 0, 0, 1]
            e, e_end = eng.circuit_run_steps(c, state, stream, emit=emit)
            assert e.shape[0] == 2 and np.array_equal(e, full[[1, 4]]) and np.array_equal(e_end, full_end), key
            # the C entry with a buffer of 5 steps: the rows past the two emitted steps keep the sentinel
            eng.set_random_flatten(key is not None, key or 0)
            out = np.full((steps, 3, inst, n + 1), SENTINEL, dtype=np.uint64)
            st = np.ascontiguousarray(state)
            em = np.array(emit, dtype=np.uint8)
            assert L.sgfhe_circuit_run_steps(eng._h, c.handle(), inst, steps, ptr(st), ptr(stream), None, ptr(em), ptr(out),
                                             None) == 0
            assert np.array_equal(out[:2], full[[1, 4]]) and (out[2:] == SENTINEL).all()
            # state_out alone
            eng.set_random_flatten(key is not None, key or 0)
            end = np.zeros_like(st)
            assert L.sgfhe_circuit_run_steps(eng._h, c.handle(), inst, steps, ptr(st), ptr(stream), None, None, None,
                                             ptr(end)) == 0
            assert np.array_equal(end, full_end)
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_no_accumulation_over_64_steps(S, oc):
    """serial_adder over 64 steps: the carry is a gate row, so nothing adds up.  The reference -- the host loop of the
    one-shot entry -- decrypts with 0 wrong, and the stepped run has its bytes."""
    params, o, lo, sk, bkey, (eng, ref) = _circuit_setup(S, oc, 1971, engines=2)
    try:
        c = S.serial_adder()
        inst, steps = 16, 64
        rng = np.random.default_rng(1972)
        x = [int(v) << 1 | t % 2 for t, v in enumerate(rng.integers(0, 1 << 63, size=inst))]     # 64-bit numbers
        y = [int(v) << 1 | 1 for v in rng.integers(0, 1 << 63, size=inst)]
        x[0], y[0] = (1 << 64) - 1, 1                                # a carry through all 64 steps
        xbits = np.array([[[(v >> i) & 1 for v in x], [(v >> i) & 1 for v in y]] for i in range(steps)], dtype=bool)
        stream = _inputs(params, sk, xbits, 1973)
        state = np.zeros((1, inst, params.n + 1), dtype=np.uint64)
        want, want_end = _host_loop(ref, c, state, stream)
        sums = [sum(int(b) << i for i, b in enumerate(_decrypt0(params, sk, want)[:, 0, t])) for t in range(inst)]
        carry = _decrypt0(params, sk, want_end)[0]
        assert [s + (int(carry[t]) << 64) for t, s in enumerate(sums)] == [x[t] + y[t] for t in range(inst)]   # 0 wrong
        got, end = eng.circuit_run_steps(c, None, stream)
        assert np.array_equal(got, want) and np.array_equal(end, want_end)
        pout, pend = c.evaluate_plain_steps(None, xbits)
        assert np.array_equal(_decrypt0(params, sk, got), pout) and np.array_equal(_decrypt0(params, sk, end), pend)
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("wide", [False, True], ids=["N=n", "N=m"])
def test_ciphertext_form(S, oc, wide):
    """crc16_stream(8) over 2 blocks and 3 steps: out_lwe and state_lwe are the LWE-form stepped run on the split inputs;
    deterministic with flags 0 an emitted step's (w, v) is pack_encrypted_bits of that step's out_lwe; under DIRECT and
    DIRECT | LIFT out_lwe is unchanged and every packed ciphertext decrypts to evaluate_plain_steps."""
    import pack_lift_ref as PL
    from sgfhe_jl_amd.circuit import pack_calls
    from sgfhe_jl_amd.scheme import split_ciphertext_array
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1981)
    n, m, r = params.n, params.m, params.r
    try:
        c = S.crc16_stream(8)
        blocks, steps = 2, 3
        rng = np.random.default_rng(1982)
        xbits = rng.integers(0, 2, size=(steps, 8, blocks, n)).astype(bool)
        sbits = rng.integers(0, 2, size=(16, blocks, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, xbits.reshape(steps * 8, blocks, n), 1983)
        sa, sb = PL.craft_cts(S, params, sk, sbits, 1984, bound=1)   # (a register enters the XORs as it is, doubled)
        stream = split_ciphertext_array(a, b, n, r).reshape(steps, 8, blocks * n, n + 1)
        state = split_ciphertext_array(sa, sb, n, r).reshape(16, blocks * n, n + 1)
        if wide:
            a, b = PL.widen_cts(a, b, m, 1985)
            sa, sb = PL.widen_cts(sa, sb, m, 1986)
        a, b = a.reshape((steps, 8, blocks, -1)), b.reshape((steps, 8, blocks, -1))
        pout, pend = c.evaluate_plain_steps(sbits.reshape(16, -1), xbits.reshape(steps, 8, -1))
        eng.set_random_flatten(False)
        want, want_end = eng.circuit_run_steps(c, state, stream)
        assert np.array_equal(_decrypt0(params, sk, want), pout)
        ((w, v), lwe), end = eng.circuit_run_steps_ct(c, sa, sb, a, b, packed=True, lwe=True)
        assert np.array_equal(lwe, want) and np.array_equal(end, want_end)
        cpc = pack_calls(n)
        for s in range(steps):
            g = want[s].reshape(16 * blocks, n, n + 1)
            for q0 in range(0, len(g), cpc):
                pw, pv = eng.pack_encrypted_bits(np.ascontiguousarray(g[q0:q0 + cpc, :, :n]),
                                                 np.ascontiguousarray(g[q0:q0 + cpc, :, n]))
                assert np.array_equal(w[s].reshape(-1, m)[q0:q0 + cpc], pw), (s, q0)
                assert np.array_equal(v[s].reshape(-1, m)[q0:q0 + cpc], pv), (s, q0)

        def decrypts(w, v, plain):
            dec = np.array([[S.host.decrypt_rlwe(params, sk, w[q, t], v[q, t]) for t in range(blocks)]
                            for q in range(w.shape[0])]).astype(bool)
            return np.array_equal(dec.reshape(w.shape[0], -1), plain)

        assert all(decrypts(w[s], v[s], pout[s]) for s in range(steps))
        # registers that start FALSE, the last step only, every flag set, both modes
        want0, want0_end = eng.circuit_run_steps(c, None, stream)
        p0, _ = c.evaluate_plain_steps(None, xbits.reshape(steps, 8, -1))
        for key, direct, lift in ((None, False, False), (KEY32, True, False), (None, True, True), (KEY32, False, False)):
            eng.set_random_flatten(key is not None, key or 0)
            ref_out, ref_end = eng.circuit_run_steps(c, None, stream, emit=[0, 0, 1])
            eng.set_random_flatten(key is not None, key or 0)
            ((w, v), lwe), end = eng.circuit_run_steps_ct(c, None, None, a, b, packed=True, lwe=True, direct=direct, lift=lift,
                                                          emit=[0, 0, 1])
            where = (key is not None, direct, lift)
            assert w.shape == (1, 16, blocks, m) and np.array_equal(lwe, ref_out) and np.array_equal(end, ref_end), where
            if key is None:
                assert np.array_equal(lwe[0], want0[2]) and np.array_equal(end, want0_end), where
            assert decrypts(w[0], v[0], p0[2]), where
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_ciphertext_form_lifted_output_and_scaled_refusal(S, oc):
    """An output that names a register is lifted under DIRECT | LIFT: its ciphertext is pack_lwe_modq(lwe_lift(rows)) of
    that step's out_lwe rows.  A plan with a scaled register is refused before anything is written."""
    import pack_lift_ref as PL
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1991)
    n, m = params.n, params.m
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    try:
        c = S.Circuit(2, registers=1)
        g = c.gate(c.registers[0], c.stream_inputs[0])
        c.output(g[0], c.registers[0])
        c.next_state(g[1])
        steps = 2
        rng = np.random.default_rng(1992)
        xbits = rng.integers(0, 2, size=(steps, 1, 1, n)).astype(bool)
        sbits = rng.integers(0, 2, size=(1, 1, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, xbits.reshape(steps, 1, n), 1993)
        a, b = a.reshape(steps, 1, 1, n), b.reshape(steps, 1, 1, n)
        sa, sb = PL.craft_cts(S, params, sk, sbits, 1994)
        pout, pend = c.evaluate_plain_steps(sbits.reshape(1, n), xbits.reshape(steps, 1, n))
        eng.set_random_flatten(False)
        ((w, v), lwe), end = eng.circuit_run_steps_ct(c, sa, sb, a, b, packed=True, lwe=True, lift=True)
        assert np.array_equal(_decrypt0(params, sk, lwe), pout) and np.array_equal(_decrypt0(params, sk, end), pend)
        for s in range(steps):
            lw, lv = eng.pack_lwe_modq(eng.lwe_lift(lwe[s, 1]))
            assert np.array_equal(w[s, 1, 0], lw[0]) and np.array_equal(v[s, 1, 0], lv[0]), s
            for q in range(2):
                assert np.array_equal(S.host.decrypt_rlwe(params, sk, w[s, q, 0], v[s, q, 0]).astype(bool), pout[s, q]), (s, q)
        # a scaled register has no ciphertext form
        e = S.Circuit(2, registers=1, reg_scales=[1])
        e.output(e.stream_inputs[0])
        e.next_state(~e.registers[0])
        a1, b1 = np.ascontiguousarray(a[:1]), np.ascontiguousarray(b[:1])
        ow = np.full((1, 1, 1, m), SENTINEL, dtype=np.uint64)
        ov, ol = np.full_like(ow, SENTINEL), np.full((1, 1, n, n + 1), SENTINEL, dtype=np.uint64)
        os_ = np.full((1, n, n + 1), SENTINEL, dtype=np.uint64)
        eng.set_random_flatten(True, KEY32)
        first = eng.circuit_run_steps_ct(c, sa, sb, a, b, packed=True, lwe=True)
        eng.set_random_flatten(True, KEY32)
        assert L.sgfhe_circuit_run_steps_ct(eng._h, e.handle(), 1, 1, None, None, ptr(a1), ptr(b1), n, None, None, ptr(ow),
                                            ptr(ov), ptr(ol), ptr(os_), 0) == INVALID
        assert all((x == SENTINEL).all() for x in (ow, ov, ol, os_))
        again = eng.circuit_run_steps_ct(c, sa, sb, a, b, packed=True, lwe=True)     # no call number was consumed
        assert all(np.array_equal(p, q) for p, q in zip((*first[0][0], first[0][1], first[1]), (*again[0][0], again[0][1], again[1])))
        # ... but the LWE form takes it
        out, end = eng.circuit_run_steps(e, None, np.zeros((1, 1, n, n + 1), dtype=np.uint64))
        assert end[0, 0, n] == params.r // 8 and not end[0, :, :n].any()
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_errors(S, oc):
    """What the stepped entries refuse, sentinels untouched; a plan with registers through every one-shot entry; steps = 0
    consumes no call number."""
    import pack_lift_ref as PL
    params, o, lo, sk, bkey, (eng,) = _circuit_setup(S, oc, 1996)
    n, m = params.n, params.m
    L = S.lib()
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    try:
        c = S.Circuit(3, group=4, planes=1, registers=1)
        f, fx = c.fan(c.registers[0]), c.fan(c.stream_inputs[0])
        t = c.lut_data(0, f[2], fx[1], c.stream_inputs[1])
        c.output(t[0])
        c.next_state(t[0])
        inst, steps = 8, 2
        rng = np.random.default_rng(1997)
        xbits = rng.integers(0, 2, size=(steps, 2, inst)).astype(bool)
        stream = np.ascontiguousarray(_inputs(params, sk, xbits, 1998))
        state = np.ascontiguousarray(_inputs(params, sk, np.zeros((1, inst), dtype=bool), 1999))
        data = rng.integers(0, 256, size=(steps, 1, inst), dtype=np.uint8)
        cbits = rng.integers(0, 2, size=(steps * 2, 1, n)).astype(bool)
        a, b = PL.craft_cts(S, params, sk, cbits, 2000)
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        cdata = rng.integers(0, 256, size=(steps, 1, n), dtype=np.uint8)
        skw = np.ascontiguousarray(sk, dtype=np.uint64)
        pbits = np.ascontiguousarray(np.zeros((3, inst), dtype=np.uint8))
        h, plan = eng._h, c.handle()
        eng.set_random_flatten(True, KEY32)
        want = eng.circuit_run_steps(c, state, stream, data=data)
        out = np.full((steps, 1, inst, n + 1), SENTINEL, dtype=np.uint64)
        end = np.full((1, inst, n + 1), SENTINEL, dtype=np.uint64)
        w = np.full((steps, 1, 1, m), SENTINEL, dtype=np.uint64)
        v, lwe = np.full_like(w, SENTINEL), np.full((steps, 1, n, n + 1), SENTINEL, dtype=np.uint64)
        slwe = np.full((1, n, n + 1), SENTINEL, dtype=np.uint64)
        stats = np.full((3 + 3 * c.n_gates, 8), SENTINEL, dtype=np.uint64)
        untouched = lambda: all((x == SENTINEL).all() for x in (out, end, w, v, lwe, slwe, stats))
        in3 = np.ascontiguousarray(np.concatenate([state, stream[0]]))
        run, run_ct = L.sgfhe_circuit_run_steps, L.sgfhe_circuit_run_steps_ct
        eng.set_random_flatten(True, KEY32)
        refused = [
            run(h, None, inst, steps, ptr(state), ptr(stream), ptr(data), None, ptr(out), ptr(end)),
            run(h, plan, inst, steps, ptr(state), None, ptr(data), None, ptr(out), ptr(end)),
            run(h, plan, inst, steps, ptr(state), ptr(stream), None, None, ptr(out), ptr(end)),
            run(h, plan, inst, steps, ptr(state), ptr(stream), ptr(data), None, None, None),
            run(h, plan, inst - 2, steps, ptr(state), ptr(stream), ptr(data), None, ptr(out), ptr(end)),   # group = 4
            run_ct(h, None, 1, steps, None, None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), 0),
            run_ct(h, plan, 1, steps, None, None, None, ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), 0),
            run_ct(h, plan, 1, steps, None, None, ptr(a), ptr(b), n, None, None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), 0),
            run_ct(h, plan, 1, steps, None, None, ptr(a), ptr(b), n, ptr(cdata), None, None, None, None, None, 0),
            run_ct(h, plan, 1, steps, None, None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), None, ptr(lwe), ptr(slwe), 0),
            run_ct(h, plan, 1, steps, ptr(a), None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), 0),
            run_ct(h, plan, 1, steps, None, None, ptr(a), ptr(b), n + 1, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), 0),
            run_ct(h, plan, 1, steps, None, None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), LIFT),
            run_ct(h, plan, 1, steps, None, None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe), 4),
            # a plan with registers through every one-shot entry
            L.sgfhe_circuit_run(h, plan, inst, ptr(in3), ptr(out)),
            L.sgfhe_circuit_run_data(h, plan, inst, ptr(in3), ptr(data), ptr(out)),
            L.sgfhe_circuit_run_ct(h, plan, 1, ptr(a), ptr(b), n, ptr(w), ptr(v), ptr(lwe)),
            L.sgfhe_circuit_run_ct_ex(h, plan, 1, ptr(a), ptr(b), n, ptr(w), ptr(v), ptr(lwe), DIRECT),
            L.sgfhe_circuit_run_ct_data(h, plan, 1, ptr(a), ptr(b), n, ptr(cdata), ptr(w), ptr(v), ptr(lwe), 0),
            L.sgfhe_circuit_run_probe(h, plan, inst, ptr(in3), ptr(out), ptr(skw), ptr(pbits), ptr(stats)),
            L.sgfhe_circuit_run_probe_data(h, plan, inst, ptr(in3), ptr(data), ptr(out), ptr(skw), ptr(pbits), ptr(stats)),
        ]
        assert refused == [INVALID] * len(refused) and untouched()
        assert run(None, plan, inst, steps, ptr(state), ptr(stream), ptr(data), None, ptr(out), ptr(end)) == INVALID
        # no steps, or no instances: OK, nothing written
        assert run(h, plan, inst, 0, ptr(state), ptr(stream), ptr(data), None, ptr(out), ptr(end)) == 0 and untouched()
        assert run(h, plan, 0, steps, ptr(state), ptr(stream), None, None, ptr(out), ptr(end)) == 0 and untouched()
        assert run_ct(h, plan, 1, 0, None, None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe), ptr(slwe),
                      0) == 0 and untouched()
        # no call number was consumed: the next randomised run is calls 0 .. again
        got = eng.circuit_run_steps(c, state, stream, data=data)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        fresh = S.Engine(params)
        try:
            rcs = [run(fresh._h, plan, inst, steps, ptr(state), ptr(stream), ptr(data), None, ptr(out), ptr(end)),
                   run_ct(fresh._h, plan, 1, steps, None, None, ptr(a), ptr(b), n, ptr(cdata), None, ptr(w), ptr(v), ptr(lwe),
                          ptr(slwe), 0)]
            assert rcs == [NO_KEY] * 2 and untouched()
        finally:
            fresh.close()
        with pytest.raises(ValueError):
            eng.circuit_run_steps(c, state, stream)                  # planes and no data
        with pytest.raises(ValueError):
            eng.circuit_run_steps(c, state, stream, data=data[:1])
        with pytest.raises(ValueError):
            eng.circuit_run_steps(c, state[:, :4], stream, data=data)
        with pytest.raises(ValueError):
            eng.circuit_run_steps(c, state, stream, data=data, emit=[1])
        with pytest.raises(S.SgfheError):
            eng.circuit_run(c, in3, data=data[0])                    # a plan with registers through the one-shot method
    finally:
        eng.set_random_flatten(False)
        eng.close()


def test_params_1024_serial_adder_on_a_clone(S, gpu_keys):
    """serial_adder at Params(1024), 8 instances, 16 steps -- 16 small calls -- on a clone: the 16-bit sums, and the bytes
    of the host loop on the original."""
    params, o, sk, eng = gpu_keys.engine(1024)
    c = S.serial_adder()
    inst, steps = 8, 16
    rng = np.random.default_rng(2011)
    x, y = rng.integers(0, 1 << 16, size=inst), rng.integers(0, 1 << 16, size=inst)
    x[0], y[0] = 0xFFFF, 1
    xbits = np.array([[(x >> i) & 1, (y >> i) & 1] for i in range(steps)], dtype=bool)
    stream = _inputs(params, sk, xbits, 2012)
    state = np.zeros((1, inst, params.n + 1), dtype=np.uint64)
    try:
        eng.set_random_flatten(False)
        want, want_end = _host_loop(eng, c, state, stream)
        clone = eng.clone()
        try:
            got, end = clone.circuit_run_steps(c, None, stream)
        finally:
            clone.close()
        assert np.array_equal(got, want) and np.array_equal(end, want_end)
        bits = _decrypt0(params, sk, got)[:, 0]
        total = sum(bits[i].astype(np.int64) << i for i in range(steps)) + (_decrypt0(params, sk, end)[0].astype(np.int64) << 16)
        assert np.array_equal(total, x + y)
    finally:
        eng.set_random_flatten(False)
