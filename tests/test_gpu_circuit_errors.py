"""What every run entry of the C ABI answers to arguments it cannot run (tests/run_error_cases.py) against the record
tests/golden/circuit_run_errors.json: code and message, nothing written, nothing queued; an empty probe run clears its
records; and after all of it the same ctx runs each of the four forms, host and device-resident, correctly."""

import json
import os

import numpy as np
import pytest

import lut_ref as LR
import pack_lift_ref as PL
import run_error_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctxs(S, oc):
    """(params, secret key, a ctx with a key, a ctx without one) at Params(64)."""
    params = S.Params(RC.N)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(2411)
    keyed, bare = S.Engine(params), S.Engine(params)
    keyed.generate_key(sk, 2412)
    yield params, sk, keyed, bare
    keyed.close()
    bare.close()


def test_refusals_match_the_record(S, ctxs):
    params, sk, keyed, bare = ctxs
    L = S.lib()
    with open(os.path.join(ROOT, "tests", "golden", "circuit_run_errors.json")) as fh:
        golden = json.load(fh)["cases"]
    assert set(golden) == {RC.case_id(e, c) for e, c in RC.CASES}
    plans = RC.make_plans(S)
    for name, c in plans.items():   # (the counts of the addressing cases rest on these)
        assert (c.info()["widest"], c.group) == (RC.PLAN_FACTS[name][4], RC.PLAN_FACTS[name][3]), name
    empty_probes = 0
    for entry, case in RC.CASES:
        call = RC.Call(entry, case, params)
        eng = keyed if case.key else bare
        code, msg = call.run(L, eng._h, plans[case.plan].handle())
        want = golden[RC.case_id(entry, case)]
        assert (code != 0) == (case.expect == "refused"), (entry, case.name, code, msg)   # (before any other look)
        assert [code, msg if code else ""] == want, (entry, case.name)
        eng.sync()
        zeroed = ("stats",) if code == 0 and RC.ENTRIES[entry].probe else ()
        empty_probes += len(zeroed)
        assert call.untouched(zeroed), (entry, case.name)
    assert empty_probes == 2   # sgfhe_circuit_run_probe and _probe_data: an empty run zero-fills `stats`


def _lwes(params, sk, bits, seed):
    """bits [...] -> LWEs [...][n + 1] with |e| <= Dr/16."""
    import noise_ref as NR
    rng = np.random.default_rng(seed)
    flat = np.asarray(bits).reshape(-1)
    e = rng.integers(-(params.r // 64), params.r // 64 + 1, size=flat.size)
    return np.ascontiguousarray(NR.handmade_zr(params, sk, rng, e, flat).reshape(np.asarray(bits).shape + (params.n + 1,)))


def _t(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def _np(t):
    import torch
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


def test_correct_runs_after_the_refusals(S, ctxs):
    """8 instances or 1 block on the ctx the refusals went through: an AND gate one-shot; over two steps the register
    plan, whose output is register AND input and whose register takes their XOR, from a FALSE register."""
    params, sk, eng, _bare = ctxs
    n = params.n
    plans = RC.make_plans(S)
    plain, regs = plans["plain"], plans["regs"]
    rng = np.random.default_rng(2421)
    # (an LWE that decrypts to neither bit comes back as 2 or 3 and equals no expected bit)
    dec = lambda rows: LR.decrypt_scaled(params, sk, rows, 0).reshape(np.shape(rows)[:-1])
    dec_ct = lambda w, v: np.stack([S.host.decrypt_rlwe(params, sk, w[o, 0], v[o, 0]) for o in range(w.shape[0])])
    # LWE forms
    bits = rng.integers(0, 2, size=(2, 8)).astype(bool)
    x = _lwes(params, sk, bits, 2422)
    sbits = rng.integers(0, 2, size=(2, 1, 8)).astype(bool)          # [steps][stream inputs][instances]
    xs = _lwes(params, sk, sbits, 2423)
    want_steps = np.stack([np.zeros(8, dtype=bool), sbits[0, 0] & sbits[1, 0]])
    want_state = sbits[0, 0] ^ sbits[1, 0]
    assert np.array_equal(dec(eng.circuit_run(plain, x)[0]), bits[0] & bits[1])
    xt, xst = _t(x), _t(xs)                                            # (held until the queued work is done)
    got = eng.circuit_run_device(plain, xt)
    eng.sync()
    assert np.array_equal(dec(_np(got)[0]), bits[0] & bits[1])
    out, st = eng.circuit_run_steps(regs, None, xs)
    assert np.array_equal(dec(out[:, 0]), want_steps) and np.array_equal(dec(st[0]), want_state)
    out, st = eng.circuit_run_steps_device(regs, None, xst)
    eng.sync()
    assert np.array_equal(dec(_np(out)[:, 0]), want_steps) and np.array_equal(dec(_np(st)[0]), want_state)
    # ciphertext forms: one block is n instances
    cbits = rng.integers(0, 2, size=(2, 1, n)).astype(bool)
    a, b = (np.ascontiguousarray(t, dtype=np.uint64) for t in PL.craft_cts(S, params, sk, cbits, 2424))
    tbits = rng.integers(0, 2, size=(2, 1, n)).astype(bool)          # [steps (x 1 stream input)][blocks][n]
    ta, tb = (np.ascontiguousarray(t, dtype=np.uint64).reshape(2, 1, 1, n) for t in PL.craft_cts(S, params, sk, tbits, 2425))
    want_steps = np.stack([np.zeros(n, dtype=bool), tbits[0, 0] & tbits[1, 0]])
    want_state = tbits[0, 0] ^ tbits[1, 0]
    (w, v), lwe = eng.circuit_run_ct(plain, a, b, packed=True, lwe=True)
    assert np.array_equal(dec_ct(w, v)[0], cbits[0, 0] & cbits[1, 0]) and np.array_equal(dec(lwe[0]), cbits[0, 0] & cbits[1, 0])
    at, bt, tat, tbt = _t(a), _t(b), _t(ta), _t(tb)
    (w, v), lwe = eng.circuit_run_ct_device(plain, at, bt, packed=True, lwe=True)
    eng.sync()
    assert np.array_equal(dec_ct(_np(w), _np(v))[0], cbits[0, 0] & cbits[1, 0])
    assert np.array_equal(dec(_np(lwe)[0]), cbits[0, 0] & cbits[1, 0])
    ((w, v), lwe), st = eng.circuit_run_steps_ct(regs, None, None, ta, tb, packed=True, lwe=True)
    assert all(np.array_equal(dec_ct(w[s], v[s])[0], want_steps[s]) for s in range(2))
    assert np.array_equal(dec(lwe[:, 0]), want_steps) and np.array_equal(dec(st[0]), want_state)
    ((w, v), lwe), st = eng.circuit_run_steps_ct_device(regs, None, None, tat, tbt, packed=True, lwe=True)
    eng.sync()
    assert all(np.array_equal(dec_ct(_np(w)[s], _np(v)[s])[0], want_steps[s]) for s in range(2))
    assert np.array_equal(dec(_np(lwe)[:, 0]), want_steps) and np.array_equal(dec(_np(st)[0]), want_state)
