"""The lifted pack stage (sgfhe_lwe_lift_modq, sgfhe_circuit_run_ct_ex with SGFHE_CIRCUIT_PACK_LIFT; include/sgfhe_hip.h,
DESIGN.md section 11) without a device: the exports and their declarations, `circuit.lift_words` against Python
integers, and the host composition `circuit.replay_ct_direct(lift=True)` -- driven by the C oracle's un-reduced
bootstraps and the big-int tail -- decrypting to the plain evaluation in both flatten modes with no bootstrap in its
pack stage."""

import os
import re

import numpy as np
import pytest

import pack_direct_ref as R
import pack_lift_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_declarations(S):
    L = S.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read(), flags=re.S)
    name, arity = "sgfhe_lwe_lift_modq", 4
    assert name in S.EXPORTED_SYMBOLS and hasattr(L, name)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "the header does not declare %s" % name
    assert len(m.group(1).split(",")) == arity
    assert len(getattr(L, name).argtypes) == arity
    assert re.search(r"#define\s+SGFHE_CIRCUIT_PACK_DIRECT\s+1u", hdr)
    assert re.search(r"#define\s+SGFHE_CIRCUIT_PACK_LIFT\s+2u", hdr)
    from sgfhe_jl_amd import engine as E
    assert E.CIRCUIT_PACK_LIFT == 2 and E.CIRCUIT_PACK_DIRECT == 1
    assert L.sgfhe_abi_version() == 7          # an entry point and a flag bit are only added
    assert L.sgfhe_lwe_lift_modq(None, None, 1, None) == -1
    for flags in (2, 3, 4):                    # (a NULL ctx is refused before the flags are looked at)
        assert L.sgfhe_circuit_run_ct_ex(None, None, 1, None, None, 64, None, None, None, flags) == -1
    jl = open(os.path.join(ROOT, "sgfhe.jl_amd", "julia", "SGFHEHip.jl")).read()
    assert "(:sgfhe_lwe_lift_modq, libsgfhe_hip)" in jl and re.search(r"const CIRCUIT_PACK_LIFT = UInt32\(2\)", jl)


def _ints(x):
    return [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(x).reshape(-1, 2)]


def test_lift_words_against_python_integers(S):
    """L(x) = floor((x Q + r/2) / r): every x of [0, r) at Params(64) and Params(1024), and the composite Q of the
    RNS ring (n = 1024, Q = B Bp) at x = 0, 1, r/2, r - 1.  L(x) < Q, L(Dr) is 2 DQ_tilde to within 1, and ModRed of
    L(x) is x."""
    import bench
    from sgfhe_jl_amd import circuit as C
    B, Bp = bench.rns2_moduli(S)
    cases = [(S.Params(64), None), (S.Params(1024), None)]
    pc = S.Params.custom(1024, B * Bp, B)
    cases.append((pc, [0, 1, pc.r // 2, pc.r - 1]))
    for p, xs in cases:
        Q, r = p.Q, p.r
        xs = list(range(r)) if xs is None else xs
        got = C.lift_words(np.array(xs, dtype=np.uint64), Q, r)
        assert got.shape == (len(xs), 2) and got.dtype == np.uint64
        vals = _ints(got)
        assert vals == [(x * Q + r // 2) // r for x in xs]
        assert all(v < Q for v in vals)
        assert [int(x) for x in C.modred_words(got, Q, r)] == xs
        (LDr,) = _ints(C.lift_words(np.array([p.Dr], dtype=np.uint64), Q, r))
        assert abs(LDr - 2 * p.DQ_tilde) <= 1
        # a wrap of r is a wrap of Q: L(x) + L(r - x) is Q to within the two roundings
        assert all(abs(vals[i] + (((r - x) * Q + r // 2) // r) - Q) <= 1 for i, x in enumerate(xs) if x)
    # any leading shape
    p = S.Params(64)
    x = np.arange(2 * 3 * 5, dtype=np.uint64).reshape(2, 3, 5)
    assert C.lift_words(x, p.Q, p.r).shape == (2, 3, 5, 2)


def test_crafted_and_widened_inputs(S):
    """What the tests of the stage feed it: craft_cts gives LWEs of the chosen error bound, and widen_cts the
    Ciphertext form (N = m) that splits to the same LWEs."""
    from sgfhe_jl_amd import circuit as C
    p = S.Params(64)
    n = p.n
    rng = np.random.default_rng(5)
    sk = rng.integers(0, 2, size=n).astype(np.uint64)
    bits = rng.integers(0, 2, size=(3, 2, n))
    a, b = LR.craft_cts(S, p, sk, bits, 6)
    lwe = C.split_ciphertext_array(a, b, n, p.r)
    err = LR.lwe_errors(p, sk, lwe, bits)
    assert np.abs(err).max() <= p.Dr // 16 and np.abs(err).max() > p.Dr // 32
    am, bm = LR.widen_cts(a, b, p.m, 7)
    assert am.shape == (3, 2, p.m) and np.array_equal(C.split_ciphertext_array(am, bm, n, p.r), lwe)


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_replay_ct_lift_decrypts_without_a_pack_stage_boot(S, oc, mode):
    """ripple_adder(3) with an input, a negated input, TRUE and a negated XOR3 wire as further outputs, one block at
    Params(64), inputs crafted with |e| <= Dr/16: the call log is the three level calls and one tail, `lwe` is that of
    replay_levels, everything decrypts.  The default path of replay_ct_direct on the same inputs still refreshes.
    Worst packed phase error of a sum bit with the CPU oracles, against Dr/2 = 128: 36 (deterministic) and 34
    (randomised) for these seeds, 39 over the seeds tried when the stage was designed; the carry 4 to 6."""
    from sgfhe_jl_amd import circuit as C
    key = R.KEY32 if mode == "randomised" else None
    params = S.Params(64)
    n = params.n
    o = oc.Oracle.from_params(params)
    sk = o.private_key(41)
    bkey = o.bootstrap_key(sk, 42)
    bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
    c, lifted = LR.lift_circuit(S)
    assert c.n_outputs == 8 and c.info()["levels"] == 3
    bits = np.random.default_rng(43).integers(0, 2, size=(6, 1, n)).astype(bool)
    a, b = LR.craft_cts(S, params, sk, bits, 44)
    inputs = C.split_ciphertext_array(a, b, n, params.r).reshape(6, n, n + 1)
    assert np.abs(LR.lwe_errors(params, sk, inputs, bits.reshape(6, n))).max() <= params.Dr // 16
    log = []
    oboot, otail = R.oracle_boot(o, bkey, key), R.oracle_tail(bp, bk, key)

    def boot_raw(call, a1, b1, a2, b2):
        log.append(("boot", call, len(b1)))
        return oboot(call, a1, b1, a2, b2)

    def tail(call, group):
        log.append(("tail", call, len(group)))
        return otail(call, group)

    (w, v), lwe = C.replay_ct_direct(c, a, b, params, boot_raw, tail, lift=True)
    assert log == [("boot", 0, n), ("boot", 1, n), ("boot", 2, n), ("tail", 3, 8)]
    want = C.replay_levels(c, inputs, params.r, R.oracle_boot(o, bkey, key, raw=False))
    assert np.array_equal(lwe, want), "the LWE outputs are those of the reduced run"
    plain = c.evaluate_plain(bits.reshape(6, -1))
    dec = np.stack([S.host.decrypt_rlwe(params, sk, w[q, 0], v[q, 0]) for q in range(c.n_outputs)])
    assert np.array_equal(dec.astype(bool), plain)
    err = [R.phase_error(params, sk, w[q, 0], v[q, 0], plain[q]) for q in range(c.n_outputs)]
    print("worst packed phase error against Dr / 2 = %d (%s): sum bits %d, carry %d, pass-through outputs %d, ~XOR3 %d"
          % (params.Dr // 2, mode, max(err[:3]), err[3], max(err[4:7]), err[7]))
    # the default path is unchanged: the same inputs with lift=False refresh the seven outputs that are not direct
    del log[:]
    calls = []
    C.replay_ct_direct(c, a, b, params, lambda call, a1, *rest: calls.append(("boot", call, len(a1))) or oboot(call, a1, *rest),
                       lambda call, group: calls.append(("tail", call, len(group))) or
                       (np.zeros((len(group), params.m), np.uint64),) * 2)
    assert calls == [("boot", 0, n), ("boot", 1, n), ("boot", 2, n), ("boot", 3, 7 * n), ("tail", 4, 8)]
