"""The direct pack stage (sgfhe_pack_lwe_modq, sgfhe_circuit_run_ct_ex with SGFHE_CIRCUIT_PACK_DIRECT; include/sgfhe_hip.h,
DESIGN.md section 11) without a device: the exports and their declarations, and the host composition
`circuit.replay_ct_direct` -- driven by the C oracle's un-reduced bootstraps and the big-int tail -- decrypting to the
plain evaluation in both flatten modes, with the LWE outputs of the reduced run."""

import os
import re

import numpy as np
import pytest

import pack_direct_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_declarations(S):
    L = S.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read(), flags=re.S)
    for name, arity in (("sgfhe_pack_lwe_modq", 5), ("sgfhe_circuit_run_ct_ex", 10)):
        assert name in S.EXPORTED_SYMBOLS and hasattr(L, name)
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "the header does not declare %s" % name
        assert len(m.group(1).split(",")) == arity
        assert len(getattr(L, name).argtypes) == arity
    assert re.search(r"#define\s+SGFHE_CIRCUIT_PACK_DIRECT\s+1u", hdr)
    assert L.sgfhe_abi_version() == 7          # functions are only added
    assert L.sgfhe_pack_lwe_modq(None, None, 1, None, None) == -1
    assert L.sgfhe_circuit_run_ct_ex(None, None, 1, None, None, 64, None, None, None, 1) == -1


def test_host_modred_and_not_against_the_oracle(S):
    """circuit.modred_words / lwe_not_modq (vectorised, two 64-bit words) against big-int arithmetic, at the
    rounding boundaries and at both ends of [0, Q)."""
    import bigint_oracle as BO
    from sgfhe_jl_amd import circuit as C
    for n in (64, 1024):
        p = S.Params(n)
        Q, r = p.Q, p.r
        rng = np.random.default_rng(n)
        vals = [0, 1, Q - 1, Q // 2, Q // 2 + 1, Q // 4, 2 * p.DQ_tilde, 2 * p.DQ_tilde + 1]
        for k in (1, 2, 3, r // 2, r - 1):                    # around (k + 1/2) Q / r, where the rounding turns
            c = ((2 * k + 1) * Q) // (2 * r)
            vals += [c - 1, c, c + 1]
        vals += [int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % Q for _ in range(2000)]
        x = np.array([[v & (2 ** 64 - 1), v >> 64] for v in vals], dtype=np.uint64)
        assert [int(q) for q in C.modred_words(x, Q, r)] == [BO.reduce_modulus(r, v, Q) for v in vals]
        rows = x[:len(vals) // 5 * 5].reshape(-1, 5, 2)       # LWEs of n + 1 = 5 residues: the last one is b
        got = C.lwe_not_modq(rows, Q, p.DQ_tilde)
        want = [[(-v) % Q for v in vals[5 * i:5 * i + 4]] + [(2 * p.DQ_tilde - vals[5 * i + 4]) % Q]
                for i in range(len(rows))]
        assert [[int(lo) | (int(hi) << 64) for lo, hi in row] for row in got] == want


@pytest.mark.parametrize("mode", ["deterministic", "randomised"])
def test_replay_ct_direct_decrypts_and_keeps_the_lwe_outputs(S, oc, mode):
    from sgfhe_jl_amd import circuit as C
    key = R.KEY32 if mode == "randomised" else None
    params = S.Params(64)
    n = params.n
    o = oc.Oracle.from_params(params)
    sk = o.private_key(31)
    bkey = o.bootstrap_key(sk, 32)
    bp, bk = R.bigint_params(params), R.key_lists(oc, bkey, n, params.m)
    c = R.direct_circuit(S)
    rng = np.random.default_rng(33)
    bits = rng.integers(0, 2, size=(3, 1, n)).astype(bool)
    a = np.zeros(bits.shape, dtype=np.uint64)
    b = np.zeros(bits.shape, dtype=np.uint64)
    for i in range(3):
        u = rng.integers(0, 2, size=n).astype(np.uint8)
        e = rng.integers(-(params.Dr // 8), params.Dr // 8 + 1, size=n).astype(np.int64)
        a[i, 0], b[i, 0] = S.host.encrypt_private(params, sk, u, e, bits[i, 0])
    log = []
    oboot, otail = R.oracle_boot(o, bkey, key), R.oracle_tail(bp, bk, key)

    def boot_raw(call, a1, b1, a2, b2):
        log.append(("boot", call, len(b1)))
        return oboot(call, a1, b1, a2, b2)

    def tail(call, group):
        log.append(("tail", call, len(group)))
        if len(log) == 4:    # the tail itself, once: composed from the oracle's own functions (ciphertext 1: z is not 0)
            ow, ov = R.tail_bigint(bp, bk, group[1], seed=key, ct=1, call=call)
            fw, fv = R.FastTail(bp, bk)(group[1], seed=key, ct=1, call=call)
            assert np.array_equal(ow, fw) and np.array_equal(ov, fv)
        return otail(call, group)

    (w, v), lwe = C.replay_ct_direct(c, a, b, params, boot_raw, tail)
    # two levels of n rows; one group: its three refreshed ciphertexts as one call, then one tail of all seven
    assert log == [("boot", 0, n), ("boot", 1, n), ("boot", 2, 3 * n), ("tail", 3, 7)]
    plain = c.evaluate_plain(bits.reshape(3, -1))
    dec = np.stack([S.host.decrypt_rlwe(params, sk, w[q, 0], v[q, 0]) for q in range(c.n_outputs)])
    assert np.array_equal(dec.astype(bool), plain)
    inputs = C.split_ciphertext_array(a, b, n, params.r).reshape(3, n, n + 1)
    want = C.replay_levels(c, inputs, params.r, R.oracle_boot(o, bkey, key, raw=False))
    assert np.array_equal(lwe, want), "the LWE outputs are those of the reduced run"
    assert np.array_equal(w[0], w[6]) == (key is None)      # one wire named twice: z differs, so do the draws
    worst = max(R.phase_error(params, sk, w[q, 0], v[q, 0], plain[q]) for q in range(c.n_outputs))
    print("worst packed phase error %d against Dr / 2 = %d (%s)" % (worst, params.Dr // 2, mode))
