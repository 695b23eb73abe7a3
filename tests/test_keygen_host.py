"""Bootstrap-key generation without a device, on every case of tests/keygen_cases.py: the C oracle's key against the
big-integer oracle's, residue for residue, and against the definition of the key (src/fhe.jl:181-201), which neither
generator is consulted for: row (k, row) is (a, b) + s_k G[row] on the constant terms with b = a (*) s + e, so

    b - s_k G[row][1] - (a - s_k G[row][0]) (*) s

is a polynomial whose centred coefficients all lie in [-noise, noise] -- identically 0 at noise 0.  The product is the sum
of the shifts of a by the set bits of s, in Python integers.  tests/test_gpu_keygen.py then holds the device's key to the
C oracle's: two generators that agree and one property neither was written from."""

import numpy as np
import pytest

import bigint_oracle as BO
import keygen_cases as KC
import pack_direct_ref as R


def _times_bits(a, bits):
    """a (*) s mod x^m + 1 over the integers: a an object array of m integers, s the polynomial of `bits`."""
    m = len(a)
    out = np.zeros(m, dtype=object)
    for k, bit in enumerate(bits):
        if bit:
            out = out + (np.concatenate([-a[m - k:], a[:m - k]]) if k else a)
    return out


def _row_errors(p, key, sk):
    """Centred coefficients of the definition's polynomial, every row: [n * 4][m] Python integers."""
    Q = p.Q
    G = BO.gadget_matrix(p)
    out = []
    for k in range(p.n):
        for row in range(4):
            a = np.array(key[k][row][0], dtype=object)
            b = np.array(key[k][row][1], dtype=object)
            a[0] -= sk[k] * G[row][0]
            b[0] -= sk[k] * G[row][1]
            e = (b - _times_bits(a, sk)) % Q
            out.append([int(x) - Q if x > Q // 2 else int(x) for x in e])
    return out


@pytest.mark.parametrize("name", KC.NAMES)
def test_oracle_keys_agree_and_satisfy_the_definition(S, oc, name):
    rg = KC.ring(S, name)
    p = rg.params
    bp = R.bigint_params(p)
    o = oc.Oracle(p.n, p.r, p.m, p.Q, p.B, p.DQ_tilde, rns2=rg.rns2)
    cases = KC.cases(rg)
    assert cases[0][0] == rg.noise and {c[0] for c in cases} >= {0, 1, p.n, KC.noise_max(p.Q)}
    for case in cases:
        noise, kind, seed = case
        where = "%s: %s" % (name, KC.case_id(case))
        sk = KC.secret_key(o, rg, kind)
        bits = [int(x) & 1 for x in sk]
        assert len(bits) == p.n
        key = R.key_lists(oc, o.bootstrap_key(sk, seed, noise=noise), p.n, p.m)
        assert key == BO.bootstrap_key(bp, bits, seed, noise=noise), where
        assert all(0 <= x < p.Q for C in key for row in C for col in row for x in col), where
        errs = _row_errors(p, key, bits)
        worst = max(abs(x) for e in errs for x in e)
        assert worst <= noise, (where, worst)
        if noise >= 1 and p.m * 4 * p.n >= 2048:
            # (not a constant: 2048 draws or more from 2 noise + 1 values reach both ends of the range at noise 1, and
            # come within an eighth of it at the larger bounds, except with probability below 2^-100)
            assert worst >= noise - noise // 8 and min(x for e in errs for x in e) <= -(noise - noise // 8), where
        if kind == "zeros":                 # no gadget term, and b = e
            assert all(C[row][1] == [x % p.Q for x in errs[4 * k + row]] for k, C in enumerate(key) for row in range(4))


def test_noise_bound_is_refused_at_the_boundary_value(S, oc):
    """2 noise >= Q at noise = (Q + 1) / 2 on the smallest ring, and noise = 2^30 where Q allows more: both oracles raise,
    as sgfhe_bkey_generate refuses (tests/test_gpu_keygen.py)."""
    for name, bad in (("q16", None), ("wide", 1 << 30)):
        rg = KC.ring(S, name)
        p = rg.params
        bad = (p.Q + 1) // 2 if bad is None else bad
        assert bad == KC.noise_max(p.Q) + 1
        o = oc.Oracle.from_params(p)
        sk = KC.secret_key(o, rg, "oracle")
        with pytest.raises(ValueError):
            o.bootstrap_key(sk, KC.SEEDS[0], noise=bad)
        with pytest.raises(ValueError):
            BO.bootstrap_key(R.bigint_params(p), [int(x) for x in sk], KC.SEEDS[0], noise=bad)
