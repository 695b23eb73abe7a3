"""The pack tail (sgfhe_pack_lwe_modq: k_pack_flatten -> k_shortprod -> k_pack_finish) on chosen operands.  Elsewhere the
tail runs on bootstrap outputs and oracle keys, uniform residues whose exact group sums sit near the square root of what
the stage is sized for.  Here both operands of every half-width product are chosen: key rows 2 and 3 of every slice (the
only rows the tail reads) hold +-(Q - 1)/2 -- or, in one pattern, values within 1/32 of that which let every bit of every
digit reach the result (chosen_key) --, and every LWE a-word is a residue whose flatten digits are both at the top or
both at the bottom of their range (pack_direct_ref.extreme_residue, which tests/test_gpu_worstcase.py drives the k-loop's
CRT with).  (w, v) of every ciphertext, word for word, against pack_direct_ref.FastTail, and on one ring against
tail_bigint as well; on every ring of tests/ring_cases.py and the n = 32 ring of tests/keygen_cases.py, in every flatten
mode the ring packs in.

Randomised mode: the test knows the flatten key, so it computes the draws (x0, x1) of call 0, ciphertext ct, slice i,
coefficient j and sets a[j][i] = x0 + x1 B + t mod Q with t the top residue where x0 + x1 >= 0 and the bottom one
elsewhere: flatten(a - x) + x is then the extreme digit plus a draw of its own sign, the largest digits the mode has.
Coefficients j >= n of every as_i are the zero padding of the resize (fhe.jl:675-677): the randomised flatten draws for
them too, and their digits cannot be chosen.

The figures each case prints -- max |exact group sum| over 0.4 prod(primes), the bound the stage's CRT is exact to -- are
measurements, recorded in RESULTS.md and DESIGN.md section 11; no ratio is asserted."""

import math
import random

import numpy as np
import pytest

import bigint_oracle as BO
import keygen_cases as KC
import pack_direct_ref as R
import ring_cases as RC
import rns_model as RM
from conftest import oracle_threads

pytestmark = pytest.mark.gpu

NAMES = RC.NAMES + ("synth32",)
KEY_PATTERNS = ("all +", "all -", "column 0 +, column 1 -", "alternating", "jittered")
BIGINT_RING = "limb64"          # also against tail_bigint: two groups deterministic, a basis per mode


# The sizing rule (plan_bases / derive_basis of csrc/constants.h), restated once in rns_model: (primes, pack group) of the
# ctx's basis for a flatten mode -- the fewest of the largest primes below 2^29 with p = 1 mod 2^15 whose product covers
# 5 m B Q (20 m B Q randomised), two at least; G the largest power of two, n at most, with G m B Q / 2 (four times that
# randomised) below 0.4 of the product.
basis = RM.basis


# ---- operands ------------------------------------------------------------------------------------------------------------

def chosen_key(p, pattern):
    """key[k][row][col] = m residues +-(Q - 1)/2 centred (all four rows alike; the tail reads rows 2 and 3).

    "jittered" is there for what the other four cannot see.  d (Q - 1)/2 = -d/2 or (Q - d)/2 mod Q, so under a key of
    +-(Q - 1)/2 a column sum is -D/2 or (Q - D)/2 mod Q with D the signed sum of the digits: the exact integer is as
    large as it gets, which is what the CRT has to survive, but after the reduction mod Q and ModRed only the parity of D
    is left wherever (r n m)^2 < Q -- a digit that is wrong by an even amount, such as a lost padding term, changes no
    word.  The jittered key holds +-((Q - 1)/2 - u), u uniform below Q/64 and different for every coefficient, row,
    column and slice: within 1/32 of the extreme size, and every bit of every digit reaches the result."""
    m, Q = p.m, p.Q
    pos, neg = (Q - 1) // 2, (Q + 1) // 2
    assert Q % 2 == 1 and pos + neg == Q
    if pattern == "jittered":
        rng = random.Random(621)
        res = lambda i: (pos - rng.randrange(Q // 64)) if i & 1 else (neg + rng.randrange(Q // 64))
        return [[[[res(i + col + row) for i in range(m)] for col in range(2)] for row in range(4)] for _ in range(p.n)]
    if pattern == "all +":
        cols = [[pos] * m, [pos] * m]
    elif pattern == "all -":
        cols = [[neg] * m, [neg] * m]
    elif pattern == "column 0 +, column 1 -":
        cols = [[pos] * m, [neg] * m]
    else:
        assert pattern == "alternating"
        cols = [[neg if i & 1 else pos for i in range(m)], [pos if i & 1 else neg for i in range(m)]]
    return [[[list(c) for c in cols] for _ in range(4)] for _ in range(p.n)]


def key_words(oc, p, key):
    flat = [x for C in key for row in C for col in row for x in col]
    return oc.ints_to_u128(flat).reshape(p.n, 4, 2, p.m, 2)


def flatten_offset(p):
    s = (p.B - 1) // 2 if p.B % 2 else p.B // 2 - 1
    return (1 + p.B) * s % p.Q


def _lwe_words(p, a, b):
    """a [n bits][n] integers, b [n] -> [n][n + 1][2] uint64."""
    out = np.zeros((p.n, p.n + 1, 2), dtype=np.uint64)
    for j in range(p.n):
        for i, x in enumerate(list(a[j]) + [b[j]]):
            assert 0 <= x < p.Q
            out[j, i] = (x & 0xFFFFFFFFFFFFFFFF, x >> 64)
    return out


def deterministic_lwes(p):
    """[(label, [n][n + 1][2])]: bit j's a-words all top, all bottom, alternating by j (so that the products alternate)
    both ways; then every a-word 0, Q - 1, and the residues either side of where the flatten wraps: off - 1 and off, and
    -off - 1 (x' = Q - 1; -off itself is the bottom residue).  b alternates 0 and Q - 1."""
    n, Q = p.n, p.Q
    top, bot, off = R.extreme_residue(p, +1), R.extreme_residue(p, -1), flatten_offset(p)
    assert bot == (Q - off) % Q
    b = [0 if j % 2 == 0 else Q - 1 for j in range(n)]
    rows = [("all top", [[top] * n] * n), ("all bottom", [[bot] * n] * n),
            ("top, bottom by bit", [[top if j % 2 == 0 else bot] * n for j in range(n)]),
            ("bottom, top by bit", [[bot if j % 2 == 0 else top] * n for j in range(n)])]
    for label, x in (("0", 0), ("Q - 1", Q - 1), ("off - 1", (off - 1) % Q), ("off", off), ("-off - 1", (Q - off - 1) % Q)):
        rows.append(("every word " + label, [[x] * n] * n))
    return [(label, _lwe_words(p, a, b if k % 2 == 0 else b[::-1])) for k, (label, a) in enumerate(rows)]


def randomised_lwes(p, bp, key, call):
    """Two ciphertexts (ct = 0 draws with z = 0, ct = 1 with z = 1): a[j][i] = x0 + x1 B + (top | bottom) by the sign of
    the draws of (call, ct, slice i, coefficient j) -- see the module docstring."""
    n, Q, B = p.n, p.Q, p.B
    top, bot = R.extreme_residue(p, +1), R.extreme_residue(p, -1)
    out = []
    for ct in range(2):
        rng = BO.ChaChaFlatten(bp, key, ct, call)
        a = [[0] * n for _ in range(n)]
        for i in range(n):
            f = rng.draws(0, (1 << 31) | i)
            for j in range(n):
                x0, x1 = f(j, 0), f(j, 1)
                a[j][i] = (x0 + x1 * B + (top if x0 + x1 >= 0 else bot)) % Q
        b = [0 if (j + ct) % 2 == 0 else Q - 1 for j in range(n)]
        out.append(("draw-aligned, ct %d" % ct, _lwe_words(p, a, b)))
    return out


def margin(sums, primes):
    """max |exact group sum| over 0.4 prod(primes)."""
    worst = max(abs(x) for grp in sums for col in grp for x in col)
    return worst / (0.4 * math.prod(primes))


# ---- the comparison --------------------------------------------------------------------------------------------------------

def _ring(S, name):
    return KC.ring(S, name)


@pytest.fixture(scope="module", params=NAMES)
def ring(S, oc, request):
    rg = _ring(S, request.param)
    eng = S.Engine(rg.params)
    yield rg, eng, RC.oracles(oc, rg)[0]
    eng.close()


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_tail_on_chosen_operands(S, oc, ring, rnd):
    rg, eng, o = ring
    p = rg.params
    n = p.n
    bp = R.bigint_params(p)
    primes, G = basis(p, rnd)
    assert rg.pack[rnd] and G >= 1                        # (every ring of the table packs in both modes)
    rows = np.random.default_rng(620).integers(0, p.r, size=(4, 2, n + 1), dtype=np.uint64)
    boot = (rows[0, :, :n], rows[0, :, n], rows[1, :, :n], rows[1, :, n])
    worst = {}
    try:
        for pattern in KEY_PATTERNS:
            key = chosen_key(p, pattern)
            words = key_words(oc, p, key)
            RC.upload(eng, rg, words)
            fast = R.FastTail(bp, key)
            # the call number is the one the ctx is at: the mode is set immediately before (the counter starts at 0)
            assert RC.set_mode(S, eng, rg, rnd)
            assert eng.primes() == primes, (rg.name, rnd)
            cts = randomised_lwes(p, bp, RC.KEY32, 0) if rnd else deterministic_lwes(p)
            w, v = eng.pack_lwe_modq(np.stack([x for _, x in cts]))
            assert w.shape == v.shape == (len(cts), p.m)
            for ct, (label, lwe) in enumerate(cts):
                fw, fv, sums = fast(lwe, seed=RC.KEY32 if rnd else None, ct=ct, call=0, exact=G)
                where = "%s, %s, key %s, LWEs %s" % (rg.name, RC.MODE_IDS[rnd], pattern, label)
                assert len(sums) == n // G
                assert np.array_equal(w[ct], fw), where + ": w"
                assert np.array_equal(v[ct], fv), where + ": v"
                if rg.name == BIGINT_RING:
                    bw, bv = R.tail_bigint(bp, key, lwe, seed=RC.KEY32 if rnd else None, ct=ct, call=0)
                    assert np.array_equal(fw, bw) and np.array_equal(fv, bv), where + ": FastTail against tail_bigint"
                worst[(pattern, label)] = margin(sums, primes)
            if rnd:     # the tail took call 0 and no bootstrap draws: the next bootstrap call is call 1
                khat = o.key_transform(words, threads=oracle_threads())    # (the default is every core)
                want = o.bootstrap_batch(khat, *boot, opt=True, rnd=(RC.KEY32, 1))
                assert np.array_equal(eng.bootstrap_batch(*boot), want), (rg.name, pattern, "call 1")
    finally:
        eng.set_random_flatten(False)
    top = max(worst, key=worst.get)
    sized = G * p.m * p.B * p.Q // 2 * (4 if rnd else 1)      # what derive_basis sizes pack_G for
    print("pack margin %-9s %-13s %d primes, G = %2d of n = %2d (%d groups): max |group sum| = %.3g of 0.4 M, %.3g of the "
          "G m B Q / 2%s the group is sized for  (key %s, LWEs %s)"
          % (rg.name, RC.MODE_IDS[rnd], len(primes), G, n, n // G, worst[top],
             worst[top] * 0.4 * math.prod(primes) / sized, " x 4" if rnd else "", top[0], top[1]))


def test_some_ring_runs_more_than_one_group(S):
    """From the sizing rule (test_tail_on_chosen_operands holds its primes to the engine's): the stage sums the groups'
    CRTs mod Q in k_pack_finish only where pack_G < n."""
    groups = {(name, rnd): _ring(S, name).params.n // basis(_ring(S, name).params, rnd)[1]
              for name in NAMES for rnd in RC.MODES}
    assert groups[("limb64", False)] == 2 and groups[("synth32", False)] == 8, groups
    assert any(g > 1 for (name, _), g in groups.items() if name in RC.NAMES)
