"""TEST INFRASTRUCTURE: the cases of bootstrap-key generation, once (tests/test_keygen_host.py, tests/test_gpu_keygen.py).

Rings: the five kinds of tests/ring_cases.py and two more that only the key tests need (they are not in ring_cases.NAMES,
which every test of tests/test_gpu_rings.py runs over):

  synth32    n = 32, m = 256, Q ~ 2^50, B = 2^26 (test_small_synthetic_bootstrap at n = 32): 128 key rows = two batches
             of sgfhe_bkey_generate, the k_shat / k_polymul_s of m = 256, and a ctx with a basis per flatten mode (three
             primes deterministic, four randomised), so that k_key_derive runs after the generation
  q16        n = 8, Q = 65537, the smallest modulus sgfhe_bkey_generate accepts (Q >= 2^16), B = 2^9 - 1 (the recipe of
             `tiny`, Q < 2^30 and an odd B < 2^12, scaled down: B^2 ~ 4 Q); deterministic mode only.  No noise: as on
             `tiny`, one noisy external product would use up what a bootstrap input may be off by

n = 8 has 32 key rows, fewer than the batch of 64 rows sgfhe_bkey_generate works in; n = 16 has exactly one batch; n = 32
two.  m = 64, 128 and 256 are the k_shat / k_polymul_s instantiations no Params(n) of the reference reaches.

Per ring, `cases(rg)` is a cross, not a product: every noise bound under the oracle's secret key and the small seed, every
secret key and every seed under the ring's own noise -- (noise, secret-key name, seed) triples, the first one the ring's
plain case."""

import bigint_oracle as BO
import numpy as np

import ring_cases as RC

NAMES = RC.NAMES + ("synth32", "q16")
SK_SEED = 601                                         # oracle.private_key(SK_SEED + index of the ring)
SEEDS = (602, bytes([0xFF] * 32), bytes(range(1, 33)))
SK_KINDS = ("oracle", "zeros", "ones", "last bit")
NOISE_MAX = (1 << 30) - 1                             # sgfhe_bkey_generate forms the noise in int32


def ring(S, name):
    """ring_cases.Ring; `modes`: the flatten modes the key tests run the ring in."""
    if name == "synth32":
        n = 32
        Q = BO.find_modulus(16 * n, 1 << 50)
        B = 1 << ((Q.bit_length() + 1) // 2)
        assert B == 1 << 26
        rg = RC.Ring(name, S.Params.custom(n, Q, B), 2,
                     {False: ("k_extprod<8, 3, false>", "k_crt_lean<3, 2>"),
                      True: ("k_extprod<8, 3, false>", "k_crt_lean_rnd<4, 2, false>")})
    elif name == "q16":
        n = 8
        Q, B = BO.find_modulus(16 * n, 1 << 16), (1 << 9) - 1
        assert Q == 65537 and B * B >= Q
        rg = RC.Ring(name, S.Params.custom(n, Q, B), 0,
                     {False: ("k_extprod<6, 3, false>", "k_crt_acc2<2>")})
    else:
        rg = RC.ring(S, name)
    rg.modes = (False,) if name == "q16" else RC.MODES
    return rg


def noise_max(Q):
    """The largest bound sgfhe_bkey_generate and the oracles accept: below 2^30, and 2 noise < Q."""
    return min(NOISE_MAX, (Q - 1) // 2)


def noises(rg):
    p = rg.params
    out = []
    for x in (rg.noise, 0, 1, p.n, noise_max(p.Q)):
        if x not in out:
            out.append(x)
    return out


def secret_key(o, rg, kind):
    n = rg.params.n
    if kind == "oracle":
        return o.private_key(SK_SEED + NAMES.index(rg.name))
    sk = np.zeros(n, dtype=np.uint64)
    if kind == "ones":
        sk[:] = 1
    elif kind == "last bit":
        sk[n - 1] = 1
    else:
        assert kind == "zeros"
    return sk


def cases(rg):
    out = [(x, "oracle", SEEDS[0]) for x in noises(rg)]
    out += [(rg.noise, kind, SEEDS[0]) for kind in SK_KINDS[1:]]
    out += [(rg.noise, "oracle", seed) for seed in SEEDS[1:]]
    return out


def case_id(case):
    noise, kind, seed = case
    return "noise %d, %s key, seed %s" % (noise, kind, seed if isinstance(seed, int) else seed[:2].hex() + "..")
