"""TEST INFRASTRUCTURE: the ring kinds the ctx accepts, once (tests/test_ring_mirrors_host.py, tests/test_gpu_rings.py).

Every ring is built from the recipe of the test that first ran a bootstrap on it, at n = 8 or 16 where the C oracle
costs milliseconds:

  tiny       n = 8, Q < 2^30, B < 2^12 (test_flatten_kernel_exhaustive_small_moduli): outside the bounds of the lean CRT
             kernels -- k_crt_acc2 deterministic, k_crt_acc randomised; an odd base
  limb64     n = 8, Q just below 2^64, B = 2^43 (test_two_basis_ctx_on_a_small_ring): high word 0, low word near 2^64;
             four primes deterministic, five randomised
  wide       n = 8, Q ~ 2^92, B = 3 2^45 + 1 (test_random_mode_equals_oracle_bit_for_bit): MODE_WIDE, six primes, four
             29-bit limbs, Q close to the ctx's limit of 2^94
  composite  n = 16, Q = B B' by the rule of fhe2.jl, the key uploaded as RNS2Number limb pairs
             (test_rns2_small_ring_three_ways): Q is no prime
  m128       n = 16, Q ~ 2^52, B = 2^27 (test_random_mode_equals_oracle_bit_for_bit, "synthetic"): m = 128, the other pass
             structure of the small NTT

`kernels[rnd]` is what Engine.kernel_names() must report in that flatten mode, derived from crt_form of csrc/engine.hip
and plan_bases / derive_basis of csrc/constants.h: the primes are the fewest below 2^29 whose product covers 5 m B Q (20 m B Q randomised), the limbs
ceil(bits of Q / 29) with two at least, and the lean kernels need B >= 2^12 and Q >= 2^29.  `random`: the ctx has the
randomised mode (2 log2 B + 2 - log2 Q < 50; all five do), `pack[rnd]`: the pack stage in that mode (the primes chosen
for the k-loop leave the factor 0.8 n its sums need on all five).  `noise`: the bound of the key's error draws -- 2 as in the
recipes, 0 on `tiny`, where one noisy external product (about sqrt(4 m) B / 2 = 2^15 per unit of noise and iteration)
would use up the Q / 64 = 2^17 that a LUT input may be off by.
"""

import numpy as np

import bigint_oracle as BO

NAMES = ("tiny", "limb64", "wide", "composite", "m128")
KEY32 = bytes(range(1, 33))
ERR_UNSUPPORTED = -2                                    # SGFHE_ERR_UNSUPPORTED
MODES = (False, True)
MODE_IDS = ("deterministic", "randomised")


class Ring:
    def __init__(self, name, params, noise, kernels, random=True, rns2=None, pack=(True, True)):
        self.name, self.params, self.noise, self.kernels, self.random, self.rns2 = name, params, noise, kernels, random, rns2
        self.pack = {False: pack[0], True: pack[1]}    # the pack stage exists in that mode (the primes' exactness bound)


def ring(S, name):
    if name == "tiny":
        n = 8
        Q, B = BO.find_modulus(16 * n, 1 << 23), (1 << 12) - 1
        assert Q < 1 << 30 and B < 1 << 12
        return Ring(name, S.Params.custom(n, Q, B), 0,
                    {False: ("k_extprod<6, 3, false>", "k_crt_acc2<2>"), True: ("k_extprod<6, 3, false>", "k_crt_acc<2>")})
    if name == "limb64":
        n = 8
        Q = BO.find_modulus(16 * n, (1 << 64) - (1 << 40))
        assert (1 << 63) < Q < 1 << 64
        return Ring(name, S.Params.custom(n, Q, 1 << 43), 2,
                    {False: ("k_extprod<6, 3, false>", "k_crt_lean<4, 3>"),
                     True: ("k_extprod<6, 3, false>", "k_crt_lean_rnd<5, 3, false>")})
    if name == "wide":
        n = 8
        Q, B = BO.find_modulus(16 * n, 1 << 92), 3 * (1 << 45) + 1
        assert B >= 1 << 46 and (1 << 92) <= Q < 1 << 93
        return Ring(name, S.Params.custom(n, Q, B), 2,
                    {False: ("k_extprod<6, 3, false>", "k_crt_lean<6, 4>"),
                     True: ("k_extprod<6, 3, true>", "k_crt_lean_rnd<6, 4, true>")})
    if name == "composite":
        n, m = 16, 128
        Bp = BO.find_modulus(2 * m, 1 << 24)
        B = BO.find_modulus(2 * m, Bp + 1)                  # rule of src/fhe2.jl:57-58
        return Ring(name, S.Params.custom(n, B * Bp, B), 2,
                    {False: ("k_extprod<7, 3, false>", "k_crt_lean<3, 2>"),
                     True: ("k_extprod<7, 3, false>", "k_crt_lean_rnd<3, 2, false>")}, rns2=(B, Bp))
    if name == "m128":
        n = 16
        return Ring(name, S.Params.custom(n, BO.find_modulus(16 * n, 1 << 52), 1 << 27), 2,
                    {False: ("k_extprod<7, 3, false>", "k_crt_lean<4, 2>"),
                     True: ("k_extprod<7, 3, false>", "k_crt_lean_rnd<4, 2, false>")})
    raise KeyError(name)


def moduli(S):
    """{name: (Q, r, DQ_tilde)} of the table and of the reference's Params(64), (1024) and (2048)."""
    out = {}
    for name in NAMES:
        p = ring(S, name).params
        out[name] = (p.Q, p.r, p.DQ_tilde)
    for n in (64, 1024, 2048):
        p = S.Params(n)
        out["params%d" % n] = (p.Q, p.r, p.DQ_tilde)
    return out


def oracles(oc, rg):
    """(the standard C oracle, the low-amplitude one of lut_ref.low_oracle) of a ring; over the composite modulus both
    multiply limb-wise (rns.jl:51-60)."""
    p = rg.params
    return (oc.Oracle(p.n, p.r, p.m, p.Q, p.B, p.DQ_tilde, rns2=rg.rns2),
            oc.Oracle(p.n, p.r, p.m, p.Q, p.B, p.DQ_tilde >> 2, rns2=rg.rns2))


def upload(eng, rg, bkey):
    """The key in the ring's own form: RNS2Number limb pairs over the composite modulus, canonical residues elsewhere."""
    if rg.rns2 is None:
        eng.upload_key(bkey)
        return
    B, Bp = rg.rns2
    flat = np.ascontiguousarray(bkey).reshape(-1, 2)
    pairs = np.array([BO.rns2_from_int(int(lo) | (int(hi) << 64), B, Bp) for lo, hi in flat], dtype=np.uint64)
    eng.upload_key_rns2(pairs.reshape(bkey.shape), B, Bp)


def set_mode(S, eng, rg, rnd, key=KEY32):
    """Put the ctx into a flatten mode (the call counter starts again at 0) and hold kernel_names() to the table.  Returns
    False where the ring has no randomised mode: the documented refusal is asserted, the ctx stays deterministic."""
    if rnd and not rg.random:
        try:
            eng.set_random_flatten(True, key)
        except S.SgfheError as e:
            assert e.code == ERR_UNSUPPORTED
            assert eng.kernel_names() == rg.kernels[False]
            return False
        raise AssertionError("%s: the randomised mode was expected to be refused" % rg.name)
    eng.set_random_flatten(bool(rnd), key if rnd else 0)
    assert eng.kernel_names() == rg.kernels[bool(rnd)], (rg.name, rnd, eng.kernel_names())
    return True


# ---- the mixed circuit ------------------------------------------------------------------------------------------------

def mixed_circuit(S, form="lwe"):
    """Eleven nodes in three levels, group = 4.  Level 1: three refreshes.  Level 2: two fans, a classic gate with a NOT
    input, a gate3, a sum node with a weight of 2 whose other term is lane-shifted out of the group at lane 3.  Level 3:
    a LUT node on lane-shifted scaled wires, a LUT node that reads a negated scale-1 wire and the constant, and a classic
    gate that reads the XOR3 wire.  form "lwe": outputs with a negated wire, a lane-shifted one and the constant;
    "ct": a direct gate wire, its negation, the XOR3 wire, a LUT wire, a negated LUT wire, an input and the constant."""
    c = S.Circuit(3, group=4)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy = c.fan(rx), c.fan(ry)
    g = c.gate(rx, ~ry)
    t = c.gate3(rx, ry, rz)
    s = c.sum_node([(2, rx), (1, rz.lane(1))])
    la = c.lut(0x96, fy[2].lane(-1), fx[1].lane(2), g[1])
    lb = c.lut(0xCA, fx[2], ~fy[1], S.Circuit.TRUE)
    g3 = c.gate(t[2], s[0])
    if form == "lwe":
        c.output(la[0], ~lb[0], g3[1], t[2], s[1], S.Circuit.TRUE, ~g[0].lane(1), g3[2])
    else:
        c.output(g3[1], ~g3[1], t[2], la[0], ~lb[0], c.inputs[0], S.Circuit.TRUE)
    assert [len(level) for level in c.schedule()] == [3, 5, 3]
    return c
