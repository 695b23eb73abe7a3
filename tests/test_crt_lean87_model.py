"""Host model of crt_lean87_one (kernels.h): k_crt_lean's arithmetic specialised to five primes, Q of
87 bits and B of 44 bits (Params(1024)).  Every intermediate is checked against the register it lives
in, both quotient estimates against the exact quotients, and the digits against the generic form
(rns_model.CrtLean) and the exact (x_old + D) mod Q, on every parameter set the engine hands the
specialisation (derive_basis of csrc/constants.h: npr = 5, bits(Q) = 87, bits(B) = 44) and at the edges of that range."""

import random

import pytest

import rns_model as RM

M32, M64, M96 = (1 << 32) - 1, (1 << 64) - 1, (1 << 96) - 1


def accepts(C):
    """derive_basis: the engine takes crt_lean87_one for this ctx."""
    return C.npr == 5 and C.Q.bit_length() == 87 and C.B.bit_length() == 44


def u64(v):
    assert 0 <= v <= M64, "64-bit register"
    return v


def u32(v):
    assert 0 <= v <= M32, "32-bit register"
    return v


def mad(a, b, c):
    """v_mad_u64_u32: 32 x 32 + 64 bits, no carry out."""
    return u64(u32(a) * u32(b) + u64(c))


def mulhi64_87(x, m):
    """mulhi64_87 of kernels.h: (x m) >> 64 without the low half of x0 m0."""
    x0, x1, m0, m1 = x & M32, x >> 32, m & M32, m >> 32
    assert m1 < (1 << 24)
    t1 = mad(x0, m1, (x0 * m0) >> 32)
    t2 = mad(x1, m0, t1)
    return mad(x1, m1, t2 >> 32)


class Lean87:
    def __init__(self, C):
        assert accepts(C)
        self.C, self.L = C, RM.CrtLean(C)
        assert self.L.ok and self.L.NL == 3 and self.L.a == 0
        self.mq = (1 << 122) // C.Q
        self.mb = (1 << 96) // C.B
        assert self.mq <= (1 << 36) and self.mb <= (1 << 53)

    def digits(self, y, lo_o, hi_o):
        C, L = self.C, self.L
        Q, B = C.Q, C.B
        assert lo_o < (1 << 48) and hi_o < (1 << 48)
        acc = 0
        for i in range(5):
            acc = mad(y[i], L.w[i], acc)
        alpha = acc >> 58
        yl = list(y)
        yl[4] = u32(y[4] - L.hoff)
        h0, h1 = hi_o & M32, hi_o >> 32
        B0x8, B1x8 = u32(L.B0 << 3), u32(L.B1 << 3)
        L0 = mad(h0, L.B0, lo_o)
        L1 = mad(h1, B0x8, mad(h0, L.B1, 0))
        L2 = mad(h1, B1x8, 0)
        for i in range(5):
            L0 = mad(yl[i], L.c[i][0], L0)
            L1 = mad(yl[i], L.c[i][1], L1)
            L2 = mad(yl[i], L.c[i][2], L2)
        L0 = mad(alpha, L.cMn[0], L0)
        L1 = mad(alpha, L.cMn[1], L1)
        L2 = mad(alpha, L.cMn[2], L2)
        U = mad(L1 & M32, 1 << 29, L0)
        X = mad(L1 >> 32, 8, L2)
        S = U + (X << 58)
        assert S == L0 + (L1 << 29) + (L2 << 58)
        q = mulhi64_87(X, self.mq)
        assert S // Q - 1 <= q <= S // Q, "quotient estimate"
        qa, qb = q & M32, q >> 32
        # q Q modulo 2^96 as the device forms it
        p0 = mad(qa, C.Q & M32, 0)
        p1 = mad(qa, (Q >> 32) & M32, p0 >> 32)
        p2 = ((p1 >> 32) + qa * (Q >> 64) + qb * ((Q >> 32) & M32)) & M32
        p12 = (((p2 << 32) | (p1 & M32)) + qb * (Q & M32)) & M64
        assert (p12 << 32 | (p0 & M32)) == (q * Q) & M96
        s12 = ((U >> 32) + (X << 26)) & M64
        assert (s12 << 32 | (U & M32)) == S & M96
        x = ((s12 << 32 | (U & M32)) - (p12 << 32 | (p0 & M32))) & M96
        assert x == S - q * Q and x < 2 * Q
        if x >= Q:          # the borrow chain x - Q does not borrow
            x -= Q
        X2 = x >> 32
        hq = mulhi64_87(X2, self.mb)
        assert x // B - 1 <= hq <= x // B, "digit estimate"
        g0, g1 = hq & M32, hq >> 32
        pb = mad(g0, B & M32, 0)
        pbh = ((pb >> 32) + g0 * (B >> 32) + g1 * (B & M32)) & M32
        assert (pbh << 32 | (pb & M32)) == (hq * B) & M64
        lo = ((x & M64) - (pbh << 32 | (pb & M32))) & M64
        assert lo == x - hq * B and lo < 2 * B
        if lo >= B:
            lo -= B
            hq += 1
        assert hq < (1 << 48)
        return lo, hq, alpha


def _cases():
    import bench
    import sgfhe_jl_amd as S
    for name in ("params1024", "rns2"):
        p = bench.make_params(S, name)
        yield name, (p.n, p.m, p.Q, p.B, p.DQ_tilde)
    # the edges of what derive_basis hands the specialisation: Q of 87 bits, B of 44 bits
    for i, (Q, B) in enumerate((((1 << 86) + 1, 1 << 43), ((1 << 87) - 1, (1 << 44) - 1),
                                ((1 << 86) + 1, (1 << 44) - 1), ((1 << 87) - 1, 1 << 43),
                                ((1 << 87) - 12345, (1 << 43) + 987), (0x5a5a5a5a5a5a5a5a5a5a5b, 0xb0b0b0b0b0b))):
        yield "edge%d" % i, (8, 64, Q, B, Q // 8)


def test_engine_acceptance():
    """The parameter sets of the repo that take the specialisation, and those that do not."""
    import bench
    import sgfhe_jl_amd as S
    taken = set()
    for name in ("params1024", "params512", "params64", "synth64", "rns2", "params2048"):
        p = bench.make_params(S, name)
        if accepts(RM.Consts(p.n, p.m, p.Q, p.B, p.DQ_tilde)):
            taken.add(name)
    assert taken == {"params1024", "rns2"}


@pytest.mark.parametrize("name,args", list(_cases()), ids=[c[0] for c in _cases()])
def test_crt_lean87_model(name, args):
    C = RM.Consts(*args)
    F = Lean87(C)
    rnd = random.Random(hash(name) & 0xFFFF)
    E = RM.EngineModel.__new__(RM.EngineModel)
    E.C = C
    bound = min(int(0.4 * C.Mrns), 2 * C.M * C.B * C.Q)
    inv = [pow(C.Mrns // p, -1, p) for p in C.primes]
    hoff = C.pk[-1]["hoff"]
    worst = [int(5.7 * p) for p in C.primes[:-1]] + [int(6.2 * C.primes[-1])]
    for it in range(3000):
        D = rnd.randint(-bound, bound)
        if it % 11 == 0:
            D = rnd.choice([bound, -bound, 0, 1, -1])
        y = []
        for i, p in enumerate(C.primes):
            r = D * inv[i] % p
            r += rnd.randint(0, 5 if r < 0.7 * p else 4) * p
            y.append(r + C.pk[i]["hoff"])
        xo = rnd.randrange(C.Q)
        if it % 7 == 0:
            xo = rnd.choice([0, C.Q - 1, C.B - 1, C.B % C.Q, (C.Q - C.B) % C.Q])
        if it % 13 == 0:
            xo = (-D + rnd.choice([0, 1, -1, C.B, C.B - 1])) % C.Q
        lo, hq, alpha = F.digits(y, xo % C.B, xo // C.B)
        xn = E.crt_value(y, xo)
        assert alpha == E.last_alpha and xn == (xo + D) % C.Q
        assert (lo, hq) == (xn % C.B, xn // C.B)
        assert (lo, hq, alpha) == F.L.digits(y, xo % C.B, xo // C.B)
    # register widths at the largest inputs: residues at 5.7 p_i and 6.2 p_last, old digits at B - 1
    # and floor(Q / B) (not congruent to anything: only the widths and the estimates are checked)
    for lo_o in (0, C.B - 1):
        for hi_o in (0, C.Q // C.B):
            for k in range(64):
                y = [w if (k >> i) & 1 else rnd.randrange(hoff if i == 4 else 0, w + 1)
                     for i, w in enumerate(worst)]
                F.digits(y, lo_o, hi_o)
