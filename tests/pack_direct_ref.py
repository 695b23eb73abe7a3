"""What the tests of the direct pack stage share (tests/test_pack_direct_host.py, tests/test_gpu_pack_direct.py): the
tail of pack_encrypted_bits (src/fhe.jl:675-695) composed from the big-int oracle on LWEs over Z_Q, the circuit whose
outputs take every path of the stage, and the packed phase error."""

import numpy as np

import bigint_oracle as BO

KEY32 = bytes(range(1, 33))


def key_lists(oc, bkey, n, m):
    """The C oracle's key [n][4][2][m][2] as the big-int oracle's key[k][row][col] = list of m residues."""
    vals = oc.u128_to_ints(bkey)
    return [[[vals[((k * 4 + r) * 2 + c) * m:((k * 4 + r) * 2 + c + 1) * m] for c in range(2)]
             for r in range(4)] for k in range(n)]


def bigint_params(params):
    return BO.Params.custom(params.n, params.Q, params.B, DQ_tilde=params.DQ_tilde)


def tail_bigint(bp, bk, lwe_q, seed=None, ct=0, call=0):
    """fhe.jl:675-695 on n LWEs over Z_Q (lwe_q [n][n + 1][2] uint64): as_i from the i-th coefficients, the n
    half-width external products, the sums, ModRed.  seed = None: rng = nothing; else ciphertext `ct` of call `call`
    on the engine's ChaCha stream (the flatten of as_i draws with y = 2^31 | i, z = ct).  -> (w, v), [m] uint64."""
    n, m, Q = bp.n, bp.m, bp.Q
    vals = np.asarray(lwe_q, dtype=np.uint64).reshape(n, n + 1, 2)
    ints = [[int(lo) | (int(hi) << 64) for lo, hi in row] for row in vals]
    as_ = [BO.resize([ints[j][i] for j in range(n)], m) for i in range(n)]          # fhe.jl:675-677
    b = BO.resize([ints[j][n] for j in range(n)], m)                                # fhe.jl:678
    w_tilde, v_tilde = [0] * m, [0] * m
    pack_rng = None if seed is None else BO.ChaChaFlatten(bp, seed, ct, call)
    for i in range(n):                                                              # fhe.jl:683-687
        draws = None if seed is None else pack_rng.draws(0, (1 << 31) | i)
        w, v = BO.shortened_external_product(as_[i], bk[i], bp.B, bp.ell, Q, draws)
        w_tilde = BO.poly_add(w_tilde, w, Q)
        v_tilde = BO.poly_add(v_tilde, v, Q)
    w1 = [(Q - x) % Q for x in w_tilde]                                             # fhe.jl:689
    v1 = BO.poly_sub(b, v_tilde, Q)                                                 # fhe.jl:690
    return (np.array(BO.reduce_modulus_poly(bp.r, w1, Q), dtype=np.uint64),         # fhe.jl:692-693
            np.array(BO.reduce_modulus_poly(bp.r, v1, Q), dtype=np.uint64))


def extreme_residue(p, sign):
    """The residue whose deterministic flatten digits are both as large (sign > 0) or both as small (sign < 0) as a
    residue of Z_Q allows: x' = value + off at the top / bottom of [0, Q) (tests/test_gpu_worstcase.py drives the k-loop's
    CRT with it, tests/test_gpu_pack_bound.py the pack stage's)."""
    s = p.B // 2 - 1 if p.B % 2 == 0 else (p.B - 1) // 2
    off = (1 + p.B) * s % p.Q
    if sign > 0:
        hi_max = (p.Q - 1) // p.B
        xp = (hi_max - 1) * p.B + (p.B - 1)           # digits (B - 1 - s, hi_max - 1 - s)
    else:
        xp = 0                                         # digits (-s, -s)
    return (xp - off) % p.Q


class FastTail:
    """tail_bigint in exact integer arithmetic, an order of magnitude faster (tests/test_pack_direct_host.py checks the
    two against each other): the digits of flatten / flatten_random (src/utils.jl:155-241) as SIGNED integers on whole
    polynomials at once, and all 2 n products of a column summed as one Kronecker integer before it is unpacked and
    reduced mod (x^m + 1, Q).  The key rows are packed once, lifted to (-Q/2, Q/2] as k_key_transform lifts them, so the
    integers summed here are the ones the pack stage's CRT has to recover.  `exact=G` also returns them: the sums of every
    group of G slices, [n / G][2][m] Python integers, before the reduction mod Q (tests/test_gpu_pack_bound.py)."""

    def __init__(self, bp, bk):
        self.bp = bp
        n, m, Q, B = bp.n, bp.m, bp.Q, bp.B
        # a coefficient of the sum: 2 n products of m terms, digits below 2 B in size, key residues below Q; signed
        self.slot = (Q.bit_length() + (2 * B).bit_length() + (2 * n * m).bit_length() + 2 + 7) // 8
        self.half = 1 << (8 * self.slot - 1)
        self.off = sum(self.half << (8 * self.slot * k) for k in range(2 * m))
        centred = lambda row: [x - Q if x > Q // 2 else x for x in row]
        self.K = [[[self._pack_signed(centred(bk[i][bp.ell + d][c])) for c in range(2)] for d in range(2)]
                  for i in range(n)]

    def _pack(self, coeffs):
        return int.from_bytes(b"".join(int(x).to_bytes(self.slot, "little") for x in coeffs), "little")

    def _pack_signed(self, coeffs):
        return self._pack([v if v > 0 else 0 for v in coeffs]) - self._pack([-v if v < 0 else 0 for v in coeffs])

    def _unpack(self, acc):
        """A Kronecker product of two packed polynomials -> its m signed coefficients mod x^m + 1."""
        m = self.bp.m
        raw = (acc + self.off).to_bytes(2 * m * self.slot + 1, "little")
        co = [int.from_bytes(raw[k * self.slot:(k + 1) * self.slot], "little") - self.half for k in range(2 * m)]
        return [co[k] - co[k + m] for k in range(m)]

    def _digits(self, a, x):
        """a: object array of residues; x: None, or the draws (x0, x1) as object arrays -> signed digits (d0, d1)."""
        B, Q = self.bp.B, self.bp.Q
        s = (B - 1) // 2 if B % 2 else B // 2 - 1                  # utils.jl:162-166
        if x is not None:
            a = (a - x[0] - x[1] * B) % Q                          # utils.jl:233-234
        a = (a + (1 + B) * s) % Q                                  # utils.jl:179
        d0, d1 = a % B - s, a // B - s                             # utils.jl:170-185
        return (d0, d1) if x is None else (d0 + x[0], d1 + x[1])   # utils.jl:237-239

    def __call__(self, lwe_q, seed=None, ct=0, call=0, exact=None):
        bp = self.bp
        n, m, Q = bp.n, bp.m, bp.Q
        G = n if exact is None else exact
        assert n % G == 0
        vals = np.asarray(lwe_q, dtype=np.uint64).reshape(n, n + 1, 2)
        ints = np.array([[int(lo) | (int(hi) << 64) for lo, hi in row] for row in vals], dtype=object)   # [bit][n + 1]
        rng = None if seed is None else BO.ChaChaFlatten(bp, seed, ct, call)
        acc = [[0, 0] for _ in range(n // G)]
        zero = np.array([0] * (m - n), dtype=object)
        for i in range(n):
            a = np.concatenate([ints[:, i], zero])                 # as_i, resized (fhe.jl:675-677)
            x = None
            if rng is not None:
                f = rng.draws(0, (1 << 31) | i)
                x = tuple(np.array([f(j, d) for j in range(m)], dtype=object) for d in range(2))
            for d, dig in enumerate(self._digits(a, x)):
                P = self._pack_signed(dig)
                acc[i // G][0] += P * self.K[i][d][0]
                acc[i // G][1] += P * self.K[i][d][1]
        sums = [[self._unpack(a[c]) for c in range(2)] for a in acc]
        cols = [[sum(s[c][k] for s in sums) % Q for k in range(m)] for c in range(2)]
        b = BO.resize([int(ints[j, n]) for j in range(n)], m)                           # fhe.jl:678
        w1 = [(Q - x) % Q for x in cols[0]]                                             # fhe.jl:689
        v1 = BO.poly_sub(b, cols[1], Q)                                                 # fhe.jl:690
        out = (np.array(BO.reduce_modulus_poly(bp.r, w1, Q), dtype=np.uint64),          # fhe.jl:692-693
               np.array(BO.reduce_modulus_poly(bp.r, v1, Q), dtype=np.uint64))
        return out if exact is None else out + (sums,)


def oracle_tail(bp, bk, key):
    """`tail(call, lwe_q)` of circuit.replay_ct_direct on the big-int oracle; key = None: deterministic."""
    fast = FastTail(bp, bk)

    def tail(call, group):
        res = [fast(g, seed=key, ct=ct, call=call) for ct, g in enumerate(group)]
        return np.stack([w for w, _ in res]), np.stack([v for _, v in res])
    return tail


def oracle_boot(o, bkey, key, raw=True):
    """`boot_raw(call, ...)` of circuit.replay_ct_direct (raw = False: `boot` of replay_levels) on the C oracle, through
    its NTT-domain key (same bytes, a third of the time)."""
    khat = o.key_transform(bkey)
    return lambda call, a1, b1, a2, b2: o.bootstrap_batch(khat, a1, b1, a2, b2, raw=raw, opt=True,
                                                          rnd=(key, call) if key else None)


def direct_circuit(S):
    """Two levels; outputs AND, ~OR, XOR (direct, two producing calls), an input, a negated input, TRUE (refreshed),
    and one gate wire named twice."""
    c = S.Circuit(3)
    x, y, z = c.inputs
    g1 = c.gate(x, y)
    g2 = c.gate(g1[2], ~z)
    c.output(g1[0], ~g2[1], g2[2], x, ~y, S.Circuit.TRUE, g1[0])
    return c


def phase_error(params, sk, w, v, bits):
    """Worst |phase - bit * Dr| over the n message coefficients of one packed ciphertext (w, v [m] over Z_r): what
    decrypt(key, ::Ciphertext) (src/fhe.jl:471-494) has before it snaps, centred."""
    r = params.r
    prod = BO.poly_mul_mod_pow2([int(x) for x in w], BO.resize([int(x) & 1 for x in sk], params.m), r)
    worst = 0
    for i in range(params.n):
        d = (int(v[i]) - prod[i] - int(bits[i]) * params.Dr) % r
        worst = max(worst, min(d, r - d))
    return worst
