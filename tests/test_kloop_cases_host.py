"""The chosen operands of one k-loop step (tests/kloop_cases.py) on the CPU, before any GPU test relies on them: every
built input is a pair a flatten stores (the rule sgfhe_debug_kloop_step refuses by) and the refusal cases are not;
`expected` equals the numpy model of the kernels (tests/rns_model.py, every int32 / int64 check on) on every family,
and the oracle's own flatten of acc + D; the quarter-form arithmetic takes the extreme operands inside its ranges."""

import numpy as np
import pytest

import bigint_oracle as BO
import kloop_cases as KC
import ring_cases as RC
import rns_model as RM

SEED = RC.KEY32
MODEL_RINGS = ("m128", "limb64", "wide")


def _ring(name):
    import sgfhe_jl_amd as S
    return RC.ring(S, name)


def _big_params():
    import sgfhe_jl_amd as S
    two_limb = S.Params.custom(512, BO.find_modulus(16 * 512, 1 << 52), 1 << 27)
    return [S.Params(512), S.Params(1024), S.Params(2048), two_limb]


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_every_built_input_is_storable(rnd):
    """All families, the wrap gates and the mixed calls, on the small rings and on the parameter sets of the GPU test:
    every pair passes the entry's rule; a pair one past each limit, and Q itself in the deterministic mode, do not."""
    import sgfhe_jl_amd as S
    views = [KC.RingView(RC.ring(S, name).params, rnd) for name in RC.NAMES]
    views += [KC.RingView(p, rnd) for p in _big_params()]
    for R in views:
        for name in KC.FAMILIES:
            dig = KC.family(R, name)
            assert dig.shape == (2, 2, R.m)
            assert all(KC.storable(R, int(lo), int(hi)) for c in range(2) for lo, hi in zip(dig[c, 0], dig[c, 1])), name
        digs, js = KC.mixed(R, 9)
        assert not (np.array_equal(digs[0], digs[-1]) and js[0] == js[-1]) and all(int(j) < 2 * R.m for j in js)
        for g in range(8):
            assert not (np.array_equal(digs[g], digs[g + 1]) and js[g] == js[g + 1])
        if R.m <= 128:
            for col, sl in ((0, "b to a"), (1, "a to b")):
                dig = KC.wrap_gate(R, KC.key_slice(R.p, sl), col, KC.family(R, "mid")[1 - col], R.m + 1,
                                   SEED if rnd else None, 3, 2, 1)
                assert all(KC.storable(R, int(lo), int(hi)) for c in range(2) for lo, hi in zip(dig[c, 0], dig[c, 1]))
        # the largest pair, and one past it in each digit
        assert KC.storable(R, R.top % R.B + R.draw_max, R.top // R.B + R.draw_max)
        assert not KC.storable(R, R.B + R.draw_max, 0) and not KC.storable(R, 0, R.hi_max + R.draw_max + 1)
        if not rnd:
            q_lo, q_hi = R.Q % R.B, R.Q // R.B
            assert q_hi <= R.hi_max + 1 and not KC.storable(R, q_lo, q_hi)
            assert KC.storable(R, (R.Q - 1) % R.B, (R.Q - 1) // R.B)
    # the top plane is in use where the engine keeps one (B >= 2^46 randomised), and only there
    for name in RC.NAMES:
        R = KC.RingView(RC.ring(S, name).params, rnd)
        peak = int(KC.family(R, "all +").max())
        assert (peak >= 1 << 48) == (bool(rnd) and R.B >= 1 << 46), name
        assert RM.digit_planes(peak, wide=peak >= 1 << 48) == peak


class _Model:
    """One ring and mode in the numpy model: k_extprod + k_crt_acc, and k_crt_lean[_rnd] where the set admits it."""

    def __init__(self, p, rnd):
        self.R = KC.RingView(p, rnd)
        self.E = RM.EngineModel(p.n, p.m, p.Q, p.B, p.DQ_tilde, random_flatten=rnd)
        self.L = RM.CrtLean(self.E.C)
        self.keys = {}

    def key(self, name):
        if name not in self.keys:
            C = KC.key_slice(self.R.p, name)
            self.keys[name] = (C, [[self.E.key_transform(C[rc // 2][rc % 2], pi) for rc in range(8)]
                                   for pi in range(self.E.C.npr)], KC.Products(self.R, C))
        return self.keys[name]

    def step(self, dig, slice_name, j, call, gate, k):
        """One gate through the model -> [2][2][m] stored digits."""
        R, E, L = self.R, self.E, self.L
        _, khat, _ = self.key(slice_name)
        pairs = [[(int(lo), int(hi)) for lo, hi in zip(dig[c, 0], dig[c, 1])] for c in range(2)]
        ys = E.extprod(pairs[0], pairs[1], khat, int(j), random=R.rnd)
        out = np.zeros((2, 2, R.m), dtype=np.uint64)
        key = KC.seed_int(SEED)
        for c in range(2):
            new = E.crt_acc(ys[c], pairs[c], rnd=(key, c, k + 1, gate, call) if R.rnd else None)
            out[c, 0], out[c, 1] = [d[0] for d in new], [d[1] for d in new]
            if not L.ok:
                continue
            span = 2 * R.xmax + 1
            for i in range(R.m):                       # the integer-only kernel on the same residues
                y = [int(ys[c][pi][i]) for pi in range(E.C.npr)]
                if R.rnd:
                    rv = RM.rnd128(key, ((c << R.logm) + i, k + 1, gate, call))
                    r0, r1 = (((rv[1] << 32) | rv[0]) * span) >> 64, (((rv[3] << 32) | rv[2]) * span) >> 64
                    lo, hi, _ = L.digits_random(y, pairs[c][i][0], pairs[c][i][1], r0, r1)
                else:
                    lo, hi, _ = L.digits(y, pairs[c][i][0], pairs[c][i][1])
                assert (lo, hi) == new[i], (c, i)
        return out


_MODELS = {}


def _model(name, rnd):
    if (name, rnd) not in _MODELS:
        _MODELS[(name, rnd)] = _Model(_ring(name).params, rnd)
    return _MODELS[(name, rnd)]


def _oracle_flatten(R, dig, D, call, gate, k):
    """The stored digits of acc + D by bigint_oracle.flatten_poly (src/utils.jl:155-241) with the stream's draws."""
    off = (1 + R.B) * R.shift
    rng = BO.ChaChaFlatten(R.p, SEED, gate, call) if R.rnd else None
    out = np.zeros((2, 2, R.m), dtype=np.uint64)
    for c in range(2):
        acc = [(int(lo) + int(hi) * R.B - off + d) % R.Q for lo, hi, d in zip(dig[c, 0], dig[c, 1], D[c])]
        u = BO.flatten_poly(acc, R.B, 2, R.Q, rng.draws(c, k + 1) if R.rnd else None)
        for d in range(2):
            out[c, d] = [(v if v <= R.Q // 2 else v - R.Q) + R.shift for v in u[d]]
    return out


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", MODEL_RINGS)
def test_model_equals_the_reference_on_every_family(name, rnd):
    """Every family once, the key slices and the rotations dealt round (every slice and every rotation at least once), at
    k = 0 and k = n - 1, gate indices 0 and up and a call number above 0: the model's stored digits (its range checks are
    the kernels' documented bounds) == expected == the oracle's flatten of acc + D."""
    M = _model(name, rnd)
    R = M.R
    rot = KC.rotations(R.m)
    call = 2
    digs = [KC.family(R, f) for f in KC.FAMILIES]
    for g, dig in enumerate(digs):
        sl = KC.SLICES[g % len(KC.SLICES)]
        j, k = rot[(3 * g + 1) % len(rot)], (0 if g & 1 else R.n - 1)
        C, _, prods = M.key(sl)
        got = M.step(dig, sl, j, call, g, k)
        jv = np.zeros(g + 1, dtype=np.uint32)
        jv[g] = j
        want = KC.expected(R.p, SEED if rnd else None, call, np.stack([dig] * (g + 1)), C, jv, k, prods)
        assert np.array_equal(got, want[g]), (name, rnd, KC.FAMILIES[g], sl, j)
        assert np.array_equal(want[g], _oracle_flatten(R, dig, KC.step_delta(R, prods, dig, j), call, g, k))
        if sl == "zero" and not rnd:
            assert np.array_equal(want[g], dig)          # the CRT stage alone is the identity
    assert {KC.SLICES[g % len(KC.SLICES)] for g in range(len(digs))} == set(KC.SLICES)
    assert {rot[(3 * g + 1) % len(rot)] for g in range(len(digs))} == set(rot)


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", MODEL_RINGS)
def test_value_wrap_in_the_model(name, rnd):
    """wrap_gate: the new value of the chosen column is 0, Q - 1, B - 1, B by turns (checked on the reference's result),
    and the model agrees -- the digit and modulus wrap of the flatten inside the CRT kernels."""
    M = _model(name, rnd)
    R = M.R
    for col, sl, j, gate, k in ((0, "b to a", R.m, 1, 0), (1, "a to b", 2 * R.m - 1, 0, R.n - 1)):
        C, _, prods = M.key(sl)
        dig = KC.wrap_gate(R, C, col, KC.family(R, "alternating")[1 - col], j, SEED if rnd else None, 5, gate, k)
        jv = np.full(gate + 1, j, dtype=np.uint32)
        want = KC.expected(R.p, SEED if rnd else None, 5, np.stack([dig] * (gate + 1)), C, jv, k, prods)[gate]
        nd = KC.next_draws(R, SEED, 5, gate, k)[col] if rnd else [[0] * R.m] * 2
        vals = [int(want[col, 0, i]) - nd[0][i] + (int(want[col, 1, i]) - nd[1][i]) * R.B for i in range(R.m)]
        assert vals == [KC.wrap_targets(R)[i % 4] for i in range(R.m)]
        assert np.array_equal(M.step(dig, sl, j, 5, gate, k), want)


# ---- the quarter form at m = 4096 (k_fwd_quarter / k_inv_quarter / k_ext_quarter, k_crt_lean1q / k_crt_lean_rnd1) ----------

def _signed_pack(poly, slot):
    pos = int.from_bytes(b"".join(max(int(c), 0).to_bytes(slot, "little") for c in poly), "little")
    neg = int.from_bytes(b"".join(max(-int(c), 0).to_bytes(slot, "little") for c in poly), "little")
    return pos - neg


def _exact_products(R, dig, C):
    """sum_row u_row (*) C[row][col] mod x^m + 1 over the INTEGERS, u the signed digits and the key residues lifted to
    (-Q/2, Q/2] as k_key_transform lifts them: the integers whose residues the transforms carry and the CRT recovers."""
    m, Q = R.m, R.Q
    slot = (R.B.bit_length() + 3 + Q.bit_length() + m.bit_length() + 3 + 8 + 7) // 8
    half = 1 << (8 * slot - 1)
    off = sum(half << (8 * slot * k) for k in range(2 * m))          # every coefficient non-negative in its slot
    pu = [_signed_pack([e - R.shift for e in dig[c, d].tolist()], slot) for c in range(2) for d in range(2)]
    out = []
    for col in range(2):
        tot = sum(pu[row] * _signed_pack([v if v <= Q // 2 else v - Q for v in C[row][col]], slot) for row in range(4)) + off
        b = tot.to_bytes(2 * m * slot + 1, "little")
        co = [int.from_bytes(b[k * slot:(k + 1) * slot], "little") - half for k in range(2 * m)]
        out.append([co[i] - co[i + m] for i in range(m)])
    return out


def _rotate_minus_one(P, j):
    m = len(P)
    rot = [0] * m
    for i, v in enumerate(P):
        k = (i + j) % (2 * m)
        rot[k % m] = -v if k >= m else v
    return [a - b for a, b in zip(rot, P)]


class _QuarterModel:
    """The steps of test_quarter_form_equals_the_whole_transforms (tests/test_rns_model.py) strung into one external
    product of the quarter form, for one prime: digit_reduce, the radix-4 head and the quarter-size forward transforms of
    the four digit rows, the products with the key rows summed per column, the factor psi^(j (2 brv(s) + 1)) - 1 per slot,
    the quarter-size inverse transforms and the last two stages -- every operation checked against int32 (RM.i32)."""

    def __init__(self, E, pi):
        from test_rns_model import _quarter_tables
        self.E, self.pi = E, pi
        self.P = P = E.C.pk[pi]
        self.logm, self.m = E.C.logm, E.C.M
        self.ms = self.m // 4
        self.sub = RM.NttModel(self.logm - 2, 3)
        self.QT = _quarter_tables(P, self.logm)
        p, R1 = P["p"], (1 << 32) % P["p"]
        pw, x = [], 1
        for _ in range(2 * self.m):                                  # PrimeK::pw: psi^e R, centred
            pw.append(RM.centre(x * R1, p))
            x = x * P["psi"] % p
        self.pw = np.array(pw, dtype=np.int64)
        self.br = np.array([RM.bitrev(s, self.logm) for s in range(self.m)], dtype=np.int64)

    def forward(self, dig, random):
        P, ms, sub = self.P, self.ms, self.sub
        f1, f2, f3, fp2, fp3 = (int(P["twf"][1]), int(P["twf"][2]), int(P["twf"][3]), int(P["twfp"][2]), int(P["twfp"][3]))
        U = []
        for c in range(2):
            for d in range(2):
                v = RM.i32(RM.sredc(dig[c, d].astype(np.int64), P) + (P["sRr"] if random else P["sR"]))
                assert int(np.abs(v).max()) <= P["p"] + (1 << 16)
                X = v.reshape(4, ms)
                u = RM.smont(X[2], f1, P)
                slots = []
                for q in range(4):
                    a = RM.i32(X[0] - u) if q & 2 else RM.i32(X[0] + u)
                    wB, wP = (f3, fp3) if q & 2 else (f2, fp2)
                    w = RM.sredc(RM.i32(X[1]) * wB + RM.i32(X[3]) * wP, P)
                    xq = RM.sred_floor(RM.i32(a - w) if q & 1 else RM.i32(a + w), P)
                    slots.append(sub.forward(sub.to_regs(xq), self.QT[q]["twf"], self.QT[q]).reshape(-1))
                U.append(np.concatenate(slots))
        return U

    def column(self, U, khat, c, j):
        """The residues k_crt_lean1q forms for column c: natural order, |.| < 1.5 * 2^29."""
        P, m, ms, sub = self.P, self.m, self.ms, self.sub
        z = np.zeros(m, dtype=np.int64)
        for row in range(4):
            z = RM.i32(z + RM.smont(U[row], khat[row * 2 + c], P))
        assert int(np.abs(z).max()) < 2.99 * 2 ** 29
        d = RM.scentre(RM.i32(self.pw[(j * (2 * self.br + 1)) % (2 * m)] - P["r1"]), P)    # rot_factors, rot_centre
        zr = RM.smont(z, d, P)
        assert int(np.abs(zr).max()) < 0.75 * 2 ** 29
        Y = [sub.from_regs(sub.inverse(zr[q * ms:(q + 1) * ms].reshape(sub.T, sub.E), self.QT[q]["twi"], self.QT[q]))
             for q in range(4)]
        assert max(int(np.abs(y).max()) for y in Y) < 1.4 * 2 ** 29
        v1, v2, v3 = int(P["twi"][1]), int(P["twi"][2]), int(P["twi"][3])
        c0, c2 = RM.sred(RM.i32(Y[0] + Y[1]), P), RM.sred(RM.i32(Y[2] + Y[3]), P)
        c1, c3 = RM.smont(RM.i32(Y[0] - Y[1]), v2, P), RM.smont(RM.i32(Y[2] - Y[3]), v3, P)
        got = np.concatenate([RM.i32(c0 + c2), RM.i32(c1 + c3), RM.smont(RM.i32(c0 - c2), v1, P), RM.smont(RM.i32(c1 - c3), v1, P)])
        assert int(np.abs(got).max()) < 1.5 * 2 ** 29
        return got


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_quarter_arithmetic_on_the_extreme_operands(rnd):
    """Params(512), m = 4096, the model's constants for it.  (a) One prime, extreme digits in halves against the slice whose
    rows all differ, every rotation of kloop_cases.rotations: the residues equal those of the exact integer D (times the
    CRT factor the key carries), inside every documented range.  (b) All primes, alternating digits and key residues,
    j = m + 1: the residues through k_crt_lean's integer algorithm (non-negative after + 3 p, the last prime's offset
    added) give the digits of `expected`."""
    import sgfhe_jl_amd as S
    p = S.Params(512)
    R = KC.RingView(p, rnd)
    E = RM.EngineModel(p.n, p.m, p.Q, p.B, p.DQ_tilde, random_flatten=rnd)
    C, L = E.C, RM.CrtLean(E.C)
    assert C.npr == 5 and L.ok
    # (a)
    Ck = KC.key_slice(p, "rows")
    dig = KC.family(R, "halves")
    M1 = _QuarterModel(E, 1)
    khat = [E.key_transform(Ck[rc // 2][rc % 2], 1) for rc in range(8)]
    U = M1.forward(dig, rnd)
    exact = _exact_products(R, dig, Ck)
    prods = KC.Products(R, Ck)
    pp, ei = M1.P["p"], M1.P["ei"]
    for j in KC.rotations(R.m):
        D = [_rotate_minus_one(exact[c], j) for c in range(2)]
        assert [[x % R.Q for x in D[c]] for c in range(2)] == KC.step_delta(R, prods, dig, j)
        assert max(abs(x) for c in range(2) for x in D[c]) * 5 < C.Mrns * 2          # |D| < 0.4 M: what the primes are sized for
        for c in range(2):
            got = M1.column(U, khat, c, j)
            assert np.array_equal(got % pp, np.array([x * ei % pp for x in D[c]], dtype=np.int64)), (j, c)
    # (b)
    Ck = KC.key_slice(p, "alternating")
    dig = KC.family(R, "alternating")
    j, k, gate, call = R.m + 1, 3, 2, 1
    ys = []
    for pi in range(C.npr):
        Mq = _QuarterModel(E, pi)
        khat = [E.key_transform(Ck[rc // 2][rc % 2], pi) for rc in range(8)]
        U = Mq.forward(dig, rnd)
        ys.append([Mq.column(U, khat, c, j) + 3 * Mq.P["p"] + Mq.P["hoff"] for c in range(2)])
    jv = np.zeros(gate + 1, dtype=np.uint32)
    jv[gate] = j
    want = KC.expected(p, SEED if rnd else None, call, np.stack([dig] * (gate + 1)), Ck, jv, k)[gate]
    nd = KC.next_draws(R, SEED, call, gate, k) if rnd else None
    for c in range(2):
        for i in range(R.m):
            y = [int(ys[pi][c][i]) for pi in range(C.npr)]
            assert all(0 <= v < 5.7 * C.primes[pi] + C.pk[pi]["hoff"] for pi, v in enumerate(y))
            if rnd:
                lo, hi, _ = L.digits_random(y, int(dig[c, 0, i]), int(dig[c, 1, i]), nd[c][0][i], nd[c][1][i])
            else:
                lo, hi, _ = L.digits(y, int(dig[c, 0, i]), int(dig[c, 1, i]))
            assert (lo, hi) == (int(want[c, 0, i]), int(want[c, 1, i])), (c, i)
