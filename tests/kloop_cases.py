"""TEST INFRASTRUCTURE: chosen operands of one k-loop step and their big-integer reference, once
(tests/test_kloop_cases_host.py, tests/test_gpu_kloop_step.py; the entry is sgfhe_debug_kloop_step).

A gate of a case is (digits [2][2][m], j): the stored digit planes of the accumulator pair (a, b) and the rotation
amount u.a[k].  No builder writes a raw digit: every coefficient is a value x in [0, Q) -- what the flatten before
this step reduced, accumulator + offset -- and, in the randomised mode, that flatten's draws r0, r1 in [0, 2 xmax];
the stored pair is (x mod B + r0, x div B + r1), so every pair is one a flatten of the mode can have stored
(`storable`, the rule the entry refuses by).

Families (FAMILIES; `family(R, name)`):
  extreme digits, by sign pattern   x = TOP (digits (B - 1, hi_max - 1): both signed digits at +B/2 where B^2 ~ Q) or
                                    BOT (x = 0: both at -B/2), pack_direct_ref.extreme_residue(p, +-1) plus the offset;
                                    all +, all -, + on a and - on b, alternating by coefficient, + on the first half
                                    of every polynomial and - on the second (the first radix-4 head).  Randomised:
                                    draws 2 xmax with TOP and 0 with BOT (the largest stored values, which fill the
                                    third plane of a MODE_WIDE record, and stored zeros), and the crossed choice
  "q-1"                             x = Q - 1: the largest high digit (plus 2 xmax randomised)
  "mid"                             fixed pseudo-random x and draws (a gate unlike the structured ones)
Key slices (SLICES; `key_slice(p, name)`): residues (Q - 1) / 2 and (Q + 1) / 2 (centred +-(Q - 1) / 2) in the
patterns of tests/test_gpu_worstcase.py, the all-zero slice (the step is then the CRT stage's identity), "rows", whose
eight polynomials all differ (the others repeat one polynomial down the rows, which a wrong row index survives), and "b to a"
/ "a to b", where only rows 2, 3 x column 0 (rows 0, 1 x column 1) are non-zero: D of that column does not depend on
the column's own digits, which `wrap_gate` then chooses so that the NEW value lands on 0, Q - 1, B - 1 and B.
Rotations: `rotations(m)`.  Gate mixing: `mixed(R, count, ...)` deals families and rotations round so that
neighbouring gates, and the first and the last, differ.

`expected(...)` is Python integers only (bigint_oracle's negacyclic product and monomial rule, its restatement of the
ChaCha8 draw stream); test_kloop_cases_host.py holds it to the numpy model of the kernels and to the oracle's own
flatten before any GPU test relies on it.
"""

import numpy as np

import bigint_oracle as BO
from pack_direct_ref import extreme_residue

FAMILIES = ("all +", "all -", "+ a, - b", "alternating", "halves", "crossed draws", "q-1", "mid")
SLICES = ("all +", "+ col 0, - col 1", "alternating", "zero", "rows")


class RingView:
    """What the cases read of a parameter set (n, m, Q, B) in one flatten mode."""

    def __init__(self, p, rnd):
        self.p, self.rnd = p, bool(rnd)
        self.n, self.m, self.Q, self.B = p.n, p.m, p.Q, p.B
        self.logm = p.m.bit_length() - 1
        self.s = (p.B - 1) // 2 if p.B % 2 else p.B // 2 - 1
        self.xmax = BO.flatten_xmax(p.B)
        assert self.xmax == 3 * (p.B // 2)
        self.draw_max = 2 * self.xmax if rnd else 0
        self.shift = self.s + (self.xmax if rnd else 0)        # stored digit e = signed digit u + shift
        self.hi_max = (p.Q - 1) // p.B
        off = (1 + p.B) * self.s % p.Q
        self.top = (extreme_residue(p, +1) + off) % p.Q
        self.bot = (extreme_residue(p, -1) + off) % p.Q
        assert self.top == (self.hi_max - 1) * p.B + p.B - 1 and self.bot == 0


def storable(R, e_lo, e_hi):
    """The entry's validity rule: a pair some flatten of the mode stores."""
    if not (0 <= e_lo <= R.B - 1 + R.draw_max and 0 <= e_hi <= R.hi_max + R.draw_max):
        return False
    return R.rnd or e_lo + e_hi * R.B < R.Q


def store(R, xs, r0=0, r1=0):
    """[2][m] stored digits of the values xs (one polynomial) with draws r0, r1: scalars or per-coefficient lists."""
    m = R.m
    r0 = [r0] * m if isinstance(r0, int) else r0
    r1 = [r1] * m if isinstance(r1, int) else r1
    assert all(0 <= x < R.Q for x in xs) and all(0 <= r <= R.draw_max for r in list(r0) + list(r1))
    return np.array([[x % R.B + a for x, a in zip(xs, r0)], [x // R.B + b for x, b in zip(xs, r1)]], dtype=np.uint64)


def _lcg(seed):
    state = seed & ((1 << 64) - 1)
    while True:
        state = (state * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        yield state


def _uniform(gen, bound):
    """An integer in [0, bound) from enough 64-bit words."""
    words = (bound.bit_length() + 63) // 64 + 1
    v = 0
    for _ in range(words):
        v = (v << 64) | next(gen)
    return v % bound


def family(R, name):
    """digits [2][2][m] uint64 of one gate."""
    m, top, bot, dm = R.m, R.top, R.bot, R.draw_max
    pm = lambda plus: (top, dm) if plus else (bot, 0)     # the value and the draw that goes with it
    if name == "crossed draws":                           # TOP with draw 0, BOT with 2 xmax
        sel = [[(top, 0) if i & 1 else (bot, dm) for i in range(m)], [(bot, dm) if i & 1 else (top, 0) for i in range(m)]]
    elif name == "q-1":
        sel = [[(R.Q - 1, dm)] * m, [(R.Q - 1, 0) if i & 1 else (R.Q - 1, dm) for i in range(m)]]
    elif name == "mid":
        g = _lcg(0x6B6C6F6F70 + m)
        sel = [[(_uniform(g, R.Q), None) for _ in range(m)] for _ in range(2)]
        out = []
        for c in range(2):
            r0 = [_uniform(g, dm + 1) for _ in range(m)]
            r1 = [_uniform(g, dm + 1) for _ in range(m)]
            out.append(store(R, [x for x, _ in sel[c]], r0, r1))
        return np.stack(out)
    else:
        plus = {"all +": lambda c, i: True, "all -": lambda c, i: False, "+ a, - b": lambda c, i: c == 0,
                "alternating": lambda c, i: bool((i + c) & 1), "halves": lambda c, i: i < m // 2}[name]
        sel = [[pm(plus(c, i)) for i in range(m)] for c in range(2)]
    return np.stack([store(R, [x for x, _ in sel[c]], [r for _, r in sel[c]], [r for _, r in sel[c]]) for c in range(2)])


def key_slice(p, name):
    """C[row][col] lists of m canonical residues."""
    m, Q = p.m, p.Q
    kpos, kneg = (Q - 1) // 2, (Q + 1) // 2
    zero = [0] * m
    if name == "all +":
        return [[[kpos] * m, [kpos] * m] for _ in range(4)]
    if name == "+ col 0, - col 1":
        return [[[kpos] * m, [kneg] * m] for _ in range(4)]
    if name == "alternating":
        return [[[kpos if i & 1 else kneg for i in range(m)], [kneg if i & 1 else kpos for i in range(m)]] for _ in range(4)]
    if name == "zero":
        return [[zero, zero] for _ in range(4)]
    if name == "rows":            # every row and column its own pattern: a kernel that takes the wrong key row shows
        return [[[kpos if (i >> row) & 1 else kneg for i in range(m)], [kneg if (i >> (3 - row)) & 1 or i == row else kpos for i in range(m)]]
                for row in range(4)]
    if name == "b to a":          # column 0 from the digits of b alone
        return [[zero, zero], [zero, zero], [[kpos] * m, zero], [[kneg if i & 1 else kpos for i in range(m)], zero]]
    if name == "a to b":
        return [[zero, [kneg] * m], [zero, [kpos if i & 1 else kneg for i in range(m)]], [zero, zero], [zero, zero]]
    raise KeyError(name)


def slice_words(C):
    """[4][2][m][2] uint64 of a slice, the entry's layout."""
    out = np.zeros((4, 2, len(C[0][0]), 2), dtype=np.uint64)
    for row in range(4):
        for col in range(2):
            out[row, col, :, 0] = [v & 0xFFFFFFFFFFFFFFFF for v in C[row][col]]
            out[row, col, :, 1] = [v >> 64 for v in C[row][col]]
    return out


def rotations(m):
    """The special rotations, and one odd and one even amount mid-range."""
    out = [0, 1, m - 1, m, m + 1, 2 * m - 1, m // 2 + 1, 3 * m // 2 - 2]
    assert out[6] & 1 and not out[7] & 1 and len(set(out)) == 8
    return out


def mixed(R, count, first=0, families=FAMILIES):
    """`count` gates: families and rotations dealt round from position `first`, so that neighbours differ in both and
    (the two lists have different lengths, or one is rotated) the first gate differs from the last.
    Returns (digits [count][2][2][m], j [count])."""
    rot = rotations(R.m)
    fam = {}
    digs, js = [], []
    for g in range(count):
        name = families[(first + g) % len(families)]
        if name not in fam:
            fam[name] = family(R, name)
        digs.append(fam[name])
        js.append(rot[(first + 3 * g) % len(rot)])
    if count > 1 and np.array_equal(digs[0], digs[-1]) and js[0] == js[-1]:
        js[-1] = rot[(rot.index(js[-1]) + 1) % len(rot)]
    return np.stack(digs), np.array(js, dtype=np.uint32)


# ---- the reference ----------------------------------------------------------------------------------------------------

def _pack(poly, slot):
    return int.from_bytes(b"".join(int(c).to_bytes(slot, "little") for c in poly), "little")


class Products:
    """sum_row u_row (*) C[row][col] mod (x^m + 1, Q) for the signed digit rows u of a gate, by Kronecker substitution
    (bigint_oracle.poly_mul's, slots wide enough for the sum of four products).  Rows that meet the same key polynomial
    are added before the one multiplication they need, a polynomial whose negative has been multiplied by the same sum
    takes that product negated, and gates with equal digits share the result: the structured slices cost one big
    multiplication per distinct gate, "rows" eight."""

    def __init__(self, R, C):
        self.R = R
        m, Q = R.m, R.Q
        self.slot = (2 * (Q - 1).bit_length() + m.bit_length() + 2 + 8 + 7) // 8
        self.C = [[_pack(C[row][col], self.slot) for col in range(2)] for row in range(4)]
        self.neg = {self.C[row][col]: _pack([(Q - v) % Q for v in C[row][col]], self.slot) for row in range(4) for col in range(2)}
        self.cache = {}

    def _unpack(self, value):
        m, Q, slot = self.R.m, self.R.Q, self.slot
        prod = value.to_bytes(2 * m * slot + 1, "little")
        return [(int.from_bytes(prod[i * slot:(i + 1) * slot], "little")
                 - int.from_bytes(prod[(i + m) * slot:(i + m + 1) * slot], "little")) % Q for i in range(m)]

    def of(self, dig):
        """dig [2][2][m] stored digits -> [2][m] Python integers."""
        key = dig.tobytes()
        if key not in self.cache:
            R = self.R
            m, Q = R.m, R.Q
            rows = [[(e - R.shift) % Q for e in dig[c, d].tolist()] for c in range(2) for d in range(2)]   # a_lo, a_hi, b_lo, b_hi
            packed = [_pack(u, self.slot) for u in rows]
            done = {}                                       # (sum of rows, key polynomial) -> their product, unpacked
            out = []
            for col in range(2):
                groups = {}
                for row in range(4):
                    groups[self.C[row][col]] = groups.get(self.C[row][col], 0) + packed[row]
                total = [0] * m
                for kp, usum in groups.items():
                    if kp == 0:
                        continue
                    if (usum, kp) not in done:
                        if (usum, self.neg[kp]) in done:
                            done[(usum, kp)] = [(Q - v) % Q for v in done[(usum, self.neg[kp])]]
                        else:
                            done[(usum, kp)] = self._unpack(usum * kp)
                    total = [(a + b) % Q for a, b in zip(total, done[(usum, kp)])]
                out.append(total)
            self.cache[key] = out
        return self.cache[key]


def seed_int(rnd_key):
    return rnd_key if isinstance(rnd_key, int) else int.from_bytes(rnd_key, "little")


def next_draws(R, rnd_key, call, gate, k):
    """r'[c][d][i] in [0, 2 xmax]: the draws of the flatten that ends iteration k (tag k + 1) for bootstrap `gate` of call
    number `call`, from the oracle's restatement of the engine's ChaCha8 stream."""
    rng = BO.ChaChaFlatten(R.p, rnd_key, gate, call)
    out = []
    for c in range(2):
        f = rng.draws(c, k + 1)
        out.append([[f(i, d) + R.xmax for i in range(R.m)] for d in range(2)])
    return out


def step_delta(R, prods, dig, j):
    """D[c] = (x^j - 1) sum_row u_row (*) C[row][c]."""
    return [BO.mul_by_xj_minus_one(col, int(j), R.Q) for col in prods.of(dig)]


def expected(params, rnd_key, call, digits, C, j, k, prods=None):
    """The stored digits [gates][2][2][m] after iteration k.  rnd_key None: the deterministic mode.  With V = sum_i e_i B^i
    the value the digits store (accumulator + offset: acc = sum_i (e_i - s - xmax rnd) B^i) and D as step_delta:
    deterministic (x mod B, x div B) of x = (V + D) mod Q; randomised (x2 mod B + r0', x2 div B + r1') of
    x2 = (V + D - r0' - r1' B) mod Q with the draws r' of next_draws.  `prods`: a Products of the same slice to share."""
    R = RingView(params, rnd_key is not None)
    Q, B = R.Q, R.B
    prods = prods if prods is not None else Products(R, C)
    out = np.zeros(digits.shape, dtype=np.uint64)
    for g in range(digits.shape[0]):
        D = step_delta(R, prods, digits[g], j[g])
        draws = next_draws(R, rnd_key, call, g, k) if R.rnd else [[[0] * R.m] * 2] * 2
        for c in range(2):
            lo, hi = digits[g, c, 0].tolist(), digits[g, c, 1].tolist()
            r0, r1 = draws[c]
            x2 = [(lo[i] + hi[i] * B + D[c][i] - r0[i] - r1[i] * B) % Q for i in range(R.m)]
            out[g, c, 0] = [x % B + r for x, r in zip(x2, r0)]
            out[g, c, 1] = [x // B + r for x, r in zip(x2, r1)]
    return out


def wrap_targets(R):
    return [0, R.Q - 1, R.B - 1, R.B]


def wrap_gate(R, C, col, other, j, rnd_key=None, call=0, gate=0, k=0):
    """A gate whose column `col` (0: a, 1: b) lands on wrap_targets after the step -- coefficient i on target i mod 4:
    the value the flatten takes its digits of is exactly 0, Q - 1, B - 1 or B.  C is a slice whose column `col` reads the
    OTHER polynomial's digits only ("b to a" for col 0, "a to b" for col 1); `other` [2][m] are that polynomial's stored
    digits.  The old draws of the chosen polynomial alternate between 0 and 2 xmax."""
    m, Q, B = R.m, R.Q, R.B
    dig = np.zeros((2, 2, m), dtype=np.uint64)
    dig[1 - col] = other
    D = step_delta(R, Products(R, C), dig, j)[col]        # does not read dig[col]
    nd = next_draws(R, rnd_key, call, gate, k)[col] if R.rnd else [[0] * m, [0] * m]
    tg = wrap_targets(R)
    old = [[R.draw_max if i & 4 else 0 for i in range(m)], [0 if i & 4 else R.draw_max for i in range(m)]]
    # stored value x + old draws; new value stored value + D - new draws
    xs = [(tg[i % 4] + nd[0][i] + nd[1][i] * B - D[i] - old[0][i] - old[1][i] * B) % Q for i in range(m)]
    dig[col] = store(R, xs, old[0], old[1])
    return dig
