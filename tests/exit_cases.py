"""TEST INFRASTRUCTURE: chosen accumulators for the kernels either side of the k-loop and their big-integer reference,
once (tests/test_exit_cases_host.py, tests/test_gpu_entry_exit.py; the entries are sgfhe_debug_chunk_entry and
sgfhe_debug_chunk_exit).

A row of an exit case is an accumulator pair (acc_a, acc_b): two lists of m Python integers in [0, Q).  `digits` turns
it into the stored form [2][2][m] through kloop_cases.store -- the draws r0, r1 of the flatten that stored it (0 in the
deterministic mode) and the value x = acc + offset - r0 - r1 B mod Q that flatten reduced -- so every pair is one a
flatten of the mode can have stored.  The one pair
written as digits is `largest_pair` (B - 1 + 2 xmax, hi_max + 2 xmax), the largest the entry's rule admits: no x < Q
has it, it is there for the size of mod_wide's argument in acc_from_digits.

Classic rows.  The exit reads acc_a[3m/4 - e] (the AND word va) and acc_a[m/4 - e] (w, the OR word is vo = -w) for
e < n, and acc_b[3m/4], acc_b[m/4] (va = DQ + ., vo = DQ - .); XOR is vo - va.  `classic_rows` places a list of
(va, vo) pairs into those slots, n + 1 to a row, and fills every other coefficient with pseudo-random residues.
The pairs (`classic_pairs`):
  thresholds   for k in `ks` the two residues either side of the ModRed boundary between k and k + 1 (`boundary`), each
               once as va and once as vo; every k in [0, r) where r is 128 or 256
  specials     x_tie = roundthr r^-1 mod Q (remainder exactly roundthr: the first that rounds up), (roundthr - 1) r^-1
               (one below), 0, 1, Q - 1: every ordered pair of them, so each is va, vo = -w (w = 0 among them) and, as
               differences, vo - va; then each as the difference vo - va of a pseudo-random va
  folds        vo = va, vo = va - 1, vo = va + 1
  b words      acc_b[3m/4] in {Q - DQ - 1, Q - DQ, Q - DQ + 1, 0, Q - 1} with acc_b[m/4] in {DQ - 1, DQ, DQ + 1, 0, Q - 1}
In the deterministic mode the accumulators Q - 1, 0, 1 are the stored values with x + offneg = Q - 1, Q, Q + 1 (the
single conditional subtraction of acc_from_digits); in the randomised mode the same rows are stored with the draws of
DRAWS, and the result must not depend on them.

LUT rows.  c(j) - e for j in 1..8, e in [0, n) visits every coefficient of the polynomial once (c(j - 1) = c(j) + n),
so `lut_row` sets P(acc_a, c(j) - e) and P(acc_b, c(j)) freely:
  "zero"       every coefficient 0: the negated half reads 0 (the branch neg && w of lut_coeff)
  "targets"    the values of `lut_targets` dealt round: a table with its single transition at j (SINGLE[j]: kappa = +1)
               has the coefficient itself as base word -- (Q - 1)/2, (Q + 1)/2, the quarter-way values either side of
               the fold of 4 v, the tie residues, 0, 1, Q - 1 -- and on the b word DQL + P = Q - 1, Q, Q + 1 before the fold
  "sums c"     +-c and +-2c pseudo-randomly: the partial sums of a table's +-1 combination return to 0 through exactly Q
               before the fold (two equal coefficients of opposite kappa), also at the last add; c = 3 and c = DQL, where
               on the b word DQL plus the combination is Q
  "mid"        pseudo-random residues
`lut_trace` restates the folds of lut_base / lut_store_rows to say which of these a (row, table) meets; the host test
holds it to lut_ref.rows_from_acc and asserts that every listed event occurs.

The reference is Python integers only: classic rows by the lines of bigint_oracle.bootstrap_internal after its loop
and reduce_modulus, LUT rows by lut_ref.rows_from_acc, the entry by initial_poly, mul_by_monomial(t, -u.b), the
amplitude and flatten_poly with the draws of ChaChaFlatten for tag 0.
"""

import math

import numpy as np

import bigint_oracle as BO
import kloop_cases as KC
import lut_ref as LR

LUT_ROW = 0x100
DRAWS = ("zero", "max", "crossed")
# the table whose one transition is at j, with kappa = +1: sigma = -1 below j, +1 from j on
SINGLE = {j: (0xFF << j) & 0xFF for j in range(1, 9)}
TABLES16 = (0x00, 0xFF, 0x80, 0x7F, 0xF0, 0x0F, 0xFE, 0x01, 0xFC, 0xF8, 0x96, 0xE8, 0xCA, 0x69, 0xAA, 0xB2)


def offset(R):
    return (1 + R.B) * R.shift % R.Q


def roundthr(p):
    return p.Q // 2 + (p.Q & 1)


def _draws(R, name):
    dm = R.draw_max
    if name == "zero" or not R.rnd:
        return 0, 0
    if name == "max":
        return dm, dm
    return [dm if i & 1 else 0 for i in range(R.m)], [0 if i & 1 else dm for i in range(R.m)]


def digits(R, row, draws="zero"):
    """[2][2][m] stored digits of one row (acc_a, acc_b)."""
    off = offset(R)
    r0, r1 = _draws(R, draws)
    l0 = [r0] * R.m if isinstance(r0, int) else r0
    l1 = [r1] * R.m if isinstance(r1, int) else r1
    # the flatten reduced x = acc + offset - r0 - r1 B and stored (x mod B + r0, x div B + r1)
    return np.stack([KC.store(R, [(v + off - a - b * R.B) % R.Q for v, a, b in zip(poly, l0, l1)], r0, r1) for poly in row])


def digits_of(R, rows, draws="zero"):
    return np.stack([digits(R, row, draws) for row in rows])


def largest_pair(R):
    """([2][2][m] digits, the row they store): every coefficient the pair (B - 1 + draw_max, hi_max + draw_max)."""
    lo, hi = R.B - 1 + R.draw_max, R.hi_max + R.draw_max
    assert KC.storable(R, lo, hi) == R.rnd            # (deterministic: the value is Q or more, the entry refuses it)
    dig = np.zeros((2, 2, R.m), dtype=np.uint64)
    dig[:, 0, :], dig[:, 1, :] = lo, hi
    acc = (lo + hi * R.B - offset(R)) % R.Q
    return dig, ([acc] * R.m, [acc] * R.m)


def acc_of(R, dig):
    """The row (acc_a, acc_b) that [2][2][m] stored digits hold."""
    off = offset(R)
    return tuple([(int(lo) + int(hi) * R.B - off) % R.Q for lo, hi in zip(dig[c, 0], dig[c, 1])] for c in range(2))


def acc_words(rows):
    """[rows][2][m][2] uint64 {lo, hi} residues: the layout of sgfhe_debug_accumulators."""
    out = np.zeros((len(rows), 2, len(rows[0][0]), 2), dtype=np.uint64)
    for t, row in enumerate(rows):
        for c in range(2):
            out[t, c, :, 0] = [v & 0xFFFFFFFFFFFFFFFF for v in row[c]]
            out[t, c, :, 1] = [v >> 64 for v in row[c]]
    return out


def _words(vals, raw):
    """[...] nested lists of ints -> uint64 array, a last axis {lo, hi} with raw."""
    a = np.array(vals, dtype=object)
    if not raw:
        return a.astype(np.uint64)
    return np.stack([(a & 0xFFFFFFFFFFFFFFFF).astype(np.uint64), (a >> 64).astype(np.uint64)], axis=-1)


# ---- ModRed ---------------------------------------------------------------------------------------------------------------

def boundary(p, k):
    """(x, x + 1): the last residue ModRed sends to k and the first it sends to k + 1 (mod r)."""
    hi = -(-(k * p.Q + roundthr(p)) // p.r)
    return hi - 1, hi


def tie(p):
    """(x_tie, x_below): x r mod Q is exactly roundthr, and roundthr - 1."""
    assert math.gcd(p.r, p.Q) == 1
    rinv = pow(p.r, -1, p.Q)
    return roundthr(p) * rinv % p.Q, (roundthr(p) - 1) * rinv % p.Q


def threshold_ks(p):
    if p.r <= 256:
        return list(range(p.r))
    return [0, 1, p.Dr - 1, p.Dr, p.r // 2, p.r - 2, p.r - 1]


# ---- classic rows -----------------------------------------------------------------------------------------------------

def specials(p):
    return list(tie(p)) + [0, 1, p.Q - 1]


def classic_pairs(p, seed=0x65786974):
    """(pairs for the a words, pairs for the b word), each (va, vo)."""
    Q, DQ = p.Q, p.DQ_tilde % p.Q
    g = KC._lcg(seed + p.m)
    X = [x for k in threshold_ks(p) for x in boundary(p, k)]
    pairs = [(X[i], X[(i + len(X) // 2) % len(X)]) for i in range(len(X))]
    S = specials(p)
    pairs += [(s1, s2) for s1 in S for s2 in S]
    for s in S:
        v = KC._uniform(g, Q)
        pairs.append((v, (v + s) % Q))
    v = KC._uniform(g, Q - 2) + 1
    pairs += [(v, v), (v, v - 1), (v, v + 1)]
    b3 = [Q - DQ - 1, Q - DQ, Q - DQ + 1, 0, Q - 1]          # acc_b[3m/4]
    b1 = [DQ - 1, DQ, DQ + 1, 0, Q - 1]                      # acc_b[m/4]
    bpairs = [((DQ + x) % Q, (DQ - y) % Q) for x, y in zip(b3, b1)]
    if p.r <= 256:
        bpairs += [((DQ + x) % Q, (DQ - b1[(i + 2) % 5]) % Q) for i, x in enumerate(b3)]
    return pairs, bpairs


def classic_rows(p, pairs, bpairs, seed=0x726F7773):
    """The rows that hold `pairs` in their a slots (n to a row) and `bpairs` in their b slot (then, where rows are left,
    the a pairs again from the front); every other coefficient pseudo-random."""
    n, m, Q, DQ = p.n, p.m, p.Q, p.DQ_tilde % p.Q
    g = KC._lcg(seed + m)
    count = max(-(-len(pairs) // n), len(bpairs))
    rows = []
    for t in range(count):
        a = [KC._uniform(g, Q) for _ in range(m)]
        b = [KC._uniform(g, Q) for _ in range(m)]
        for e, (va, vo) in enumerate(pairs[t * n:(t + 1) * n]):
            a[3 * m // 4 - e], a[m // 4 - e] = va, (Q - vo) % Q
        va, vo = bpairs[t] if t < len(bpairs) else pairs[(7 * t) % len(pairs)]
        b[3 * m // 4], b[m // 4] = (va - DQ) % Q, (DQ - vo) % Q
        rows.append((a, b))
    return rows


def classic_raw(p, row):
    """[3][n + 1] integers mod Q: bootstrap_internal's lines after its loop (fhe.jl:585-592)."""
    a, b = row
    m, n, Q = p.m, p.n, p.Q
    and_a = BO.extract(a, 3 * m // 4 + 1, n, Q)
    and_b = (p.DQ_tilde + b[3 * m // 4]) % Q
    or_a = [(Q - x) % Q for x in BO.extract(a, m // 4 + 1, n, Q)]
    or_b = (p.DQ_tilde - b[m // 4]) % Q
    xor_a = [(x - y) % Q for x, y in zip(or_a, and_a)]
    return [and_a + [and_b], or_a + [or_b], xor_a + [(or_b - and_b) % Q]]


def _reduce(p, words):
    return [[BO.reduce_modulus(p.r, x, p.Q) for x in w] for w in words]


def expected_classic(p, rows, raw=False, rns2=None):
    """[rows][3][n + 1] uint64 over Z_r; raw: [..][2] residues mod Q; rns2 = (m1, m2): their RNS2Number limb pairs."""
    vals = [classic_raw(p, row) for row in rows]
    if rns2:
        return np.array([[[BO.rns2_from_int(x, *rns2) for x in w] for w in r3] for r3 in vals], dtype=np.uint64)
    return _words(vals if raw else [_reduce(p, r3) for r3 in vals], raw)


# ---- LUT rows -----------------------------------------------------------------------------------------------------------

def lut_targets(p):
    Q = p.Q
    q4 = (Q + 3) // 4                                        # the first v with 4 v >= Q (2 v < Q)
    return [(Q - 1) // 2, (Q + 1) // 2, q4, q4 - 1, (Q + 1) // 2 + q4 // 2] + specials(p)


def lut_btargets(p):
    """P(acc_b, c(j)) for j = 1..8: DQL + P is Q - 1, Q, Q + 1 before the fold, then base words b."""
    Q, A0 = p.Q, p.DQ_tilde >> 2
    q4 = (Q + 3) // 4
    return [Q - 1 - A0, Q - A0, Q + 1 - A0] + [(v - A0) % Q for v in ((Q - 1) // 2, (Q + 1) // 2, q4, q4 - 1, tie(p)[0])]


def lut_row(p, kind, seed=0x6C7574):
    """One row from the values P(acc_a, c(j) - e) and P(acc_b, c(j)) of its kind (module docstring)."""
    n, m, Q = p.n, p.m, p.Q
    g = KC._lcg(seed + m + sum(kind.encode()))
    if kind == "zero":
        return [0] * m, [0] * m
    if kind == "mid":
        return [KC._uniform(g, Q) for _ in range(m)], [KC._uniform(g, Q) for _ in range(m)]
    if kind == "targets":
        T, TB = lut_targets(p), lut_btargets(p)
        pa = lambda j, e: T[(j + 3 * e) % len(T)]
        pb = lambda j: TB[j - 1]
    else:
        c = {"sums 3": 3, "sums DQL": p.DQ_tilde >> 2}[kind]
        pick = lambda: ((1 + (next(g) >> 40 & 1)) * c * (1 if next(g) >> 41 & 1 else -1)) % Q
        va = {(j, e): pick() for j in range(1, 9) for e in range(n)}
        vb = {j: pick() for j in range(1, 9)}
        pa = lambda j, e: va[(j, e)]
        pb = lambda j: vb[j]
    a = [None] * m
    b = [KC._uniform(g, Q) for _ in range(m)]
    for j in range(1, 9):
        for e in range(n):
            idx = (LR.coefficient(p, j) - e) % (2 * m)
            a[idx % m] = pa(j, e) if idx < m else (Q - pa(j, e)) % Q
        idx = LR.coefficient(p, j)
        b[idx % m] = pb(j) if idx < m else (Q - pb(j)) % Q
    assert None not in a
    return a, b


LUT_KINDS = ("zero", "targets", "sums 3", "sums DQL", "mid")


def lut_rows(p, kinds=LUT_KINDS):
    return [lut_row(p, k) for k in kinds]


def expected_lut(p, rows, tables, raw=False):
    """[rows][3][n + 1] (raw: [..][2]) of single-table LUT rows: lut_ref.rows_from_acc."""
    return LR.rows_from_acc(p, acc_words(rows), [int(t) for t in tables], raw=raw)


def expected_family(p, rows, tables, raw=False):
    """tables [rows][T] -> [rows][T][3][n + 1] (raw: [..][2])."""
    tables = np.asarray(tables)
    acc = acc_words(rows)
    return np.stack([LR.rows_from_acc(p, acc, [int(t) for t in tables[:, j]], raw=raw) for j in range(tables.shape[1])], axis=1)


def expected_mixed(p, rows, words, raw=False):
    """A per-row descriptor: 0 a classic row, LUT_ROW | table a LUT row."""
    out = expected_classic(p, rows, raw=raw)
    for t, w in enumerate(words):
        if int(w) & LUT_ROW:
            out[t] = expected_lut(p, [rows[t]], [int(w) & 0xFF], raw=raw)[0]
    return out


def lut_trace(p, row, table):
    """The folds of lut_base and lut_store_rows restated: (words [3][n + 1] mod Q, events) with events the set of
    ("zero from the negated half"), ("v == Q", last add or not), ("b pre-fold", Q - 1 | Q | Q + 1), ("base", name),
    ("v4 only") met on the way."""
    n, m, Q, A0 = p.n, p.m, p.Q, p.DQ_tilde >> 2
    js, ks = LR.transitions(table), LR.kappas(table)
    T = lut_targets(p)
    names = {T[0]: "(Q - 1)/2", T[1]: "(Q + 1)/2", T[2]: "first v4 fold", T[3]: "last without v4 fold"}
    events = set()
    base = []
    for e in range(n + 1):
        poly, shift = (row[0], e) if e < n else (row[1], 0)
        v = A0 if e == n else 0
        for i, (j, k) in enumerate(zip(js, ks)):
            idx = (LR.coefficient(p, j) - shift) % (2 * m)
            w = poly[idx % m]
            if idx >= m:
                if w == 0:
                    events.add("zero from the negated half")
                w = (Q - w) % Q
            if k < 0:
                w = (Q - w) % Q
            v += w
            if v == Q:
                events.add(("v == Q", "last add" if i == len(js) - 1 else "earlier add"))
            if e == n and len(js) == 1 and Q - 1 <= v <= Q + 1:
                events.add(("b pre-fold", v - Q))
            if v >= Q:
                v -= Q
        if v in names:
            events.add(("base", names[v]))
        if 2 * v < Q <= 4 * v:
            events.add("v4 only")
        base.append(v)
    return [[(4 * v) % Q for v in base], [(2 * v) % Q for v in base], base], events


# ---- the entry ---------------------------------------------------------------------------------------------------------

def entry_rows(p, count, seed=0x656E7472, lut_every=0):
    """`count` rows (a1, b1, a2, b2, lut words): row t has u.b = t mod r, reached through a sum b1 + b2 that wraps past r
    (b1 = r - 1; u.b = r - 1 alone cannot wrap with both words below r); a1 + a2 wraps on about half the words;
    every lut_every-th row a LUT row."""
    n, r = p.n, p.r
    g = KC._lcg(seed + r)
    a1 = np.array([[next(g) % r for _ in range(n)] for _ in range(count)], dtype=np.uint64)
    a2 = np.array([[next(g) % r for _ in range(n)] for _ in range(count)], dtype=np.uint64)
    b1 = np.full(count, r - 1, dtype=np.uint64)
    b2 = np.array([(t + 1) % r for t in range(count)], dtype=np.uint64)
    lut = np.array([(LUT_ROW | (0x96 + t) & 0xFF) if lut_every and t % lut_every == lut_every - 1 else 0 for t in range(count)],
                   dtype=np.uint32)
    return a1, b1, a2, b2, lut


def entry_acc(p, b1, b2, low):
    """(a, b) before the first iteration: a = 0, b = x^(-u.b) t amplitude (fhe.jl:566-573)."""
    ub = (int(b1) + int(b2)) % p.r
    amp = p.DQ_tilde >> 2 if low else p.DQ_tilde
    return [0] * p.m, [(c * amp) % p.Q for c in BO.mul_by_monomial(BO.initial_poly(p), -ub, p.Q)]


def stored_flatten(R, acc, draws=None):
    """[2][m] stored digits of flatten_poly(acc) (src/utils.jl:155-264): signed digit + shift."""
    u = BO.flatten_poly(acc, R.B, 2, R.Q, draws)
    return np.array([[(v if v <= R.Q // 2 else v - R.Q) + R.shift for v in u[d]] for d in range(2)], dtype=np.uint64)


def expected_entry(p, rnd_key, call, a1, b1, a2, b2, lut=None, boot0=0):
    """(digits [rows][2][2][m], u.a [rows][n]) as k_init leaves them: row t draws (tag 0) as bootstrap boot0 + t of call
    `call`.  rnd_key None: the deterministic mode."""
    R = KC.RingView(p, rnd_key is not None)
    rows = len(b1)
    ua = ((np.asarray(a1, dtype=np.uint64) + np.asarray(a2, dtype=np.uint64)) % np.uint64(p.r)).astype(np.uint32)
    dig = np.zeros((rows, 2, 2, p.m), dtype=np.uint64)
    cache = {}
    for t in range(rows):
        low = bool(lut is not None and int(lut[t]) & LUT_ROW)
        key = ((int(b1[t]) + int(b2[t])) % p.r, low)
        if R.rnd:
            rng = BO.ChaChaFlatten(p, rnd_key, boot0 + t, call)
            acc = entry_acc(p, b1[t], b2[t], low)
            dig[t] = np.stack([stored_flatten(R, acc[c], rng.draws(c, 0)) for c in range(2)])
            continue
        if key not in cache:
            acc = entry_acc(p, b1[t], b2[t], low)
            cache[key] = np.stack([stored_flatten(R, acc[c]) for c in range(2)])
        dig[t] = cache[key]
    return dig, ua
