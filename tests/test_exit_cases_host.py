"""The chosen accumulators of the chunk entry and exit (tests/exit_cases.py) on the CPU, before any GPU test relies on
them: the case reference applied to the accumulators of a real oracle bootstrap gives the oracle's own raw and reduced
rows; the entry reference gives the oracle's accumulators and its flatten at zero iterations in both modes; every
built input is a pair a flatten stores; the tie residues have the remainders claimed and every ModRed boundary sits
where it is said to; and the LUT rows meet every fold they were built for."""

import math

import numpy as np
import pytest

import bigint_oracle as BO
import exit_cases as EC
import kloop_cases as KC
import lut_ref as LR
import ring_cases as RC

SEED = RC.KEY32
ORACLE_RINGS = ("m128", "limb64", "wide")


def _all_params():
    import sgfhe_jl_amd as S
    return [(name, RC.ring(S, name).params) for name in RC.NAMES] + [("p1024", S.Params(1024))]


def _ints(arr):
    return [int(lo) | (int(hi) << 64) for lo, hi in np.ascontiguousarray(arr).reshape(-1, 2)]


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", ORACLE_RINGS)
def test_exit_reference_equals_the_oracle_on_real_accumulators(S, oc, name, rnd):
    """Three rows through the C oracle with want_acc: expected_classic of the accumulators == the oracle's raw rows and
    its reduced rows; and the accumulators survive digits -> acc_of."""
    rg = RC.ring(S, name)
    p = rg.params
    o, _ = RC.oracles(oc, rg)
    sk = o.private_key(61)
    bkey = o.bootstrap_key(sk, 62, noise=rg.noise)
    a, b = o.lwe_encrypt_bits(sk, np.array([0, 1, 1, 0, 1, 1], dtype=np.uint8), 63)
    kw = dict(rnd=(SEED, 4)) if rnd else {}
    raw, acc = o.bootstrap_batch(bkey, a[0::2], b[0::2], a[1::2], b[1::2], raw=True, want_acc=True, **kw)
    red = o.bootstrap_batch(bkey, a[0::2], b[0::2], a[1::2], b[1::2], **kw)
    rows = [(_ints(acc[t, 0]), _ints(acc[t, 1])) for t in range(3)]
    assert np.array_equal(EC.expected_classic(p, rows, raw=True), raw)
    assert np.array_equal(EC.expected_classic(p, rows), red)
    assert np.array_equal(EC.acc_words(rows), acc)
    R = KC.RingView(p, rnd)
    for draws in EC.DRAWS:
        assert EC.acc_of(R, EC.digits(R, rows[0], draws)) == rows[0]


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", ORACLE_RINGS)
def test_entry_reference_equals_the_oracle_at_zero_iterations(S, oc, name, rnd):
    """Classic rows on the standard oracle and LUT rows on the low-amplitude one, n_iters = 0: entry_acc == the oracle's
    accumulators, and the digits of expected_entry == the oracle's own flatten of them (flatten_random with the draws of
    its restatement of the stream for tag 0, bootstrap t, the call number)."""
    rg = RC.ring(S, name)
    p = rg.params
    o, lo = RC.oracles(oc, rg)
    R = KC.RingView(p, rnd)
    a1, b1, a2, b2, lut = EC.entry_rows(p, 5, lut_every=2)
    b1[3], b2[3] = p.Dr, 0                                    # u.b = Dr: the zero coefficient lands on index 0
    key = np.zeros((p.n, 4, 2, p.m, 2), dtype=np.uint64)      # (no iteration reads it)
    call = 3
    dig, ua = EC.expected_entry(p, SEED if rnd else None, call, a1, b1, a2, b2, lut)
    assert np.array_equal(ua, ((a1 + a2) % np.uint64(p.r)).astype(np.uint32))
    for t in range(5):
        low = bool(lut[t] & EC.LUT_ROW)
        _, acc = (lo if low else o).bootstrap_batch(key, a1[t], b1[t:t + 1], a2[t], b2[t:t + 1], n_iters=0, want_acc=True)
        mine = EC.entry_acc(p, b1[t], b2[t], low)
        assert [_ints(acc[0, 0]), _ints(acc[0, 1])] == [mine[0], mine[1]], (name, t)
        for c in range(2):
            d = o.flatten_draws(SEED, c, 0, boot=t, call=call) if rnd else None
            for i in (0, 1, p.m // 2, p.m - 1, (7 * t + 3) % p.m):
                u = o.flatten_random(mine[c][i], int(d[i, 0]), int(d[i, 1])) if rnd else o.flatten(mine[c][i])
                want = [(v if v <= p.Q // 2 else v - p.Q) + R.shift for v in u]
                assert [int(dig[t, c, 0, i]), int(dig[t, c, 1, i])] == want, (name, t, c, i)
        assert EC.acc_of(R, dig[t]) == mine


def test_entry_rows_cover_every_rotation():
    for name, p in _all_params()[:5]:
        a1, b1, a2, b2, lut = EC.entry_rows(p, p.r + 3, lut_every=3)
        ub = (b1 + b2) % np.uint64(p.r)
        assert set(ub.tolist()) == set(range(p.r))
        assert all(int(x) + int(y) >= p.r for x, y, u in zip(b1, b2, ub) if u != p.r - 1)
        assert int(a1.max()) < p.r and int(a2.max()) < p.r and ((a1 + a2) >= np.uint64(p.r)).mean() > 0.25
        assert (p.r + 3) % 8 and 0 < np.count_nonzero(lut) < len(lut)


@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_every_built_input_is_storable(rnd):
    """Classic and LUT rows of every ring and of Params(1024) with every draw pattern, and the largest pair where the
    mode admits it: all pass the entry's rule (kloop_cases.storable)."""
    for name, p in _all_params():
        R = KC.RingView(p, rnd)
        rows = EC.classic_rows(p, *EC.classic_pairs(p)) + EC.lut_rows(p)
        if name == "p1024":
            rows = rows[:2] + rows[-2:]
        for draws in EC.DRAWS if rnd else EC.DRAWS[:1]:
            dig = EC.digits_of(R, rows, draws)
            lo, hi = dig[:, :, 0].reshape(-1).tolist(), dig[:, :, 1].reshape(-1).tolist()
            assert all(KC.storable(R, a, b) for a, b in zip(lo, hi)), (name, draws)
        if rnd:
            dig, row = EC.largest_pair(R)
            assert EC.acc_of(R, dig) == row and not KC.storable(R, R.B + R.draw_max, R.hi_max + R.draw_max)


def test_modred_boundaries_and_the_tie():
    """gcd(r, Q) = 1; x_tie has remainder exactly roundthr and is the first of its pair to round up, the residue below it
    has remainder roundthr - 1; every boundary pair straddles its k; where r <= 256 all 2 r residues are there."""
    for name, p in _all_params():
        assert math.gcd(p.r, p.Q) == 1 and p.Q & 1
        thr = EC.roundthr(p)
        x_tie, x_below = EC.tie(p)
        assert x_tie * p.r % p.Q == thr and x_below * p.r % p.Q == thr - 1
        assert LR.modred(x_tie, p) == (x_tie * p.r // p.Q + 1) % p.r and LR.modred(x_below, p) == x_below * p.r // p.Q
        ks = EC.threshold_ks(p)
        assert len(ks) == (p.r if p.r <= 256 else 7)
        for k in ks:
            lo, hi = EC.boundary(p, k)
            assert 0 <= lo < hi < p.Q
            assert BO.reduce_modulus(p.r, lo, p.Q) == k and BO.reduce_modulus(p.r, hi, p.Q) == (k + 1) % p.r
            assert LR.modred(lo, p) == k and LR.modred(hi, p) == (k + 1) % p.r


def test_classic_rows_hold_their_pairs():
    """Every pair is read back by the reference at its slot: va as the AND word, vo as the OR word; w = 0, vo = va,
    vo = va - 1, the b-word folds and (deterministic) the stored values x + offneg = Q - 1, Q, Q + 1 all occur."""
    for name, p in _all_params():
        Q, n, m, DQ = p.Q, p.n, p.m, p.DQ_tilde % p.Q
        pairs, bpairs = EC.classic_pairs(p)
        rows = EC.classic_rows(p, pairs, bpairs)
        assert len(rows) <= (5 if name == "p1024" else 40)
        raw = [EC.classic_raw(p, row) for row in rows]
        got = [(raw[t][0][e], raw[t][1][e]) for t in range(len(rows)) for e in range(n)]
        assert got[:len(pairs)] == pairs
        assert [(raw[t][0][n], raw[t][1][n]) for t in range(len(bpairs))] == bpairs
        assert all(raw[t][2][e] == (raw[t][1][e] - raw[t][0][e]) % Q for t in range(len(rows)) for e in range(n + 1))
        assert {(0, 0), (1, 0), (0, Q - 1)} <= set(pairs)                       # w = 0; vo = va; vo = va - 1 at the wrap
        assert {rows[t][1][3 * m // 4] for t in range(5)} == {Q - DQ - 1, Q - DQ, Q - DQ + 1, 0, Q - 1}
        assert {rows[t][1][m // 4] for t in range(5)} == {DQ - 1, DQ, DQ + 1, 0, Q - 1}
        R = KC.RingView(p, False)
        offneg = (Q - EC.offset(R)) % Q
        read = {rows[t][0][3 * m // 4 - e] for t in range(len(rows)) for e in range(n)}
        assert {Q - 1, Q, Q + 1} <= {(v + EC.offset(R)) % Q + offneg for v in read}


def test_lut_rows_meet_their_folds():
    """lut_trace == lut_ref.rows_from_acc on every LUT row and table of the family, and over the 256 tables (16 at
    Params(1024)) the rows meet: a zero read from the negated half, v == Q at the last and at an earlier add, DQL + P =
    Q - 1, Q, Q + 1 on the b word, the base words (Q -+ 1)/2 and the two quarter-way values, and a fold of 4 v alone."""
    for name, p in _all_params():
        big = name == "p1024"
        rows = EC.lut_rows(p, ("targets", "sums DQL") if big else EC.LUT_KINDS)
        tables = EC.TABLES16 if big else range(256)
        events = set()
        for t, row in enumerate(rows):
            want = EC.expected_family(p, [row], [list(tables)], raw=True)[0] if not big else None
            for i, tab in enumerate(tables):
                words, ev = EC.lut_trace(p, row, tab)
                events |= ev
                if not big:
                    got = [[int(lo) | (int(hi) << 64) for lo, hi in want[i, k]] for k in range(3)]
                    assert got == words, (name, t, tab)
        need = {"zero from the negated half", ("v == Q", "last add"), ("v == Q", "earlier add"), ("b pre-fold", -1),
                ("b pre-fold", 0), ("b pre-fold", 1), ("base", "(Q - 1)/2"), ("base", "(Q + 1)/2"),
                ("base", "first v4 fold"), ("base", "last without v4 fold"), "v4 only"}
        if big:
            need.discard("zero from the negated half")       # (the all-zero row is left to the small rings)
        assert need <= events, (name, sorted(map(str, need - events)))
        assert all(LR.transitions(tab) == [j] and LR.kappas(tab) == [1] for j, tab in EC.SINGLE.items())
