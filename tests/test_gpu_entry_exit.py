"""The kernels either side of the k-loop on chosen operands: k_init through sgfhe_debug_chunk_entry, and k_final,
k_final_lut, k_final_lut_multi (the primitive's instantiation), k_canon_to_rns2 and k_dump_acc through
sgfhe_debug_chunk_exit -- the functions every bootstrap call runs before and after its iterations, on caller-chosen
rows and stored digits.  The operands and their big-integer reference are tests/exit_cases.py (held to the oracle on the
CPU by tests/test_exit_cases_host.py): every ModRed boundary and the exact tie, w = 0, vo = va, the b-word folds at
equality and one to either side, the conditional subtraction of acc_from_digits at x = Q, the largest stored pairs of
the randomised mode, LUT rows whose folds meet Q exactly, all 256 tables on them, every rotation u.b, padded chunks and
LUT rows among classic ones.  Every comparison is of equal integer arrays.  The wire-table instantiation of
k_final_lut_multi is left to tests/test_gpu_lut_multi.py, which holds a circuit's wires to the primitive's bytes.
Run with `pytest -m gpu`."""

import numpy as np
import pytest

import bigint_oracle as BO
import exit_cases as EC
import kloop_cases as KC
import ring_cases as RC

pytestmark = pytest.mark.gpu

KEY = RC.KEY32
ERR_INVALID_ARG = -1
RINGS = RC.NAMES + ("p1024",)


class Ctx:
    """One ctx without a key; the case rows and their reference once per ring (they do not depend on the mode)."""

    def __init__(self, S, name):
        self.S, self.name = S, name
        self.rg = RC.ring(S, name) if name in RC.NAMES else None
        self.p = self.rg.params if self.rg else S.Params(1024)
        self.big = self.rg is None
        self.eng = S.Engine(self.p)
        self.rnd, self.call, self.views, self.memo = False, 0, {}, {}

    def mode(self, rnd):
        self.eng.set_random_flatten(bool(rnd), KEY if rnd else 0)     # the call counter starts again
        self.rnd, self.call = bool(rnd), 0
        if rnd not in self.views:
            self.views[rnd] = KC.RingView(self.p, rnd)
        return self.views[rnd]

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def classic(self):
        return self.once("classic", lambda: EC.classic_rows(self.p, *EC.classic_pairs(self.p)))

    def luts(self):
        return self.once("lut", lambda: EC.lut_rows(self.p, ("targets", "sums DQL") if self.big else EC.LUT_KINDS))


@pytest.fixture(scope="module")
def ctxs(S):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ctx(S, name)
        return made[name]
    yield get
    for c in made.values():
        c.eng.close()


def _same(got, want, label):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert got.shape == want.shape and bad.size == 0, "%s: %d words differ, first at %s: got %s, want %s" % (
        label, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the exit: classic rows ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", RINGS)
def test_classic_rows(ctxs, name, rnd):
    """k_final, reduced and raw, on the rows of exit_cases.classic_rows: every ModRed boundary (all 2 r residues where r is
    128 or 256, the seven listed k at Params(1024)), the tie, w = 0, vo = va, the b-word folds.  Randomised: the same
    accumulators under every draw pattern give the same bytes; then every coefficient at the largest stored pair and at
    x = Q - 1.  The accumulator tap (k_dump_acc) returns the values stored.  `composite`: the RNS2 form."""
    c = ctxs(name)
    R = c.mode(rnd)
    rows = c.classic()
    want = c.once("classic ref", lambda: (EC.expected_classic(c.p, rows), EC.expected_classic(c.p, rows, raw=True)))
    for draws in EC.DRAWS if rnd else EC.DRAWS[:1]:
        dig = EC.digits_of(R, rows, draws)
        got, acc = c.eng.debug_chunk_exit(dig, want_acc=True)
        _same(got, want[0], "%s, %s draws, reduced" % (name, draws))
        _same(acc, EC.acc_words(rows), "%s, %s draws, accumulators" % (name, draws))
        _same(c.eng.debug_chunk_exit(dig, raw=True), want[1], "%s, %s draws, raw" % (name, draws))
    if c.rg is not None and c.rg.rns2:
        m1, m2 = c.rg.rns2
        c.eng.rns2_convert(np.zeros((1, 2), dtype=np.uint64), m1, m2, True)      # sets the ctx's RNS2 moduli (no key here)
        _same(c.eng.debug_chunk_exit(dig, rns2=True), EC.expected_classic(c.p, rows, rns2=(m1, m2)), name + ", RNS2")
    # storage: every coefficient x = Q - 1 under the largest draws, and (randomised) the largest pair the rule admits
    top = ([(c.p.Q - 1 - EC.offset(R)) % c.p.Q] * c.p.m,) * 2
    cases = [(EC.digits(R, top, "max"), top)]
    if rnd:
        cases.append(EC.largest_pair(R))
    dig = np.stack([d for d, _ in cases])
    stored = [row for _, row in cases]
    got, acc = c.eng.debug_chunk_exit(dig, raw=True, want_acc=True)
    _same(got, EC.expected_classic(c.p, stored, raw=True), name + ", largest stored values, raw")
    _same(acc, EC.acc_words(stored), name + ", largest stored values, accumulators")
    _same(c.eng.debug_chunk_exit(dig), EC.expected_classic(c.p, stored), name + ", largest stored values, reduced")


# ---- the exit: LUT rows -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", RINGS)
def test_lut_rows(ctxs, name, rnd):
    """k_final_lut_multi<false>: all 256 tables (16 at Params(1024)) on every LUT row of exit_cases.lut_rows in one
    family call, reduced and raw, and T = 1.  k_final_lut: single-table calls with every row a LUT row (k_final
    skipped), and a descriptor (classic, LUT, classic, LUT, classic): k_final first, k_final_lut over its own rows only."""
    c = ctxs(name)
    R = c.mode(rnd)
    p, rows = c.p, c.luts()
    tabs = np.array([EC.TABLES16 if c.big else range(256)] * len(rows), dtype=np.uint8)
    if not c.big:
        tabs[1::2] = tabs[1::2, ::-1]                         # (rows differ in their table order)
    want = c.once("family ref", lambda: (EC.expected_family(p, rows, tabs), EC.expected_family(p, rows, tabs, raw=True)))
    draws = "crossed" if rnd else "zero"
    dig = EC.digits_of(R, rows, draws)
    _same(c.eng.debug_chunk_exit(dig, tables=tabs), want[0], name + ", family, reduced")
    _same(c.eng.debug_chunk_exit(dig, tables=tabs, raw=True), want[1], name + ", family, raw")
    _same(c.eng.debug_chunk_exit(dig, tables=tabs[:, 3:4]), want[0][:, 3:4], name + ", family of one")
    # single-table calls: column t of the family's reference
    dig = EC.digits_of(R, rows, "max")
    for col in (0, 9, 10) if c.big else (0, 255, 0x96, 0xE8, 0x80):
        words = (EC.LUT_ROW | tabs[:, col].astype(np.uint32)).astype(np.uint32)
        _same(c.eng.debug_chunk_exit(dig, lut=words), want[0][:, col], "%s, single table, column %d" % (name, col))
        _same(c.eng.debug_chunk_exit(dig, lut=words, raw=True), want[1][:, col], "%s, single table, column %d, raw" % (name, col))
    # classic rows and LUT rows in one chunk
    cl = c.classic()
    mixed = [cl[0], rows[0], cl[1], rows[1], cl[-1]]
    words = np.array([0, EC.LUT_ROW | 0x96, 0, EC.LUT_ROW | 0xFC, 0], dtype=np.uint32)
    dig = EC.digits_of(R, mixed, "zero")
    for raw in (False, True):
        got, acc = c.eng.debug_chunk_exit(dig, lut=words, raw=raw, want_acc=True)
        _same(got, EC.expected_mixed(p, mixed, words, raw=raw), "%s, mixed descriptor, raw = %s" % (name, raw))
        _same(acc, EC.acc_words(mixed), name + ", mixed descriptor, accumulators")


# ---- the entry ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", RINGS)
def test_entry(ctxs, name, rnd):
    """k_init: r + 3 rows in one call (5 at Params(1024)) -- every u.b in [0, r) through a sum that wraps, a1 + a2
    wrapping, every third row a LUT row (amplitude DQ_tilde >> 2), a row count that is no multiple of 8 -- then one row
    alone and eight rows without a descriptor.  Randomised: row t draws as bootstrap t of the call, call after call."""
    c = ctxs(name)
    c.mode(rnd)
    p = c.p
    for count, every in ((5, 3), (1, 0)) if c.big else ((p.r + 3, 3), (1, 0), (8, 0)):
        a1, b1, a2, b2, lut = EC.entry_rows(p, count, seed=0x656E + count, lut_every=every)
        if c.big:                                             # u.b = 0 (wrapped), Dr, m, m + Dr, r - 1
            b2[:5] = [(u - int(b1[0])) % p.r for u in (0, p.Dr, p.m, p.m + p.Dr, p.r - 1)][:count]
        dig, ua = c.eng.debug_chunk_entry(a1, b1, a2, b2, lut if every else None)
        want = EC.expected_entry(p, KEY if rnd else None, c.call, a1, b1, a2, b2, lut if every else None)
        c.call += 1 if rnd else 0
        _same(ua, want[1], "%s, %d rows, u.a" % (name, count))
        _same(dig, want[0], "%s, %d rows, digits" % (name, count))


# ---- refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["limb64", "composite"])
def test_refusals_leave_the_ctx_as_it_was(ctxs, name):
    """Every refusal of both entries is SGFHE_ERR_INVALID_ARG before anything is queued or a call number taken, and the
    exit takes none when it runs: a randomised k-loop step before and one after the series draw with consecutive call
    numbers, and the same valid exit call gives the same rows before and after."""
    c = ctxs(name)
    S, p = c.S, c.p
    for rnd in RC.MODES:
        R = c.mode(rnd)
        rows = c.classic()[:2]
        dig = np.ascontiguousarray(EC.digits_of(R, rows, "max"))
        want = EC.expected_classic(p, rows)
        C = KC.key_slice(p, "all +")
        kdig, j = KC.mixed(R, 2, first=1)

        def step():
            got, _ = c.eng.debug_kloop_step(kdig, KC.slice_words(C), j, 1)
            _same(got, KC.expected(p, KEY if rnd else None, c.call, kdig, C, j, 1), name + ", k-loop step")
            c.call += 1 if rnd else 0

        def refused(fn, *args, **kw):
            with pytest.raises(S.SgfheError) as e:
                fn(*args, **kw)
            assert e.value.code == ERR_INVALID_ARG

        step()
        _same(c.eng.debug_chunk_exit(dig), want, name + ", before")
        ex, en = c.eng.debug_chunk_exit, c.eng.debug_chunk_entry
        tabs = np.zeros((2, 1), dtype=np.uint8)
        lutw = np.array([EC.LUT_ROW | 1, 0], dtype=np.uint32)
        refused(ex, np.zeros((0, 2, 2, p.m), dtype=np.uint64))                                   # rows = 0
        refused(ex, dig, tables=np.zeros((2, 257), dtype=np.uint8))                              # T = 257
        refused(c.eng._call, "sgfhe_debug_chunk_exit", dig.ctypes.data, 2, None, tabs.ctypes.data, 0, 0, dig.ctypes.data, None)  # T = 0
        refused(ex, dig, lut=lutw, tables=tabs)                                                  # both descriptors
        refused(ex, dig, lut=np.array([0x200, 0], dtype=np.uint32))                              # not 0 or LUT_ROW | table
        refused(ex, dig, lut=np.array([0x7, 0], dtype=np.uint32))                                # a table without LUT_ROW
        refused(c.eng._call, "sgfhe_debug_chunk_exit", dig.ctypes.data, 2, None, None, 0, 4, dig.ctypes.data, None)     # unknown flag
        refused(c.eng._call, "sgfhe_debug_chunk_exit", dig.ctypes.data, 2, None, None, 0, 2, dig.ctypes.data, None)     # RNS2 without MODQ
        if c.rg.rns2:
            c.eng.rns2_convert(np.zeros((1, 2), dtype=np.uint64), c.rg.rns2[0], c.rg.rns2[1], True)
            refused(ex, dig, lut=lutw, rns2=True)
            refused(ex, dig, tables=tabs, rns2=True)
        else:
            refused(ex, dig, rns2=True)                                                          # no RNS2 moduli
        for (cc, d), over in (((0, 0), R.B + R.draw_max), ((1, 1), R.hi_max + R.draw_max + 1)):
            bad = dig.copy()
            bad[1, cc, d, R.m - 1] = over
            assert not KC.storable(R, *(int(bad[1, cc, e, R.m - 1]) for e in (0, 1)))
            refused(ex, bad)
        if not rnd:                                           # both digits in range, the pair Q itself
            bad = dig.copy()
            bad[0, 1, 0, 0], bad[0, 1, 1, 0] = R.Q % R.B, R.Q // R.B
            refused(ex, bad)
        for args in ((None, 2, None, None, 0, 0, dig.ctypes.data, None), (dig.ctypes.data, 2, None, None, 0, 0, None, None)):
            assert c.eng._L.sgfhe_debug_chunk_exit(c.eng._h, *args) == ERR_INVALID_ARG           # a null pointer
        a1, b1, a2, b2, lut = EC.entry_rows(p, 9, lut_every=2)
        refused(en, a1[:0], b1[:0], a2[:0], b2[:0])                                              # rows = 0
        refused(en, a1, b1, a2, b2, np.full(9, 0x300, dtype=np.uint32))
        over = a1.copy()
        over[1, 0] = p.r                                                                         # row 1 is a LUT row
        refused(en, over, b1, a2, b2, lut)
        out = np.zeros((9, 2, 2, p.m), dtype=np.uint64)
        assert c.eng._L.sgfhe_debug_chunk_entry(c.eng._h, a1.ctypes.data, b1.ctypes.data, a2.ctypes.data, None, 9, None,
                                                out.ctypes.data, out.ctypes.data) == ERR_INVALID_ARG
        c.eng.set_chunk(8)                                    # more rows than one chunk of the ctx
        try:
            refused(en, a1, b1, a2, b2)
            refused(ex, np.concatenate([dig] * 5)[:9])
        finally:
            c.eng.set_chunk(0)
        _same(c.eng.debug_chunk_exit(dig), want, name + ", after")
        step()


# ---- the hooks run what a call runs -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
def test_a_real_call_equals_the_hooks(S, oc, rnd):
    """m128 with a key, 11 rows: bootstrap_batch (reduced and raw) == the exit hook on debug_digits(..., n) of the same rows
    at the same call number, its accumulator tap == debug_accumulators(..., n), and the entry hook == debug_digits(..., 0)."""
    rg = RC.ring(S, "m128")
    p = rg.params
    o, _ = RC.oracles(oc, rg)
    sk = o.private_key(71)
    bits = np.arange(22, dtype=np.uint8) % 3 % 2
    a, b = o.lwe_encrypt_bits(sk, bits, 73)
    rows = (a[0::2], b[0::2], a[1::2], b[1::2])
    eng = S.Engine(p)
    try:
        RC.upload(eng, rg, o.bootstrap_key(sk, 72, noise=rg.noise))

        def fresh():
            RC.set_mode(S, eng, rg, rnd)                      # the call counter starts again: every call below is call 0

        fresh()
        dig = eng.debug_digits(*rows, p.n)
        fresh()
        acc = eng.debug_accumulators(*rows, p.n)
        for raw in (False, True):
            fresh()
            out = eng.bootstrap_batch(*rows, raw=raw)
            got, tap = eng.debug_chunk_exit(dig, raw=raw, want_acc=True)
            _same(got, out, "m128, real call, raw = %s" % raw)
            _same(tap, acc, "m128, accumulator tap")
        fresh()
        dig0 = eng.debug_digits(*rows, 0)
        fresh()
        got0, ua = eng.debug_chunk_entry(*rows)
        _same(got0, dig0, "m128, entry against debug_digits at zero iterations")
        _same(ua, ((rows[0] + rows[2]) % np.uint64(p.r)).astype(np.uint32), "m128, u.a")
        want0, _ = EC.expected_entry(p, KEY if rnd else None, 0, *rows)
        _same(dig0, want0, "m128, debug_digits at zero iterations against the reference")
    finally:
        eng.close()
