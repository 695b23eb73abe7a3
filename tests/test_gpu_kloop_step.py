"""Every form of the k-loop step on chosen operands, one step at a time (sgfhe_debug_kloop_step: the function every
bootstrap call runs per iteration, from caller-chosen stored digits).  The operands and their big-integer reference are
tests/kloop_cases.py (held to the numpy model and the oracle's flatten on the CPU by tests/test_kloop_cases_host.py):
digits at +-B/2 and at the largest stored values of the randomised mode, key residues at +-(Q - 1)/2, the rotations
0, 1, m - 1, m, m + 1, 2m - 1, gates that differ from their neighbours, and values that land on 0, Q - 1, B - 1 and B.
Every comparison is of equal arrays of stored digits.  Before it, the kernels the step reports are held to `forms`
below, which restates the rules documented at ext_form / crt_form of csrc/engine.hip; the last test holds the union of
what was observed to the list of kernels the k-loop has.  Run with `pytest -m gpu`."""

import ctypes
import os

import numpy as np
import pytest

import bigint_oracle as BO
import kloop_cases as KC
import ring_cases as RC
import rns_model as RM

pytestmark = pytest.mark.gpu

KEY = RC.KEY32
ERR_INVALID_ARG = -1
OBSERVED = set()          # every kernel name a step reported after its pair was held to `forms`


# ---- the table: which kernels a step of `gates` gates takes --------------------------------------------------------------

def forms(p, rnd, gates, small_max=None, split_max=7, fused_min=7):
    """(external-product kernels, CRT kernel) by the rules at ext_form / crt_form: a chunk of at most small_max gates
    (padded to 8; 24, 16 from m = 16384) takes the latency kernels, which index `gates` gates; of those, from fused_min
    gates to one round of the 256 compute units (256 / (4 primes)) the fused quarter kernel (m = 4096, 8192), up to
    split_max gates the quarter pair (m >= 4096), where the mode's lean CRT kernel exists and the records have no third
    plane; the CRT is the lean kernel of the mode where the parameter set admits it -- after a quarter form the one that
    reads partial residues, up to 8 gates' worth one coefficient per thread (never with the third plane), else four, in
    the 87-bit instantiation where five primes, Q of 87 bits and B of 44 bits meet -- else k_crt_acc2 / k_crt_acc."""
    m, B, Q = p.m, p.B, p.Q
    logm = m.bit_length() - 1
    wide = bool(rnd) and B >= 1 << 46
    npr = RM.select_npr(logm, B, Q, bool(rnd))
    nq, nb = Q.bit_length(), B.bit_length()
    nl = max(2, -(-nq // 29))
    lean = RM.CrtLean(RM.Consts(p.n, m, Q, B, p.DQ_tilde, bool(rnd), tables=False)).ok
    lean_rnd = lean and (nl >= 3 or 7 * B < 1 << 32 or B >> 29 == 0) and B * B <= Q << 27
    if small_max is None:
        small_max = 16 if logm >= 14 else 24
    cpad = (gates + 7) & ~7
    small = cpad <= small_max
    cnt = gates if small else cpad
    quarter_ok = logm >= 12 and split_max > 0 and (lean_rnd and not wide if rnd else lean)
    fused_cap = 256 // (4 * npr) if fused_min and logm in (12, 13) and quarter_ok else 0
    w = "true" if wide else "false"
    le_small = 3 if 9 <= logm <= 13 else 4
    if small and fused_min <= cnt <= fused_cap:
        ext, quarter = "k_ext_quarter<%d, 3>" % logm, True
    elif small and quarter_ok and cnt <= split_max:
        ext, quarter = "k_fwd_quarter<%d, 3>+k_inv_quarter<%d, 3>" % (logm, logm), True
    elif small:
        ext, quarter = "k_fwd_phase<%d, %d, %s>+k_inv_column<%d, %d>" % (logm, le_small, w, logm, le_small), False
    else:
        ext, quarter = "k_extprod<%d, %d, %s>" % (logm, 3 if logm <= 9 else 4, w), False
    one = cnt <= 8
    if not rnd and lean:
        if quarter:
            crt = "k_crt_lean1q<%d, %d>" % (npr, nl)
        elif one:
            crt = "k_crt_lean1<%d, %d>" % (npr, nl)
        elif npr == 5 and nq == 87 and nb == 44:
            crt = "k_crt_lean<5, 3, true>"
        else:
            crt = "k_crt_lean<%d, %d>" % (npr, nl)
    elif rnd and lean_rnd:
        if quarter or (one and not wide):
            crt = "k_crt_lean_rnd1<%d, %d, %s>" % (npr, nl, "true" if quarter else "false")
        else:
            crt = "k_crt_lean_rnd<%d, %d, %s>" % (npr, nl, w)
    else:
        crt = ("k_crt_acc<%d>" if rnd else "k_crt_acc2<%d>") % npr
    return ext, crt


def test_the_table_itself(S):
    """`forms` against names written out: the throughput pairs of tests/ring_cases.py (what Engine.kernel_names() is
    held to), and one line per form of the reference's parameter sets."""
    for name in RC.NAMES:
        rg = RC.ring(S, name)
        for rnd in RC.MODES:
            assert forms(rg.params, rnd, 25) == rg.kernels[rnd], (name, rnd)
    small64 = "k_fwd_phase<6, 4, false>+k_inv_column<6, 4>"
    assert forms(RC.ring(S, "limb64").params, False, 8) == (small64, "k_crt_lean1<4, 3>")
    assert forms(RC.ring(S, "limb64").params, True, 9) == (small64, "k_crt_lean_rnd<5, 3, false>")
    assert forms(RC.ring(S, "tiny").params, True, 1) == (small64, "k_crt_acc<2>")
    assert forms(RC.ring(S, "wide").params, True, 1) == ("k_fwd_phase<6, 4, true>+k_inv_column<6, 4>", "k_crt_lean_rnd<6, 4, true>")
    p512, p1024, p2048 = S.Params(512), S.Params(1024), S.Params(2048)
    q12, q13, q14 = ("k_fwd_quarter<%d, 3>+k_inv_quarter<%d, 3>" % (lm, lm) for lm in (12, 13, 14))
    assert forms(p512, False, 6) == (q12, "k_crt_lean1q<5, 3>") and forms(p512, True, 1) == (q12, "k_crt_lean_rnd1<5, 3, true>")
    assert forms(p512, False, 7) == forms(p512, False, 12) == ("k_ext_quarter<12, 3>", "k_crt_lean1q<5, 3>")
    assert forms(p512, False, 13) == ("k_fwd_phase<12, 3, false>+k_inv_column<12, 3>", "k_crt_lean<5, 3>")
    assert forms(p1024, False, 1) == (q13, "k_crt_lean1q<5, 3>")
    assert forms(p1024, False, 13) == ("k_fwd_phase<13, 3, false>+k_inv_column<13, 3>", "k_crt_lean<5, 3, true>")
    assert forms(p1024, False, 25) == ("k_extprod<13, 4, false>", "k_crt_lean<5, 3, true>")
    assert forms(p1024, True, 10) == ("k_ext_quarter<13, 3>", "k_crt_lean_rnd1<6, 3, true>")
    assert forms(p1024, True, 11) == ("k_fwd_phase<13, 3, false>+k_inv_column<13, 3>", "k_crt_lean_rnd<6, 3, false>")
    assert forms(p2048, False, 7) == (q14, "k_crt_lean1q<6, 4>")
    assert forms(p2048, False, 8) == ("k_fwd_phase<14, 4, false>+k_inv_column<14, 4>", "k_crt_lean1<6, 4>")
    assert forms(p2048, True, 1) == ("k_fwd_phase<14, 4, true>+k_inv_column<14, 4>", "k_crt_lean_rnd<6, 4, true>")
    assert forms(p512, False, 8, split_max=0) == ("k_fwd_phase<12, 3, false>+k_inv_column<12, 3>", "k_crt_lean1<5, 3>")
    assert forms(p512, False, 1, fused_min=1) == ("k_ext_quarter<12, 3>", "k_crt_lean1q<5, 3>")


# ---- one ctx per ring, no key --------------------------------------------------------------------------------------------

class Ctx:
    def __init__(self, S, p):
        self.S, self.p, self.eng = S, p, S.Engine(p)
        self.rnd, self.call = False, 0
        self.slices, self.views = {}, {}

    def mode(self, rnd):
        self.eng.set_random_flatten(bool(rnd), KEY if rnd else 0)     # the call counter starts again
        self.rnd, self.call = bool(rnd), 0
        if rnd not in self.views:
            self.views[rnd] = KC.RingView(self.p, rnd)
        return self.views[rnd]

    def slice(self, name):
        """(C, its words, the shared Products) per (slice, mode)."""
        key = (name, self.rnd)
        if key not in self.slices:
            C = KC.key_slice(self.p, name)
            self.slices[key] = (C, KC.slice_words(C), KC.Products(self.views[self.rnd], C))
        return self.slices[key]

    def check(self, digits, slice_name, j, k=0, want_names=None, label=""):
        """One step: the reported kernels == want_names, the digits == the reference."""
        C, words, prods = self.slice(slice_name)
        got, names = self.eng.debug_kloop_step(digits, words, j, k)
        call = self.call
        self.call += 1 if self.rnd else 0
        if want_names is not None:
            assert names == want_names, (label, len(j), names, want_names)
            OBSERVED.update(names[0].split("+") + [names[1]])
        want = KC.expected(self.p, KEY if self.rnd else None, call, digits, C, j, k, prods)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d gates, %s, slice %r, k = %d: %d digits differ, first at (gate, c, digit, i) = %s, j = %s" % (
            label, len(j), names, slice_name, k, len(bad), tuple(bad[0]), list(j))
        return got


@pytest.fixture(scope="module")
def ctxs(S):
    made = {}

    def get(name, params=None):
        if name not in made:
            made[name] = Ctx(S, params() if params else RC.ring(S, name).params)
        return made[name]
    yield get
    for c in made.values():
        c.eng.close()


def _run_counts(c, rnd, counts, families, label, **knobs):
    """For every gate count a mixed call (kloop_cases.mixed: the families and rotations dealt round, starting one further
    each time), the slices by turns."""
    R = c.mode(rnd)
    for t, gates in enumerate(counts):
        digits, j = KC.mixed(R, gates, first=t, families=families)
        sl = "rows" if gates == 1 and R.m <= 8192 else KC.SLICES[t % 3]      # (eight big products a gate: one gate only)
        c.check(digits, sl, j, k=(t * 5) % R.n, want_names=forms(c.p, rnd, gates, **knobs), label=label)


# ---- rings of m = 64 and 128: small and throughput forms, every CRT kind ------------------------------------------------------

@pytest.mark.parametrize("rnd", RC.MODES, ids=RC.MODE_IDS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_small_rings(ctxs, name, rnd):
    """1, 8 gates: the latency kernels with one coefficient per CRT thread; 9, 24: with four; 25: k_extprod; and one gate
    with the small-batch form off: k_extprod on a chunk padded to 8.  Then every family against every slice at the special
    rotations in one call of 8 gates per slice, the zero slice (the CRT stage's identity) and the value wrap."""
    c = ctxs(name)
    R = c.mode(rnd)
    _run_counts(c, rnd, (1, 8, 9, 24, 25), KC.FAMILIES, name)
    rot = KC.rotations(R.m)
    fams = np.stack([KC.family(R, f) for f in KC.FAMILIES])
    for t, sl in enumerate(KC.SLICES):
        j = np.array([rot[(g + 3 * t) % 8] for g in range(8)], dtype=np.uint32)
        got = c.check(fams, sl, j, k=R.n - 1, want_names=forms(c.p, rnd, 8), label=name)
        if sl == "zero" and not rnd:
            assert np.array_equal(got, fams)
    for col, sl in ((0, "b to a"), (1, "a to b")):
        C = c.slice(sl)[0]
        other = KC.family(R, "alternating")[1 - col]
        gates = [KC.wrap_gate(R, C, col, other, rot[g + 2], KEY if rnd else None, c.call, g, 1) for g in range(3)]
        c.check(np.stack(gates), sl, np.array(rot[2:5], dtype=np.uint32), k=1, want_names=forms(c.p, rnd, 3), label=name)
    c.eng.set_small_batch_max(0)
    try:
        digits, j = KC.mixed(R, 1, first=5)
        c.check(digits, "alternating", j, want_names=forms(c.p, rnd, 1, small_max=0), label=name + ", small batch off")
    finally:
        c.eng.set_small_batch_max(24)


# ---- m = 4096, 8192, 16384: the quarter and fused forms ------------------------------------------------------------------

BIG = {
    "p512": lambda S: S.Params(512),
    "p1024": lambda S: S.Params(1024),
    # two limbs of Q through the quarter form (four primes in both modes: the fused kernel takes 7 to 16 gates)
    "two-limb": lambda S: S.Params.custom(512, BO.find_modulus(16 * 512, 1 << 52), 1 << 27),
    "p2048": lambda S: S.Params(2048),
}
# (ring, randomised, gate counts of one test): every test's reference stays within 25 gates (8 at m = 16384)
BIG_CASES = [("p512", False, (1, 6, 7)), ("p512", False, (12, 13)), ("p512", True, (1, 6, 7)), ("p512", True, (12, 13)),
             ("p1024", False, (1, 7, 12)), ("p1024", False, (13,)), ("p1024", False, (25,)),
             ("p1024", True, (1, 7)), ("p1024", True, (10, 11)),
             ("two-limb", False, (1, 7)), ("two-limb", False, (16,)), ("two-limb", False, (17,)), ("two-limb", True, (6, 16)),
             ("p2048", False, (1, 7)), ("p2048", False, (8,)), ("p2048", True, (1,))]
BIG_FAMILIES = ("all +", "halves", "crossed draws", "alternating", "all -")


@pytest.mark.parametrize("name,rnd,counts", BIG_CASES,
                         ids=["%s-%s-%s" % (n, RC.MODE_IDS[r], "+".join(map(str, cs))) for n, r, cs in BIG_CASES])
def test_quarter_rings(S, ctxs, name, rnd, counts):
    """m = 4096, 8192: the quarter pair up to 6 gates, the fused kernel from 7 to its cap (12 on five primes, 10 on six, 16
    on four), the small form past it (k_crt_lean four per thread: at Params(1024) the 87-bit instantiation), k_extprod at 25.
    m = 16384 (Params(2048)): deterministic, the quarter pair up to 7 gates (no fused kernel at this size) and the small
    form at 8; randomised, the records carry the third plane and no quarter form exists: one gate takes the small form
    and the WIDE CRT kernel.  Two families there, three on 16 gates and more (the reference's cost)."""
    c = ctxs(name, lambda: BIG[name](S))
    fams = BIG_FAMILIES
    if name == "p2048":
        fams = ("all +", "crossed draws") if rnd else ("all +", "halves")
        assert not rnd or "quarter" not in "".join(forms(c.p, True, 1))
    elif max(counts) >= 16:
        fams = BIG_FAMILIES[:3]
    _run_counts(c, rnd, counts, fams, name)


def test_special_rotations_through_the_quarter_forms(S, ctxs):
    """m = 4096, both modes: j = 0, 1, m - 1, m, m + 1, 2m - 1 and the two mid-range ones, one gate each -- six gates through
    the quarter pair, then all eight through the fused kernel -- on extreme digits of alternating sign, and the value wrap
    through the quarter CRT kernels."""
    c = ctxs("p512", lambda: S.Params(512))
    for rnd in RC.MODES:
        R = c.mode(rnd)
        rot = KC.rotations(R.m)
        dig = np.stack([KC.family(R, "alternating" if g & 1 else "halves") for g in range(8)])
        c.check(dig[:6], "alternating", np.array(rot[:6], dtype=np.uint32), want_names=forms(c.p, rnd, 6), label="p512")
        c.check(dig, "rows", np.array(rot, dtype=np.uint32), k=R.n - 1, want_names=forms(c.p, rnd, 8), label="p512")
        C = c.slice("b to a")[0]
        gate = KC.wrap_gate(R, C, 0, KC.family(R, "all +")[1], R.m, KEY if rnd else None, c.call, 0, 2)
        c.check(gate[None], "b to a", np.array([R.m], dtype=np.uint32), k=2, want_names=forms(c.p, rnd, 1), label="p512 wrap")


def test_first_and_last_iteration(ctxs):
    """k = 0 and k = n - 1 on one ring in both modes: the u.a index and the draw tag."""
    c = ctxs("m128")
    for rnd in RC.MODES:
        R = c.mode(rnd)
        digits, j = KC.mixed(R, 3, first=2)
        for k in (0, R.n - 1):
            c.check(digits, "all +", j, k=k, want_names=forms(c.p, rnd, 3), label="m128")


@pytest.mark.parametrize("knob,value,gates,kw", [("SGFHE_SMALL_SPLIT", "0", 8, dict(split_max=0)),
                                                 ("SGFHE_SMALL_SPLIT", "0", 1, dict(split_max=0)),
                                                 ("SGFHE_SMALL_FUSED", "1", 1, dict(fused_min=1))])
def test_environment_knobs(S, knob, value, gates, kw):
    """A fresh ctx at m = 4096 under the knobs tests/test_gpu_round4.py uses: without the quarter forms 1 to 8 gates take
    k_fwd_phase + k_inv_column and k_crt_lean1; with the fused kernel from one gate, one gate takes k_ext_quarter."""
    old = os.environ.get(knob)
    os.environ[knob] = value
    try:
        c = Ctx(S, S.Params(512))
    finally:
        if old is None:
            del os.environ[knob]
        else:
            os.environ[knob] = old
    try:
        R = c.mode(False)
        want = forms(c.p, False, gates, **kw)
        assert want[1] == ("k_crt_lean1<5, 3>" if knob == "SGFHE_SMALL_SPLIT" else "k_crt_lean1q<5, 3>")
        digits, j = KC.mixed(R, gates, first=3, families=BIG_FAMILIES)
        c.check(digits, "alternating", j, want_names=want, label=knob)
    finally:
        c.eng.close()


def test_refusals_leave_the_ctx_as_it_was(ctxs):
    """Every refusal of the entry is SGFHE_ERR_INVALID_ARG before anything is queued or a call number taken: the same
    valid call, before and after, draws with consecutive call numbers and equals the reference both times."""
    c = ctxs("limb64")
    S = c.S
    for rnd in RC.MODES:
        R = c.mode(rnd)
        digits, j = KC.mixed(R, 2, first=1)
        digits = np.ascontiguousarray(digits)
        words = c.slice("all +")[1]
        c.check(digits, "all +", j, k=1, want_names=forms(c.p, rnd, 2), label="before")

        def refused(d=digits, w=words, jj=j, k=1):
            with pytest.raises(S.SgfheError) as e:
                c.eng.debug_kloop_step(d, w, jj, k)
            assert e.value.code == ERR_INVALID_ARG

        refused(k=R.n)
        refused(jj=np.array([0, 2 * R.m], dtype=np.uint32))
        refused(d=np.zeros((0, 2, 2, R.m), dtype=np.uint64), jj=np.zeros(0, dtype=np.uint32))
        for (cc, d), over in (((0, 0), R.B + R.draw_max), ((1, 1), R.hi_max + R.draw_max + 1)):
            bad = digits.copy()
            bad[1, cc, d, R.m - 1] = over
            assert not KC.storable(R, *(int(bad[1, cc, e, R.m - 1]) for e in (0, 1)))
            refused(d=bad)
        if not rnd:                                       # both digits in range, the pair Q itself
            bad = digits.copy()
            bad[0, 1, 0, 0], bad[0, 1, 1, 0] = R.Q % R.B, R.Q // R.B
            assert R.Q // R.B <= R.hi_max and not KC.storable(R, R.Q % R.B, R.Q // R.B)
            refused(d=bad)
        names = (ctypes.create_string_buffer(96), ctypes.create_string_buffer(96))
        many = 1 << 20                                    # more gates than any chunk: refused on the count alone
        with pytest.raises(S.SgfheError) as e:
            c.eng._call("sgfhe_debug_kloop_step", digits.ctypes.data, words.ctypes.data, j.ctypes.data, many, 0,
                        digits.ctypes.data, names[0], 96, names[1], 96)
        assert e.value.code == ERR_INVALID_ARG
        assert c.eng._L.sgfhe_debug_kloop_step(c.eng._h, None, words.ctypes.data, j.ctypes.data, 2, 0, digits.ctypes.data,
                                               names[0], 96, names[1], 96) == ERR_INVALID_ARG
        c.check(digits, "all +", j, k=1, want_names=forms(c.p, rnd, 2), label="after")


def _u128(vals):
    out = np.zeros((len(vals), 2), dtype=np.uint64)
    out[:, 0] = [v & 0xFFFFFFFFFFFFFFFF for v in vals]
    out[:, 1] = [v >> 64 for v in vals]
    return out


@pytest.mark.parametrize("name", ["m128", "p512"])
def test_equals_the_cmux_hook(S, ctxs, name):
    """Deterministic, one gate, the small-batch form off: the step is sgfhe_debug_cmux's (k_flatten_canon -> k_extprod ->
    the CRT kernel four per thread) on the same operands -- the accumulators the digits store in, the accumulators of the
    digits it returns out."""
    c = ctxs(name, (lambda: S.Params(512)) if name == "p512" else None)
    R = c.mode(False)
    off = (1 + R.B) * R.s
    c.eng.set_small_batch_max(0)
    try:
        for fam, sl, j in (("+ a, - b", "+ col 0, - col 1", R.m), ("mid", "alternating", 2 * R.m - 1)):
            dig = KC.family(R, fam)
            acc = [[(int(lo) + int(hi) * R.B - off) % R.Q for lo, hi in zip(dig[cc, 0], dig[cc, 1])] for cc in range(2)]
            got = c.check(dig[None], sl, np.array([j], dtype=np.uint32), want_names=forms(c.p, False, 1, small_max=0), label=name)
            ra, rb = c.eng.debug_cmux(_u128(acc[0]), _u128(acc[1]), c.slice(sl)[1], j)
            for cc, res in enumerate((ra, rb)):
                vals = [int(lo) | (int(hi) << 64) for lo, hi in np.ascontiguousarray(res).reshape(-1, 2)]
                mine = [(int(lo) + int(hi) * R.B - off) % R.Q for lo, hi in zip(got[0, cc, 0], got[0, cc, 1])]
                assert vals == mine, (name, fam, cc)
    finally:
        c.eng.set_small_batch_max(16 if R.m >= 16384 else 24)


def test_every_kloop_kernel_was_observed():
    """Last: the union of the kernels reported above (each after its pair was held to `forms`) covers the k-loop's list."""
    base = set()
    for n in OBSERVED:                                    # the last template argument tells the instantiations apart
        stem, last = n.split("<")[0], n.endswith("true>")
        if stem in ("k_extprod", "k_fwd_phase", "k_crt_lean_rnd"):
            base.add(stem + ("<wide>" if last else ""))
        elif stem == "k_crt_lean_rnd1":
            base.add(stem + ("<quarter>" if last else "<whole>"))
        elif stem == "k_crt_lean":
            base.add(n if last else stem)
        else:
            base.add(stem)
    want = {"k_extprod", "k_extprod<wide>", "k_fwd_phase", "k_fwd_phase<wide>", "k_inv_column", "k_fwd_quarter", "k_inv_quarter",
            "k_ext_quarter", "k_crt_lean", "k_crt_lean<5, 3, true>", "k_crt_lean1", "k_crt_lean1q", "k_crt_lean_rnd",
            "k_crt_lean_rnd<wide>", "k_crt_lean_rnd1<quarter>", "k_crt_lean_rnd1<whole>", "k_crt_acc2", "k_crt_acc"}
    assert want <= base, sorted(want - base)
