"""Gathered calls across clones (sgfhe_ctx_clone, csrc/coalescer.h, coalesced_call in engine.hip) at compositions
the tests choose (tests/gather.py): which requests share a combined call, in which order, with how many rows, on
which leader and in which kernel form -- asserted through sgfhe_coalesce_stats and the leader's own timing record,
never taken from a race.  Every caller's bytes equal the same call made alone (a clone with gathering off, same
flatten key and call number), and one caller per case is held against the C oracle: live at Params(64) / (512) and
the small RNS2 ring, through the recorded digests of tests/golden/gpu_expect.json at Params(1024) / (2048)
(SGFHE_EXPECT_RECORD=1 records them on the CPU; the engine halves do not run then).

What the GPU cannot show: the padded rows of a chunk read the per-row stream table past the gathered rows
(kernels.h rnd_stream<true>), and their results are dropped.  The length of that table is checked by brute force on
the CPU (tests/native/coalescer_tsan.cpp); the row-table cases here pin the bytes of the rows that count at the
totals where the table ends."""

import os
import re

import numpy as np
import pytest

import bigint_oracle as BO
import gather as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(t):
    return bytes((29 * t + 7 * i + 1) & 0xFF for i in range(32))


def _engine_default(name):
    """A ctx default as engine.hip declares it (`uint32_t small_max = 24;`): the boundaries are read, not guessed."""
    src = open(os.path.join(ROOT, "sgfhe.jl_amd", "csrc", "engine.hip")).read()
    m = re.search(r"^\s*uint32_t %s = (\d+);" % name, src, re.M)
    assert m, name
    return int(m.group(1))


class Planner:
    """bootstrap_device's choice of chunks (engine.hip) for a ctx in its default state, from the defaults read above."""

    def __init__(self, eng, params):
        self.logm = params.m.bit_length() - 1
        self.small_max = _engine_default("small_max")
        self.small_lanes_max = _engine_default("small_lanes_max")
        if self.logm >= 14:                                  # sgfhe_ctx_create: m = 16384 ends the latency form at 16
            self.small_max = min(self.small_max, 16)
            self.small_lanes_max = min(self.small_lanes_max, 16)
        # fused_cap(): one workgroup per (gate, prime, quarter) on 256 compute units, m = 4096 / 8192, where the
        # mode's CRT kernel is the lean one (quarter_ok) -- in the mode `eng` is in now
        lean = eng.kernel_names()[1].startswith("k_crt_lean")
        on = _engine_default("fused_min") and _engine_default("split_max") and lean and self.logm in (12, 13)
        self.fused_cap = 256 // (len(eng.primes()) * 4) if on else 0

    def first_chunk(self, total, chunk=0, lanes=2, small_max=None):
        """Padded size of the first chunk of a call of `total` rows (what sgfhe_timing_read reports as `chunk`)."""
        sm = self.small_max if small_max is None else small_max
        ch = chunk or 1 << 20                                # default_chunk: hundreds of rows, above every total here
        if not chunk and lanes == 2 and total > 2 * sm:
            ch = (((total + 1) // 2) + 7) & ~7               # an even number of equal chunks: here two
        elif (not chunk and lanes == 2 and self.logm >= 12 and total >= (self.fused_cap + 1 if self.fused_cap else 8)
              and total <= self.small_lanes_max and (total + 1) // 2 <= sm):
            ch = (total + 1) // 2                            # two halves in the latency form, not rounded to 8
        return (min(total, ch) + 7) & ~7

    def form(self, total, **kw):
        sm = kw.get("small_max")
        return "latency" if self.first_chunk(total, **kw) <= (self.small_max if sm is None else sm) else "throughput"

    def edges(self):
        """Totals on each side of every boundary of the planner."""
        e = {7, 8, 9, 15, 16, 17, self.small_max, self.small_max + 1, 2 * self.small_max + 1,
             self.small_lanes_max, self.small_lanes_max + 1}
        if self.fused_cap:
            e |= {self.fused_cap, self.fused_cap + 1}
        if self.logm >= 12:
            e.add(13)                                        # halves of 7 + 6: not multiples of 8
        return sorted(e)


def _split(total):
    """Three followers whose sizes add up to `total`, none a multiple of 8 where that can be helped."""
    a = 1 if total < 12 else 3
    b = max(1, total // 2 - 1)
    if b % 8 == 0:
        b -= 1
    return [a, b, total - a - b]


def _same(got, ref, what):
    assert isinstance(got, np.ndarray), (what, got)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), what


def _oracle(exp, gpu_keys, n, how, got, job):
    """One caller against the C oracle: how = "live", or the tag of its recorded digest (None: not this caller)."""
    if how is None:
        return
    o, _sk = gpu_keys.oracle(n)
    rnd = {} if job.key is None else dict(rnd=(job.key, job.call))
    compute = lambda: o.bootstrap_batch(gpu_keys.khat(n), *job.work, opt=True, raw=job.raw, **rnd)
    if how == "live":
        assert np.array_equal(got, compute()), "caller differs from the oracle"
    else:
        exp.check(how, got, compute)


def _gathered_case(exp, gpu_keys, n, sizes, rnd, seed, oracle="live", leader=None, knobs=None, planner_kw=None,
                   leader_at=0, oracle_job=0):
    """Followers of `sizes` gates, all deterministic or all randomised (each on its own key; follower t makes call
    number t % 3 of its stream), in one round; every caller against its call alone, the leader's record against
    the planner, one caller against the oracle.  `leader`: configures the clone that leads (or, with leader_at != 0,
    that follows at that place).  Returns the followers' results."""
    params = gpu_keys.S.Params(n)
    if exp.record:                                           # the oracle half only
        if oracle not in (None, "live"):
            j = G.Job(None, G.inputs(params, sizes[oracle_job], seed + oracle_job), _key(oracle_job) if rnd else None,
                      oracle_job % 3)
            _oracle(exp, gpu_keys, n, oracle, None, j)
        return None
    _p, _o, _sk, eng = gpu_keys.engine(n)
    eng.set_random_flatten(False)
    clones = [eng.clone() for _ in sizes]
    bl = G.Blocker(eng, params)
    try:
        if leader:
            leader(clones[leader_at])
        jobs = [G.Job(c, G.inputs(params, g, seed + t), _key(t) if rnd else None, t % 3)
                for t, (c, g) in enumerate(zip(clones, sizes))]
        ref = G.alone(eng, jobs)
        for c in clones:
            c.timing_enable(True)
            c.timing_read(reset=True)
        got = G.run(eng, bl, jobs, [list(range(len(jobs)))], **(knobs or {}))
        for t, (g, r) in enumerate(zip(got, ref)):
            _same(g, r, (n, sizes, rnd, t))
        # the first follower led, once, with every row; the others ran nothing but the one-gate calls that brought
        # their call counters to t % 3 (a re-attempt of the composition repeats those: not counted then)
        total = sum(sizes)
        lead = clones[0].timing_read()
        if G.LOG[-1]["attempt"] == 0:
            assert lead["calls"] == 1 and lead["call_batch"] == total, lead
            for t, c in enumerate(clones[1:], 1):
                tr = c.timing_read()
                assert tr["calls"] == (t % 3 if rnd else 0) and tr["call_batch"] <= 1, (t, tr)
        want_crt = "k_crt_lean_rnd<" if rnd else "k_crt_lean<"
        if clones[0].kernel_names()[1].startswith("k_crt_lean"):
            assert clones[0].kernel_names()[1].startswith(want_crt)
        if planner_kw is not None:
            pl = Planner(clones[0], params)
            assert lead["chunk"] == pl.first_chunk(total, **planner_kw), (lead, total, planner_kw)
        _oracle(exp, gpu_keys, n, oracle, got[oracle_job], jobs[oracle_job])
        return got
    finally:
        eng.set_coalesce(True)
        eng.set_random_flatten(False)
        bl.close()
        for c in clones:
            c.close()


@pytest.mark.parametrize("rnd", [False, True], ids=["det", "rnd"])
@pytest.mark.parametrize("n", [64, 512, 1024])
def test_row_count_edges_of_the_launch_planner(S, oc, exp, gpu_keys, n, rnd):
    """Combined totals on each side of every boundary bootstrap_device has, in both flatten modes: multiples of 8 +- 1,
    fused_cap and fused_cap + 1 (m = 4096, 8192), the 8-gate and small_lanes_max limits of the two-half latency form
    (13 -> 7 + 6), small_max and small_max + 1 (latency -> throughput form), 2 small_max + 1 (two lanes).  The form
    that ran: the mode's CRT kernel by sgfhe_kernel_names, and the first chunk's padded size on the leader
    (sgfhe_timing_read) against the planner restated here -- it decides the form: at most small_max rows per chunk is
    the latency form.  Params(64): a wave of the CRT kernel spans rows.  (sgfhe_kernel_names names the kernels of the ctx's flatten
    mode, not of a call: that assertion only restates the mode the round ran in; the chunk figure is the form check.)"""
    params = S.Params(n)
    tag = "gather.edges.1024.%s" % ("rnd" if rnd else "det")
    if exp.record:
        if n == 1024:
            total = _engine_default("small_max") + 1
            _gathered_case(exp, gpu_keys, n, _split(total), rnd, 8100 + total, oracle=tag)
        return
    _p, _o, _sk, eng = gpu_keys.engine(n)
    eng.set_random_flatten(rnd, _key(0))
    try:
        pl = Planner(eng, params)
    finally:
        eng.set_random_flatten(False)
    edges = pl.edges()
    # the cases do sit on both sides of the form boundaries
    assert pl.form(pl.small_max) == "latency" and pl.form(pl.small_max + 1) == "throughput"
    assert pl.first_chunk(2 * pl.small_max) == 2 * pl.small_max and pl.first_chunk(2 * pl.small_max + 1) < 2 * pl.small_max
    if pl.logm >= 12:
        assert pl.fused_cap < 13 and pl.first_chunk(13) == 8
        assert pl.first_chunk(pl.small_lanes_max) == ((pl.small_lanes_max + 1) // 2 + 7) & ~7
        assert pl.first_chunk(pl.small_lanes_max + 1) == (pl.small_lanes_max + 8) & ~7
    if pl.fused_cap:
        assert pl.first_chunk(pl.fused_cap) == (pl.fused_cap + 7) & ~7
        assert pl.first_chunk(pl.fused_cap + 1) == ((pl.fused_cap + 2) // 2 + 7) & ~7
    for total in edges:
        # the oracle: live at Params(64); at Params(512) live at 13 and small_max + 1 (three rows each); at
        # Params(1024) the recorded digest at small_max + 1
        if n == 64:
            how = "live"
        elif n == 512:
            how = "live" if total in (13, pl.small_max + 1) else None
        else:
            how = tag if total == pl.small_max + 1 else None
        assert _gathered_case(exp, gpu_keys, n, _split(total), rnd, 8100 + total, planner_kw={}, oracle=how) is not None


def test_wide_digit_plane_gathered_at_params_2048(S, oc, exp, gpu_keys):
    """Params(2048), randomised: B > 2^46, the WIDE instantiations of the ROWS kernels (third digit plane), at
    small_max + 1 = 17 rows (m = 16384 ends the latency form at 16): one chunk in the throughput form."""
    got = _gathered_case(exp, gpu_keys, 2048, [2, 6, 9], True, 8300, oracle="gather.wide.2048.rnd.17", planner_kw={})
    if got is not None:
        _p, _o, _sk, eng = gpu_keys.engine(2048)
        eng.set_random_flatten(True, _key(0))
        try:
            assert eng.kernel_names()[0] == "k_extprod<14, 4, true>"
        finally:
            eng.set_random_flatten(False)


@pytest.mark.parametrize("gates_max,totals", [(100, (100, 97, 99, 100)), (64, (64, 40, 64))])
def test_row_table_ends(S, oc, exp, gpu_keys, gates_max, totals):
    """Randomised rounds whose rows end where the leader's stream table ends: gates_max = 100 with 97, 99 and 100
    gathered gates (the padded rows of the last chunk index past row 99), a gates_max that is a multiple of 8 with
    that many gates, and -- the clones and so the leader's table are kept across the totals -- a smaller round
    after a larger one, so that the table holds the larger round's rows behind the smaller one's."""
    if exp.record:
        return
    n = 64
    params, _o, _sk, eng = gpu_keys.engine(n)
    eng.set_random_flatten(False)
    clones = [eng.clone() for _ in range(4)]
    bl = G.Blocker(eng, params)
    try:
        for k, total in enumerate(totals):
            k31 = (total + 30) // 31
            sizes = [total - 31 * (k31 - 1)] + [31] * (k31 - 1)
            jobs = [G.Job(c, G.inputs(params, g, 8400 + 10 * k + t), _key(t + k), t % 3)
                    for t, (c, g) in enumerate(zip(clones, sizes))]
            ref = G.alone(eng, jobs)
            got = G.run(eng, bl, jobs, [list(range(len(jobs)))], req_max=32, gates_max=gates_max)
            for t, (g, r) in enumerate(zip(got, ref)):
                _same(g, r, (gates_max, total, t))
            _oracle(exp, gpu_keys, n, "live", got[0], jobs[0])       # the leader's few rows
    finally:
        eng.set_coalesce(True)
        bl.close()
        for c in clones:
            c.close()


def _knob_chunk8(c):
    c.set_chunk(8)


def _knob_one_lane(c):
    c.set_lanes(1)


def _knob_no_small(c):
    c.set_small_batch_max(0)


@pytest.mark.parametrize("n", [64, 512])
def test_leaders_knobs_leave_the_followers_bytes_alone(S, oc, exp, gpu_keys, n):
    """The same 20 randomised rows (7 + 4 + 9) three times, led by a clone with set_chunk(8) on two lanes (three
    chunks: ra.chunk is 8 on the second lane and 16 on the first), with set_lanes(1), with set_small_batch_max(0);
    then once more with the chunk-8 clone following: the combined call runs on the leader's ctx state, and nobody's
    bytes depend on it."""
    if exp.record:
        return
    first = None
    for leader, at, kw in ((_knob_chunk8, 0, dict(chunk=8)), (_knob_one_lane, 0, dict(lanes=1)),
                           (_knob_no_small, 0, dict(small_max=0)), (_knob_chunk8, 1, {})):
        got = _gathered_case(exp, gpu_keys, n, [7, 4, 9], True, 8500, leader=leader, leader_at=at, planner_kw=kw,
                             oracle_job=1, oracle="live" if first is None else None)     # (the later runs: same bytes)
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert a.tobytes() == b.tobytes()


def test_grouping_one_round_per_key(S, oc, exp, gpu_keys):
    """Plain, raw, randomised and randomised-raw requests queued together, two of each in mixed order: four rounds, one
    per (flags, mode) key, led in the order the keys first arrived; each caller gets its own shape and bytes."""
    if exp.record:
        return
    n = 64
    params, _o, _sk, eng = gpu_keys.engine(n)
    eng.set_random_flatten(False)
    kinds = [(False, False), (True, False), (False, True), (True, True), (False, True), (False, False), (True, True),
             (True, False)]                                   # (raw, randomised) in arrival order
    clones = [eng.clone() for _ in kinds]
    bl = G.Blocker(eng, params)
    try:
        jobs = [G.Job(c, G.inputs(params, 2 + t, 8600 + t), _key(t) if rnd else None, t % 2, raw=raw)
                for t, (c, (raw, rnd)) in enumerate(zip(clones, kinds))]
        ref = G.alone(eng, jobs)
        got = G.run(eng, bl, jobs, [[0, 5], [1, 7], [2, 4], [3, 6]])
        for t, (g, r) in enumerate(zip(got, ref)):
            _same(g, r, (kinds[t], t))
            assert g.shape == (2 + t, 3, n + 1) + ((2,) if kinds[t][0] else ())
        for t in (4, 7, 6):                                   # a follower of each non-plain round against the oracle
            _oracle(exp, gpu_keys, n, "live", got[t], jobs[t])
    finally:
        eng.set_coalesce(True)
        bl.close()
        for c in clones:
            c.close()


@pytest.mark.parametrize("rnd", [False, True], ids=["det", "rnd"])
def test_gates_max_cuts_the_round(S, oc, exp, gpu_keys, rnd):
    """Followers of 9 + 12 + 11 + 7 + 5 gates under gates_max = 32: the prefix that fits (9 + 12 + 11 = 32, exactly)
    runs, the rest in the next round; then 20 + 14 + 4, where the 14 does not fit behind the 20 and the 4 behind it
    does.  The requests left behind get their own bytes and, randomised, their own call numbers."""
    if exp.record:
        return
    n = 64
    params, _o, _sk, eng = gpu_keys.engine(n)
    eng.set_random_flatten(False)
    sizes = [9, 12, 11, 7, 5]
    clones = [eng.clone() for _ in sizes]
    bl = G.Blocker(eng, params)
    try:
        jobs = [G.Job(c, G.inputs(params, g, 8700 + t), _key(t) if rnd else None, (t + 1) % 3)
                for t, (c, g) in enumerate(zip(clones, sizes))]
        ref = G.alone(eng, jobs)
        got = G.run(eng, bl, jobs, [[0, 1, 2], [3, 4]], req_max=16, gates_max=32)
        for t, (g, r) in enumerate(zip(got, ref)):
            _same(g, r, (rnd, t))
        _oracle(exp, gpu_keys, n, "live", got[4], jobs[4])
        sizes2 = [20, 14, 4]
        jobs2 = [G.Job(c, G.inputs(params, g, 8750 + t), _key(t) if rnd else None, t % 3)
                 for t, (c, g) in enumerate(zip(clones, sizes2))]
        ref2 = G.alone(eng, jobs2)
        got2 = G.run(eng, bl, jobs2, [[0, 2], [1]], req_max=20, gates_max=32)
        for t, (g, r) in enumerate(zip(got2, ref2)):
            _same(g, r, (rnd, "skip", t))
    finally:
        eng.set_coalesce(True)
        bl.close()
        for c in clones:
            c.close()


def _ints(arr):
    flat = np.ascontiguousarray(arr).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in flat]


def test_rns2_moduli_across_clones(S, oc, exp, gpu_keys):
    """SGFHE_FLAG_RAW_RNS2 from three sharers of one key whose RNS2 state differs: the parent took the key as canonical
    residues and has no moduli, clone X was configured (B, Bp) by sgfhe_rns2_convert, clone Y (Bp, B).  Queued
    together, with each of the three leading in turn: X and Y get their own limb order (src/rns.jl:16-18 of the
    canonical raw output, which is held against the C oracle), the parent SGFHE_ERR_INVALID_ARG with its own message
    -- whoever leads.  Results only: whether these requests share a round is the engine's business."""
    if exp.record:
        return
    n, m = 32, 256
    Bp = BO.find_modulus(2 * m, 1 << 24)
    B = BO.find_modulus(2 * m, Bp + 1)
    params = S.Params.custom(n, B * Bp, B)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(9)
    bkey = o.bootstrap_key(sk, 10, noise=2)
    parent = S.Engine(params)
    parent.upload_key(bkey)
    X, Y = parent.clone(), parent.clone()
    bl = G.Blocker(parent, params)
    try:
        some = np.zeros((4, 2), dtype=np.uint64)
        X.rns2_convert(some, B, Bp, to_pairs=True)
        Y.rns2_convert(some, Bp, B, to_pairs=True)
        work = {e: G.inputs(params, g, 8800 + g) for e, g in ((parent, 3), (X, 5), (Y, 4))}
        parent.set_coalesce(False)
        raw = {e: parent.bootstrap_batch(*work[e], raw=True) for e in (X, Y)}
        assert np.array_equal(raw[X], o.bootstrap_batch(bkey, *work[X], raw=True))
        want = {X: [BO.rns2_from_int(v, B, Bp) for v in _ints(raw[X])],
                Y: [BO.rns2_from_int(v, Bp, B) for v in _ints(raw[Y])]}
        for order in ((parent, X, Y), (X, Y, parent), (Y, parent, X)):
            jobs = [G.Job(e, work[e], rns2=True) for e in order]
            got = dict(zip(order, G.run(parent, bl, jobs, None)))
            # (no composition asserted here; but the three were queued behind the blocker, not three solo calls)
            assert G.LOG[-1]["blocker_outlived_ms"] > 0, G.LOG[-1]
            for e in (X, Y):
                assert isinstance(got[e], np.ndarray), (order.index(e), got[e])
                assert [(int(a), int(b)) for a, b in got[e].reshape(-1, 2)] == want[e], \
                    "clone %s led by %s" % ("X" if e is X else "Y", "parent X Y".split()[[parent, X, Y].index(order[0])])
            err = got[parent]
            assert isinstance(err, S.SgfheError) and err.code == -1 and "no RNS2 moduli" in str(err), \
                ("the ctx without moduli, led by place %d" % order.index(parent), err)
    finally:
        parent.set_coalesce(True)
        bl.close()
        for e in (X, Y, parent):
            e.close()


def test_a_failing_request_keeps_its_error_to_itself(S, oc, exp, gpu_keys):
    """Two requests that cannot be served -- limb pairs from a ctx without RNS2 moduli, and SGFHE_FLAG_RAW_RNS2 without
    SGFHE_FLAG_RAW_MODQ -- queued between plain and raw callers: each reports its own error string on its own ctx
    (sgfhe_last_error_string), and the callers of the same moment get their bytes."""
    if exp.record:
        return
    n = 64
    params, _o, _sk, eng = gpu_keys.engine(n)
    eng.set_random_flatten(False)
    clones = [eng.clone() for _ in range(6)]
    bl = G.Blocker(eng, params)
    try:
        w = [G.inputs(params, 2 + t, 8900 + t) for t in range(6)]
        jobs = [G.Job(clones[0], w[0], rns2=True), G.Job(clones[1], w[1]), G.Job(clones[2], w[2], flags=2),
                G.Job(clones[3], w[3], raw=True), G.Job(clones[4], w[4]), G.Job(clones[5], w[5], raw=True)]
        ref = G.alone(eng, jobs)
        got = G.run(eng, bl, jobs, [[0], [1, 4], [2], [3, 5]])
        for t in (1, 3, 4, 5):
            _same(got[t], ref[t], t)
        _oracle(exp, gpu_keys, n, "live", got[4], jobs[4])
        _oracle(exp, gpu_keys, n, "live", got[5], jobs[5])
        for t, text in ((0, "no RNS2 moduli"), (2, "needs SGFHE_FLAG_RAW_MODQ")):
            assert isinstance(got[t], S.SgfheError) and got[t].code == -1 and text in str(got[t]), (t, got[t])
            assert str(got[t]) == str(ref[t])                 # the message its call gives alone
            assert text in clones[t]._L.sgfhe_last_error_string(clones[t]._h).decode()
        # the failures left their ctxs usable, and touched nobody else's error string
        assert clones[0].bootstrap_batch(*w[0]).tobytes() == eng.bootstrap_batch(*w[0]).tobytes()
        assert "RNS2" not in clones[1]._L.sgfhe_last_error_string(clones[1]._h).decode()
    finally:
        eng.set_coalesce(True)
        bl.close()
        for c in clones:
            c.close()
