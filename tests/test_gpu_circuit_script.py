"""The circuit glue kernels at chosen wire tables (sgfhe_debug_circuit_script): k_circ_split,
k_circ_gather, k_circ_xor3, k_circ_xor3_raw, k_circ_scatter, k_circ_scatter_raw, k_circ_raw_and, k_circ_lift,
k_circ_collect, k_circ_state_load and k_circ_next run as a real run launches them, on ctxs that never had a key: every
bootstrap call and the pack tail are a script, so the words the glue sees are chosen here -- the ends of Z_r and Z_Q, the
wraps of NOT, the ties of ModRed, the borrow of LOW -- and what the gather stages and what the tail would read are
looked at directly.  The expectation is circuit.py's replay with the same script behind its callables
(tests/circuit_script_cases.py); where a case sits on an edge of a numpy helper the words are held to Python integers as
well.  Every comparison is for equality.  Nothing here bootstraps but the two neutrality cases at the end."""

import ctypes

import numpy as np
import pytest

import circuit_script_cases as SC
import ring_cases as RC
import run_error_cases as EC

pytestmark = pytest.mark.gpu

U64 = np.uint64
INVALID = -1
_ENG = {}


def _ctx(S, name):
    """(params, a ctx without a key) of Params(64) or of a ring of tests/ring_cases.py, one per module run."""
    if name not in _ENG:
        p = S.Params(64) if name == "params64" else RC.ring(S, name).params
        _ENG[name] = (p, S.Engine(p))
    return _ENG[name]


def teardown_module(module):
    for _, e in _ENG.values():
        e.close()
    _ENG.clear()


def _where(c, g, inst):
    """(scripted call, rows) of node g in a one-shot run whose every level is one call."""
    for L, nodes in enumerate(c.schedule()):
        if g in nodes:
            assert len(nodes) * inst <= 8192
            k = nodes.index(g)
            return L, slice(k * inst, (k + 1) * inst)
    raise KeyError(g)


def _run(S, eng, p, c, inputs, mode="lwe", data=None, edit=None, seed=1, tables=()):
    """One scripted one-shot run against the replay of the same script.  inputs: the LWE array (mode "lwe") or (a, b)
    (modes "ct": no pack stage, "plain", "direct", "lift").  edit(calls, results): chosen rows over the seeded script.
    Returns (the hook's dict, the recorder, the replay's LWE outputs, the script)."""
    CM = S.circuit
    ct = mode != "lwe"
    count = inputs[0].shape[1] if ct else inputs.shape[1]
    kw = dict(pack=mode in ("plain", "direct", "lift"), direct=mode in ("direct", "lift"), lift=mode == "lift")
    calls = SC.script_calls(c, p.n, count, ct=ct, **kw)
    results = SC.random_script(np.random.default_rng(seed), calls, p.n, p.r, p.Q, tables)
    if edit:
        edit(calls, results)
    got = eng.debug_circuit_script(c, results, inputs, data=data, **kw)
    sc = SC.Script(p, calls, results)
    if mode == "lwe":
        want = CM.replay_levels(c, inputs, p.r, sc.boot, sc.boot_lut, data=data)
    elif mode == "ct":
        split = S.scheme.split_ciphertext_array(inputs[0], inputs[1], p.n, p.r).reshape(c.n_inputs, count * p.n, p.n + 1)
        want = CM.replay_levels(c, split, p.r, sc.boot, sc.boot_lut, data=data)
    elif mode == "plain":
        _, want = CM.replay_ct(c, inputs[0], inputs[1], p, sc.boot, sc.pack, sc.boot_lut, data=data)
    else:
        _, want = CM.replay_ct_direct(c, inputs[0], inputs[1], p, sc.boot_raw, sc.tail, lift=mode == "lift",
                                      boot_lut_raw=sc.boot_lut_raw, data=data)
    assert got["calls"] == calls
    diff = SC.same_logs(got, sc, SC.gate3_rows(c, count * p.n if ct else count))
    assert diff is None, diff
    assert np.array_equal(got["out"], want)
    if kw["pack"]:
        assert got["tail_in"].shape[0] == 1 and np.array_equal(got["tail_in"][0], sc.tail_array())
    else:
        assert got["tail_in"] is None
    return got, sc, want, results


def _edge_inputs(p, wires, inst, edge_wire=0):
    """fill() with the rows of one wire cycling through 0, 1, Dr - 1, Dr, r / 2, r - 1 in every word position."""
    x = SC.fill(wires, inst, p.n, p.r)
    x[edge_wire] = SC.cycle_words((inst, p.n + 1), np.array(SC.EDGE_WORDS(p.r), dtype=U64), stride=1)
    x[edge_wire, :6] = np.array(SC.EDGE_WORDS(p.r), dtype=U64)[:, None]        # and whole rows of each
    return x


# ---- 1. every reference form through one gather ------------------------------------------------------------------------

def _reference_forms(S, G):
    C = S.Circuit
    c = C(3, group=G)
    x, y, z = c.inputs
    nodes = [c.gate(x, y), c.gate(~x, y), c.gate(x, ~y), c.gate(~x, ~y), c.gate(C.FALSE, x), c.gate(x, C.TRUE),
             c.gate(C.TRUE, ~x), c.gate(~x, C.FALSE), c.gate(z, z)]
    if G > 1:
        for d in sorted({1, -1, G - 1, -(G - 1)}):
            nodes.append(c.gate(x.lane(d), ~x.lane(d)))                      # a negated out-of-group read fills with TRUE
            nodes.append(c.gate(~y.lane(-d), x.lane(d)))
        holes = [t if t % 2 else S.circuit.ROUTE_FALSE for t in range(G)]
        nodes.append(c.gate(x.route(holes), ~x.route(holes)))
        nodes.append(c.gate(c.bcast(x, G - 1), ~c.bcast(y, 0)))
        nodes.append(c.gate(c.reverse(x), ~c.reverse(y)))
        nodes.append(c.gate(c.rot(x, 1), ~c.swap(y, 1)))
    c.output(*[w for nd in nodes for w in nd] + [~x.lane(G - 1) if G > 1 else ~x, x, ~z, C.TRUE])
    return c


@pytest.mark.parametrize("G", [1, 6])
def test_every_reference_form_through_one_gather(S, G):
    """Params(64): rows of 65 words, so every wave of the gather straddles rows.  One level, every node a classic pair:
    the four NOT patterns, the constant in either position, lane shifts +-1 and +-(G - 1) plain and negated, a route with
    fills plain and negated, bcast, reverse, rot and swap, at G = 1 and at G = 6 (no power of two); the source rows hold
    0, 1, Dr - 1, Dr, r / 2 and r - 1.  The staged rows are the replay's inputs of the call, word for word."""
    p, eng = _ctx(S, "params64")
    c = _reference_forms(S, G)
    inst = 12
    inputs = _edge_inputs(p, 3, inst)
    got, sc, want, _ = _run(S, eng, p, c, inputs, seed=10 + G)
    assert len(got["calls"]) == 1 and got["calls"][0] == (len(c.gates) * inst, False)
    r, Dr, n = p.r, p.r // 4, p.n
    st = got["staged"][0].astype(object)
    # Python integers: node 1 = (~x, y), node 6 = (TRUE, ~x): NOT of the edge rows, -0 = 0 and Dr - b with its wrap
    for t in range(inst):
        assert list(st[1 * inst + t, 0]) == SC.not_r_int([int(v) for v in inputs[0, t]], r, Dr)
        assert list(st[6 * inst + t, 0]) == [0] * n + [Dr] and list(st[6 * inst + t, 1]) == list(st[1 * inst + t, 0])
    if G > 1:
        k = 9                                                  # the first shifted node: d = -(G - 1), (x.lane(d), ~x.lane(d))
        for t in range(inst):
            inside = t % G == G - 1
            assert list(st[k * inst + t, 0]) == ([int(v) for v in inputs[0, t - (G - 1)]] if inside else [0] * (n + 1))
            assert list(st[k * inst + t, 1]) == (SC.not_r_int([int(v) for v in inputs[0, t - (G - 1)]], r, Dr) if inside
                                                 else [0] * n + [Dr])          # TRUE at b only
        last = got["out"][3 * len(c.gates)].astype(object)                   # ~x.lane(G - 1) through k_circ_collect
        for t in range(inst):
            assert list(last[t]) == (SC.not_r_int([int(v) for v in inputs[0, t + G - 1]], r, Dr) if t % G == 0 else [0] * n + [Dr])


# ---- 2. sum nodes ----------------------------------------------------------------------------------------------------------

def _sum_circuit(S, p):
    """Level 1: one classic node per distinct word of the sum tables (and 64 for the all-(r - 1) terms), whose scripted
    AND rows hold that word throughout; level 2: the sum nodes of sum_cases and a gate3 on filled wires."""
    c = S.Circuit(3)
    x, y, z = c.inputs
    ones = [c.gate(x, y)[0] for _ in range(64)]
    words = {}
    for _, terms, _ in SC.sum_cases(p.r)[2:]:
        for _, v in terms:
            if v not in words:
                words[v] = c.gate(x, z)[0]
    fillers = [c.gate(y, z) for _ in range(3)]
    sums = []
    for label, terms, u in SC.sum_cases(p.r):
        if len(terms) == 64:
            sums.append(c.sum_node([(w, ones[i]) for i, (w, _) in enumerate(terms)]))
        else:
            sums.append(c.sum_node([(w, words[v]) for w, v in terms]))
    sums.append(c.gate3(fillers[0][0], ~fillers[1][1], fillers[2][2]))
    return c, ones, words, sums


@pytest.mark.parametrize("mode", ["lwe", "direct"])
def test_sum_nodes_at_the_ends_of_the_sum_and_low_with_a_borrow(S, mode):
    """64 terms of weight +2 and of -2 on words of r - 1, mixes that give U = 0 and U = r - 1 exactly, a gate3 on filled
    rows; then LOW = U - 2 HI with scripted HI words 0, r / 2 and r - 1 against U = 0 and U = r - 1 -- through k_circ_xor3,
    and in a direct run, where an output names a HI wire, through k_circ_xor3_raw on un-reduced HI rows."""
    p, eng = _ctx(S, "params64")
    r, n, Q = p.r, p.n, p.Q
    c, ones, words, sums = _sum_circuit(S, p)
    outs = [w for s in sums for w in s]
    c.output(*outs)
    blocks = 1
    inst = n * blocks if mode != "lwe" else 6
    cases = SC.sum_cases(r)
    his = [0, r // 2, r - 1, 1, r // 4, r - 2]

    def edit(calls, results):
        for w in ones:
            k, rows = _where(c, (w.id - 3) // 3, inst)
            results[k][rows, 0] = r - 1
        for v, w in words.items():
            k, rows = _where(c, (w.id - 3) // 3, inst)
            results[k][rows, 0] = v
        for s in sums:                                        # HI rows: word e of instance t cycles through `his`
            k, rows = _where(c, (s[0].id - 3) // 3, inst)
            hi = SC.cycle_words((inst, n + 1), np.array(his, dtype=U64), stride=1)
            if calls[k][1]:                                   # un-reduced: the least residue ModRed takes to that word
                res = [SC.modred_boundaries(Q, r, [(int(v) - 1) % r])[0][1] % Q for v in his]
                assert [SC.modred_int(v, Q, r) for v in res] == his
                results[k][rows, 0] = SC.from_int(np.array(res, dtype=object)[(np.arange(inst * (n + 1))) % len(his)]
                                                  .reshape(inst, n + 1))
            else:
                results[k][rows, 0] = hi

    if mode == "lwe":
        inputs = SC.fill(3, inst, n, r)
    else:
        inputs = (SC.fill(3, blocks, n - 1, r), SC.fill(3, blocks, n - 1, r, p=(5, 3, 7)))
    got, sc, want, results = _run(S, eng, p, c, inputs, mode=mode, edit=edit, seed=21)
    assert got["calls"][1][1] == (mode == "direct")
    k, _ = _where(c, (sums[0][0].id - 3) // 3, inst)
    st = got["staged"][k].astype(object)
    hi_words = SC.cycle_words((inst, n + 1), np.array(his, dtype=object), stride=1)
    for i, (label, terms, u) in enumerate(cases):
        rows = slice(i * inst, (i + 1) * inst)
        assert (st[rows, 0] == u).all() and (st[rows, 1] == 0).all(), label     # (U, FALSE), every word the table's U
        low = got["out"][3 * i + 2].astype(object)
        assert (low == (u - 2 * hi_words) % r).all(), label                     # Python integers, the borrow included
        assert (got["out"][3 * i].astype(object) == hi_words).all(), label
    seen = {(u, h) for _, _, u in cases for h in his}
    assert {(0, r // 2), (0, r - 1), (r - 1, r - 1), (r - 1, 0)} <= seen


# ---- 3. LUT and data nodes ---------------------------------------------------------------------------------------------------

def test_lut_not_at_every_codeword_and_every_table_of_a_plane(S):
    """Level 1: three fans, whose scripted rows give wires at Dr, Dr / 2 and Dr / 4 with b = 0, the codeword and the
    codeword + 1 in turn, and a classic node.  Level 2: LUT nodes with NOT at each of the three positions, the constant
    tables 0x00, 0xFF and 0x96, a data node whose plane holds every byte 0 .. 255 across 256 instances, and a classic
    node in the same call.  The descriptor word of every row; NOT against Python integers."""
    p, eng = _ctx(S, "params64")
    r, n, Dr = p.r, p.n, p.r // 4
    C = S.Circuit
    c = C(2, planes=1)
    x, y = c.inputs
    f = [c.fan(x), c.fan(y), c.fan(x)]
    g = c.gate(x, y)
    luts = [c.lut(0x96, ~f[0][2], f[1][1], f[2][0]), c.lut(0x00, f[0][2], ~f[1][1], f[2][0]),
            c.lut(0xFF, f[0][2], f[1][1], ~f[2][0]), c.lut(0x96, ~f[0][2], ~f[1][1], ~f[2][0]),
            c.lut_data(0, f[1][2], C.TRUE, ~g[1])]
    mixed = c.gate(g[0], ~g[2])
    c.output(*[nd[0] for nd in luts] + list(mixed))
    inst = 256
    data = np.arange(256, dtype=np.uint8)[None, :]

    def edit(calls, results):
        for fan in range(3):                                  # wire w of a fan carries scale w: codeword Dr >> w
            for w in range(3):
                cw = Dr >> w
                results[0][fan * inst:(fan + 1) * inst, w, n] = np.array([0, cw, cw + 1], dtype=U64)[np.arange(inst) % 3]
                results[0][fan * inst:(fan + 1) * inst, w, :3] = np.array([0, 1, r - 1], dtype=U64)

    got, sc, want, results = _run(S, eng, p, c, SC.fill(2, inst, n, r), data=data, edit=edit, seed=31)
    assert [rows for rows, _ in got["calls"]] == [4 * inst, 6 * inst]
    lut = got["lut"][1]
    tabs = [0x96, 0x00, 0xFF, 0x96]
    for i, t in enumerate(tabs):
        assert (lut[i * inst:(i + 1) * inst] == (0x100 | t)).all()
    assert (lut[4 * inst:5 * inst] == (0x100 | np.arange(256))).all()         # the data plane: every byte, at its own instance
    assert (lut[5 * inst:] == 0).all() and (got["lut"][0][:3 * inst] == 0x1F0).all() and (got["lut"][0][3 * inst:] == 0).all()
    # the LUT row is (X0 + X1 + X2, FALSE), NOT at position i taken at Dr >> (2 - i): Python integers
    st = got["staged"][1].astype(object)
    res0 = results[0].astype(object)
    for t in range(inst):
        x0, x1, x2 = (list(res0[0 * inst + t, 2]), list(res0[1 * inst + t, 1]), list(res0[2 * inst + t, 0]))
        nots = [SC.not_r_int(x0, r, Dr // 4), SC.not_r_int(x1, r, Dr // 2), SC.not_r_int(x2, r, Dr)]
        for i, neg in enumerate([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]):
            terms = [nots[j] if neg[j] else (x0, x1, x2)[j] for j in range(3)]
            assert list(st[i * inst + t, 0]) == [sum(v) % r for v in zip(*terms)] and not st[i * inst + t, 1].any()
    b0 = res0[0:inst, 2, n]
    assert {0, Dr // 4, Dr // 4 + 1} == set(b0) and {0, Dr, Dr + 1} == set(res0[2 * inst:3 * inst, 0, n])


# ---- 4. scatter ---------------------------------------------------------------------------------------------------------------

def test_scatter_leaves_unread_and_pruned_rows_out_and_moves_nothing_else(S):
    """Three levels on the m128 ring (n = 16), some gate outputs unread, one node pruned; the same nodes again with every
    wire an output: both runs take the same script (the pruned node has no rows in either), and every wire of the second
    is the replay's -- so a row scattered to a wrong slot, or an unread one scattered at all, shows."""
    p, eng = _ctx(S, "m128")
    n, r = p.n, p.r

    def build(every):
        c = S.Circuit(3)
        x, y, z = c.inputs
        a, b = c.gate(x, y), c.gate(y, ~z)
        dead = c.gate(x, z)                                   # pruned: nothing reads it
        d = c.gate(a[0], b[2])
        e = c.gate3(a[1], d[0], ~z)
        f = c.gate(e[2], d[1])
        del dead
        live = [a, b, d, e, f]
        c.output(*([w for nd in live for w in nd] + [x, y, z] if every else [f[0], ~e[1], b[2]]))
        return c
    inst = 37
    inputs = _edge_inputs(p, 3, inst)
    got1, sc1, _, res1 = _run(S, eng, p, build(False), inputs, seed=41)
    got2, sc2, _, res2 = _run(S, eng, p, build(True), inputs, seed=41)
    assert got1["calls"] == got2["calls"] and all(np.array_equal(u, v) for u, v in zip(res1, res2))
    assert np.array_equal(got1["out"][0], got2["out"][12]) and np.array_equal(got1["out"][2], got2["out"][5])
    assert all(np.array_equal(u, v) for u, v in zip(got1["staged"], got2["staged"]))


def test_a_level_wider_than_a_call_with_routes_across_the_boundary(S):
    """G = 48 over 2736 instances, three nodes: 8208 rows, so call 0 ends inside node 2 at lane 32 of the last group.  The
    next level reads node 2 through swap(32) and a rotation by 17 -- rows of the other call -- and node 0 reversed
    (tests/test_gpu_circuit_routes.py runs this plan on 11 000 bootstraps; here it costs none)."""
    p, eng = _ctx(S, "params64")
    G, inst = 48, 2736
    c = S.Circuit(2, group=G)
    x, y = c.inputs
    n0, n1, n2 = c.gate(x, y), c.gate(~x, y), c.gate(x, ~c.rot(y, 5))
    top = c.gate(c.swap(n2[2], 32), ~c.rot(n2[1], 17))
    c.output(top[0], top[2], c.reverse(n0[0]), ~c.swap(n2[0], 32), n1[1], n2[1])
    got, sc, want, _ = _run(S, eng, p, c, SC.fill(2, inst, p.n, p.r), seed=43)
    assert got["calls"] == [(8192, False), (16, False), (inst, False)]


# ---- 5. un-reduced calls -------------------------------------------------------------------------------------------------------

def _direct_circuit(S):
    c = S.Circuit(2)
    x, y = c.inputs
    g0, g1, g2 = c.gate(x, y), c.gate(~x, y), c.gate(x, ~y)
    h = c.gate(g0[0], ~g1[1])                                 # level 2 reads what the raw scatter reduced
    # one gate wire twice, negated and not; gates of different nodes of one call; an input (refreshed); level 2
    c.output(g0[0], ~g0[0], g1[1], ~g2[2], x, h[1], ~h[1], g2[0])
    return c, (g0, g1, g2, h)


@pytest.mark.parametrize("ring", ["tiny", "wide"])
def test_unreduced_calls_at_the_ends_of_zq_and_the_ties_of_modred(S, ring):
    """A direct run on `tiny` (Q < 2^30) and on `wide` (Q ~ 2^92: the high words carry).  The scripted residues cycle
    through 0, 1, Q - 1, 2 DQ_tilde and its two neighbours, 2^64 - 1 and 2^64 where Q allows, and for several k -- 0 and
    r - 1 among them -- the least residue ModRed rounds to k + 1 and the one below it; whole rows put a = 0 beside
    b = 2 DQ_tilde and b = 2 DQ_tilde + 1.  The wire table against ModRed, the raw table rows as they are and under NOT,
    in Python integers."""
    p, eng = _ctx(S, ring)
    n, r, Q, DQ = p.n, p.r, p.Q, p.DQ_tilde
    c, (g0, g1, g2, h) = _direct_circuit(S)
    table = SC.residue_table(Q, r, DQ)
    T = (2 * DQ) % Q
    blocks = 2
    inst = blocks * n

    def edit(calls, results):
        assert calls[0] == (3 * inst, True) and calls[1] == (inst, True)
        # node g0, gate 0: a = 0 throughout, b = 2 DQ, 2 DQ + 1, 2 DQ - 1, 0, Q - 1 in turn
        bs = [T, (T + 1) % Q, (T - 1) % Q, 0, Q - 1]
        rows = np.zeros((inst, n + 1), dtype=object)
        rows[:, n] = np.array(bs, dtype=object)[np.arange(inst) % len(bs)]
        rows[inst // 2:, :n] = np.array(table, dtype=object)[(np.arange((inst - inst // 2) * n) * 5) % len(table)].reshape(-1, n)
        results[0][0:inst, 0] = SC.from_int(rows)

    a = SC.fill(2, blocks, n - 1, r)
    b = SC.fill(2, blocks, n - 1, r, p=(3, 7, 9))
    got, sc, want, results = _run(S, eng, p, c, (a, b), mode="direct", edit=edit, seed=51, tables=table)
    res = SC.to_int(results[0])
    assert set(table) <= set(res.reshape(-1))
    # the wire table: ModRed of every residue of the call, as the outputs show it (g0 AND, g1 OR, g2 AND)
    for o, (rank, gate) in {0: (0, 0), 2: (1, 1), 7: (2, 0)}.items():
        exp = np.array([[SC.modred_int(int(v), Q, r) for v in row] for row in res[rank * inst:(rank + 1) * inst, gate]], dtype=U64)
        assert np.array_equal(got["out"][o], exp), o
    # the raw table: rows as they are, and under NOT
    tail = SC.to_int(got["tail_in"][0]).reshape(c.n_outputs, inst, n + 1)
    assert (tail[0] == res[0:inst, 0]).all() and (tail[2] == res[inst:2 * inst, 1]).all() and (tail[7] == res[2 * inst:, 0]).all()
    for t in range(inst):
        assert list(tail[1][t]) == SC.not_q_int([int(v) for v in res[t, 0]], Q, DQ)
        assert list(tail[3][t]) == SC.not_q_int([int(v) for v in res[2 * inst + t, 2]], Q, DQ)
    assert list(tail[1][0]) == [0] * (n + 1) and list(tail[1][1]) == [0] * n + [Q - 1]       # a = 0 stays 0; the wrap of b
    res1 = SC.to_int(results[1])
    for t in range(inst):
        assert list(tail[6][t]) == SC.not_q_int([int(v) for v in res1[t, 1]], Q, DQ)
    # the input is refreshed: gate 0 of the scripted refresh call, through k_circ_raw_and, and every staged row (TRUE, bit)
    assert got["calls"][2] == (blocks * n, True)
    assert (tail[4] == SC.to_int(results[2])[:, 0]).all()
    st = got["staged"][2]
    assert not st[:, 0, :n].any() and (st[:, 0, n] == r // 4).all()


def test_a_raw_call_split_inside_a_producing_node(S):
    """tiny, 342 blocks of n = 8: 2736 instances, three nodes in one level, every output a gate row -- two un-reduced
    calls of 8192 and 16 rows, the boundary inside node 2, whose direct output takes rows from both (two job ranges)."""
    p, eng = _ctx(S, "tiny")
    n, r = p.n, p.r
    c = S.Circuit(2)
    x, y = c.inputs
    g = [c.gate(x, y), c.gate(~x, y), c.gate(x, ~y)]
    c.output(g[0][0], ~g[2][1], g[1][2], g[2][1])
    blocks = 342
    table = SC.residue_table(p.Q, r, p.DQ_tilde)
    a, b = SC.fill(2, blocks, n - 1, r), SC.fill(2, blocks, n - 1, r, p=(3, 7, 9))
    got, sc, want, _ = _run(S, eng, p, c, (a, b), mode="direct", seed=53, tables=table)
    assert got["calls"] == [(8192, True), (16, True)]


# ---- 6. the pack stage ----------------------------------------------------------------------------------------------------------

def test_lift_of_every_kind_of_output_equals_the_integer_lift(S):
    """SGFHE_CIRCUIT_PACK_LIFT at Params(64), G = 8: outputs that are an input, both constants, a negated wire, a shifted
    and a routed wire and an XOR3 wire, the wires' words covering 0, 1, Dr, r / 2 and r - 1: tail_in is
    (x Q + r / 2) // r of the LWE outputs, in Python integers.  No call in the pack stage."""
    p, eng = _ctx(S, "params64")
    n, r, Q = p.n, p.r, p.Q
    C = S.Circuit
    c = C(2, group=8)
    x, y = c.inputs
    g = c.gate(x, y)
    t = c.gate3(g[0], ~g[1], x)
    c.output(x, C.TRUE, C.FALSE, ~y, g[0].lane(-3), ~c.reverse(g[2]), t[2])
    edge = np.array([0, 1, r // 4, r // 2, r - 1], dtype=U64)

    def edit(calls, results):
        results[0][:, :, :] = SC.cycle_words(results[0].shape, edge, stride=3)

    a, b = SC.fill(2, 1, n - 1, r), SC.fill(2, 1, n - 1, r, p=(3, 7, 9))
    got, sc, want, _ = _run(S, eng, p, c, (a, b), mode="lift", edit=edit, seed=61)
    assert got["calls"] == [(n, False), (n, False)]                           # nothing direct, nothing refreshed
    tail = SC.to_int(got["tail_in"][0]).reshape(c.n_outputs, n, n + 1)
    for o in range(7):
        exp = [[SC.lift_int(int(v), Q, r) for v in row] for row in got["out"][o]]
        assert tail[o].tolist() == exp, o
    assert set(edge.tolist()) <= set(got["out"][4].reshape(-1).tolist()) and tail[1][0].tolist() == [0] * n + [SC.lift_int(r // 4, Q, r)]
    assert not tail[2].any()


@pytest.mark.parametrize("mode", ["plain", "direct"])
def test_pack_groups_of_more_than_128_ciphertexts(S, mode):
    """3 outputs x 66 blocks at n = 64: 198 ciphertexts, two pack groups and a short last one.  Plain: every ciphertext
    is refreshed, the tail reads gate 0 of the refresh result at its stride.  Direct: outputs 0 and 2 are gate rows,
    output 1 (an input) is refreshed -- a run at the end of group 0 and one at the start of group 1, so the run ranks and
    the offsets of k_circ_raw_and differ.  Every staged row of a refresh call is (TRUE, output): a1 = 0, b1 = Dr."""
    p, eng = _ctx(S, "params64")
    n, r = p.n, p.r
    c = S.Circuit(2)
    x, y = c.inputs
    g = c.gate(x, y)
    c.output(g[0], ~y, ~g[1])
    blocks = 66
    a, b = SC.fill(2, blocks, n - 1, r), SC.fill(2, blocks, n - 1, r, p=(3, 7, 9))
    got, sc, want, _ = _run(S, eng, p, c, (a, b), mode=mode, seed=63)
    if mode == "plain":
        assert got["calls"] == [(blocks * n, False), (128 * n, True), (70 * n, True)]
    else:
        assert got["calls"] == [(blocks * n, True), (62 * n, True), (4 * n, True)]
    for k in (1, 2):
        st = got["staged"][k]
        assert not st[:, 0, :n].any() and (st[:, 0, n] == r // 4).all()
    # output 1 (~y) is what input 2 of the refresh rows holds: all of call 1 (direct), or behind output 0's rows (plain)
    first = got["staged"][1][:, 1] if mode == "direct" else got["staged"][1][66 * n:128 * n, 1]
    assert np.array_equal(first, want[1][:62 * n])


def test_direct_and_refreshed_ciphertexts_alternate(S):
    """One block, seven outputs that alternate between a gate row and a refreshed wire: every run of a group is one
    ciphertext long, its rank differs from its position, on the m128 ring."""
    p, eng = _ctx(S, "m128")
    n, r = p.n, p.r
    c = S.Circuit(2)
    x, y = c.inputs
    g, h = c.gate(x, y), c.gate(~x, y)
    c.output(g[0], x, ~h[1], S.Circuit.TRUE, h[2], ~y, g[1])
    a, b = SC.fill(2, 1, n - 1, r), SC.fill(2, 1, n - 1, r, p=(3, 7, 9))
    got, sc, want, _ = _run(S, eng, p, c, (a, b), mode="direct", seed=65, tables=SC.residue_table(p.Q, r, p.DQ_tilde))
    assert got["calls"] == [(2 * n, True), (3 * n, True)]


# ---- 7. split --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("big", [False, True], ids=["N=n", "N=m"])
def test_split_reads_the_negative_side_where_it_should(S, big):
    """The ciphertext form with N = n and with N = m, two blocks, three inputs of which nothing reads one.  The a-words
    at the positions the negative side reads hold 0, 1 and r - 1 (-0 stays 0); at N = m the words at indices >= n are
    read for d < 0 and never for d >= 0.  Against scheme.split_ciphertext_array and against Python-integer extract."""
    p, eng = _ctx(S, "params64")
    n, r, m = p.n, p.r, p.m
    N = m if big else n
    c = S.Circuit(3)
    x, y, z = c.inputs
    g = c.gate(x, ~z)
    c.output(x, ~z, g[0], z)
    blocks = 2
    a = SC.fill(3, blocks, N - 1, r)
    b = SC.fill(3, blocks, N - 1, r, p=(3, 7, 9))
    a[:, :, N - 6:N] = np.array([0, 1, r - 1, r - 1, 1, 0], dtype=U64)         # a[N + d] for d = -6 .. -1
    a[:, :, 0:3] = np.array([0, 1, r - 1], dtype=U64)
    if big:
        a[:, :, n:m - 6] = (a[:, :, n:m - 6] + U64(977)) % U64(r)             # never read for d >= 0
    got, sc, want, _ = _run(S, eng, p, c, (a, b), mode="ct", seed=71)
    split = S.scheme.split_ciphertext_array(a, b, n, r).reshape(3, blocks * n, n + 1)
    assert np.array_equal(got["out"][0], split[0]) and np.array_equal(got["out"][3], split[2])
    ai, bi = a.astype(object), b.astype(object)
    for w, o in ((0, 0), (2, 3)):
        for t in range(blocks):
            for i in range(n):
                exp = [int(ai[w, t, i - j]) if i >= j else (-int(ai[w, t, N + i - j])) % r for j in range(n)] + [int(bi[w, t, i])]
                assert got["out"][o][t * n + i].tolist() == exp, (w, t, i)
    assert got["out"][0][0].tolist()[1:7] == [0, r - 1, 1, 1, r - 1, 0]          # bit 0: -a[N - 1], .., -a[N - 6]


# ---- 8. stepped --------------------------------------------------------------------------------------------------------------------

def test_three_steps_with_registers_at_every_scale(S):
    """Registers at scales 0, 1 and 2 with negated next states (NOT at Dr >> scale), two registers that swap, one that
    takes itself rotated, one that nothing reads; emit masks; three steps with another script per step, the call order
    going on across steps; state_out the very array state_in is.  Against replay_steps."""
    p, eng = _ctx(S, "params64")
    n, r, Dr = p.n, p.r, p.r // 4
    C = S.Circuit
    G = 4
    c = C(8, group=G, registers=7, reg_scales=[0, 1, 2, 0, 0, 0, 0])
    r0, r1, r2, sa, sb, rot, idle = c.registers
    (x,) = c.stream_inputs
    f = c.lut(0x96, r2, r1, r0)
    g = c.gate(x, ~sa)
    c.output(g[0], ~f[0], c.rot(rot, 1), sb)
    c.next_state(~f[0], ~f[1], ~f[2], ~sb, sa.lane(1), ~c.rot(rot, 1), ~idle)
    inst, steps = 8, 3
    CM = S.circuit
    for emit in (None, [0, 1, 0], [1, 0, 1], [0, 0, 0]):
        calls = SC.script_calls(c, n, inst, steps=steps, emit=emit)
        assert len(calls) == 3 and all(rows == 2 * inst for rows, _ in calls)
        results = SC.random_script(np.random.default_rng(81), calls, n, r, p.Q)
        for k in range(steps):                                # the LUT node's wires: b = 0, codeword, codeword + 1 at each scale
            for w in range(3):
                results[k][:inst, w, n] = np.array([0, Dr >> w, (Dr >> w) + 1, r - 1], dtype=U64)[(np.arange(inst) + k) % 4]
        state = SC.fill(7, inst, n, r, p=(13, 7, 3))
        state[1, :, n] = np.array([0, Dr // 2, Dr // 2 + 1, 5], dtype=U64)[np.arange(inst) % 4]
        state[2, :, n] = np.array([0, Dr // 4, Dr // 4 + 1, 5], dtype=U64)[np.arange(inst) % 4]
        stream = SC.fill(steps, inst, n, r, p=(29, 5, 9)).reshape(steps, 1, inst, n + 1)
        sc = SC.Script(p, calls, results)
        want_out, want_state = CM.replay_steps(c, state, stream, r, sc.boot, sc.boot_lut, emit=emit)
        mine = np.ascontiguousarray(state.copy())
        got = eng.debug_circuit_script(c, results, stream, state=mine, stepped=True, emit=emit, state_in_place=True)
        assert got["state"] is mine and got["calls"] == calls
        assert SC.same_logs(got, sc) is None, SC.same_logs(got, sc)
        assert np.array_equal(got["out"], want_out) and got["out"].shape[0] == (3 if emit is None else sum(emit))
        assert np.array_equal(mine, want_state)
        # Python integers: the register nothing reads is negated three times at Dr; scale 1 and 2 from the last script
        assert mine[6, 0].tolist() == SC.not_r_int([int(v) for v in state[6, 0]], r, Dr)
        for t in range(inst):
            for w, reg in ((1, 1), (2, 2)):
                assert mine[reg, t].tolist() == SC.not_r_int([int(v) for v in results[2][t, w]], r, Dr >> w)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------

def _raw_call(eng, c, form, count, inputs, out, results, staged, lut, tail=None, steps=0):
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return eng._L.sgfhe_debug_circuit_script(eng._h, c.handle() if c is not None else None, form, count, steps, None, None,
                                             P(inputs), None, 0, None, None, P(out), None, 0, P(results), P(staged), P(lut), P(tail))


def test_refusals_come_before_anything_is_written(S):
    p, eng = _ctx(S, "params64")
    n, r = p.n, p.r
    c = S.Circuit(2)
    x, y = c.inputs
    c.output(c.gate(x, y)[0])
    inst = 8
    inputs = SC.fill(2, inst, n, r)
    good = np.random.default_rng(91).integers(0, r, size=(inst, 3, n + 1), dtype=U64)
    SENT = U64(EC.SENTINEL)

    def fresh():
        return (np.full((1, inst, n + 1), SENT), np.full((inst, 2, n + 1), SENT), np.full(inst, 0xA5A5A5A5, dtype=np.uint32))

    def refused(code, why, *args, **kw):
        out, staged, lut = fresh()
        rc = _raw_call(eng, kw.pop("circ", c), kw.pop("form", 0), inst, inputs, out, kw.pop("results", good),
                       staged if kw.pop("staged", True) else None, lut, **kw)
        msg = eng._L.sgfhe_last_error_string(eng._h).decode()
        assert rc == code and why in msg, (rc, msg)
        assert (out == SENT).all() and (staged == SENT).all() and (lut == 0xA5A5A5A5).all()

    refused(INVALID, "NULL script", results=None)
    refused(INVALID, "NULL script", staged=False)
    bad = good.copy()
    bad[inst - 1, 2, n] = r
    refused(INVALID, "a scripted word is not below r", results=bad)
    refused(INVALID, "no probe, no device form", form=S.engine.SCRIPT_PROBE)
    refused(INVALID, "no probe, no device form", form=S.engine.SCRIPT_DEVICE)
    refused(INVALID, "unknown form bits", form=16)
    refused(INVALID, "NULL circuit", circ=None)
    fam = S.Circuit(2)
    (lead, sib) = fam.lut_multi([0x96, 0xE8], S.Circuit.FALSE, S.Circuit.FALSE, fam.inputs[0])
    fam.output(lead[0], sib[0])
    refused(INVALID, "a plan with a live LUT sibling", circ=fam)
    # a residue = Q, in the un-reduced call of a direct run
    d = S.Circuit(2)
    d.output(d.gate(*d.inputs)[0])
    a, b = SC.fill(2, 1, n - 1, r), SC.fill(2, 1, n - 1, r, p=(3, 7, 9))
    res = SC.random_script(np.random.default_rng(92), [(n, True)], n, r, p.Q)
    res[0][n - 1, 2, n] = SC.from_int(p.Q)
    with pytest.raises(S.SgfheError) as e:
        eng.debug_circuit_script(d, res, (a, b), direct=True)
    assert e.value.code == INVALID and "a scripted residue is not below Q" in str(e.value)
    res[0][n - 1, 2, n] = SC.from_int(p.Q - 1)
    eng.debug_circuit_script(d, res, (a, b), direct=True)
    # the hook after all that: the bytes of a run on a fresh ctx
    _run(S, eng, p, c, inputs, seed=93)


@pytest.mark.parametrize("entry", ["sgfhe_circuit_run_data", "sgfhe_circuit_run_ct_data", "sgfhe_circuit_run_steps",
                                   "sgfhe_circuit_run_steps_ct"])
def test_every_refusal_of_the_ordinary_check_unchanged(S, entry):
    """The cases of tests/run_error_cases.py through the hook in the form of `entry`, on a ctx without a key: the code and
    the message the entry itself gives (tests/golden/circuit_run_errors.json) -- but that a missing key is no defect here:
    such a case has the verdict of its other defect, or runs.  Nothing is written."""
    import json
    import os
    p, eng = _ctx(S, "params64")
    with open(os.path.join(os.path.dirname(__file__), "golden", "circuit_run_errors.json")) as fh:
        golden = json.load(fh)["cases"]
    plans = EC.make_plans(S)
    E = EC.ENTRIES[entry]
    form = (S.engine.SCRIPT_CT if E.ct else 0) | (S.engine.SCRIPT_STEPPED if E.stepped else 0)
    n_cases = 0
    for case in EC.cases_of(entry):
        if not case.key:
            continue                                          # (a missing key is no defect here)
        if case.name.startswith("out_w_without_v"):
            continue                                          # the hook has tail_in where the entries have out_w and out_v
        call = EC.Call(entry, case, p)
        A = call.arrays
        P = lambda name: call._pointer(name)
        script = np.zeros(64 * 3 * (p.n + 1) * 2, dtype=U64)
        staged = np.full(64 * 2 * (p.n + 1), U64(EC.SENTINEL))
        lut = np.full(64, 0xA5A5A5A5, dtype=np.uint32)
        tail = np.full(1, U64(EC.SENTINEL)) if "out_w" in A else None     # (never reached: every case ends before a run)
        h = None if "circ" in case.null else plans[case.plan].handle()
        vp = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
        rc = eng._L.sgfhe_debug_circuit_script(
            eng._h, h, form, case.count, case.steps, P("state_a") if E.ct else P("state_in"), P("state_b"),
            P("in_a") if E.ct else P("in"), P("in_b"), p.n + (case.N == "n+1"), P("data"), P("emit"), P("out"), P("state_out"),
            case.flags, vp(script), vp(staged), vp(lut), vp(tail))
        msg = eng._L.sgfhe_last_error_string(eng._h).decode()
        want_code, want_msg = golden[EC.case_id(entry, case)]
        assert rc == want_code and (rc == 0 or msg == want_msg), (case.name, rc, msg)
        assert call.untouched() and (staged == U64(EC.SENTINEL)).all() and (lut == 0xA5A5A5A5).all(), case.name
        n_cases += 1
    assert n_cases >= 8


# ---- 10. neutrality ------------------------------------------------------------------------------------------------------------------

def test_a_scripted_run_leaves_the_draw_stream_and_last_call_alone(S, gpu_keys):
    """Randomised mode on a keyed ctx: bootstrap_batch after a scripted run (with a pack stage) has the bytes of the same
    call made without it."""
    p, o, sk, eng = gpu_keys.engine(64)
    n, r = p.n, p.r
    key = bytes(range(7, 39))
    c, _ = _direct_circuit(S)
    rows = SC.fill(4, 16, n, r)
    a, b = SC.fill(2, 1, n - 1, r), SC.fill(2, 1, n - 1, r, p=(3, 7, 9))
    try:
        eng.set_random_flatten(True, key)
        first = eng.bootstrap_batch(rows[0, :, :n], rows[0, :, n], rows[1, :, :n], rows[1, :, n])
        plain = eng.bootstrap_batch(rows[2, :, :n], rows[2, :, n], rows[3, :, :n], rows[3, :, n])
        eng.set_random_flatten(True, key)
        again = eng.bootstrap_batch(rows[0, :, :n], rows[0, :, n], rows[1, :, :n], rows[1, :, n])
        for mode in ("direct", "plain", "lift"):
            _run(S, eng, p, c, (a, b), mode=mode, seed=101)
        after = eng.bootstrap_batch(rows[2, :, :n], rows[2, :, n], rows[3, :, :n], rows[3, :, n])
        assert np.array_equal(first, again) and np.array_equal(plain, after)
    finally:
        eng.set_random_flatten(False, 0)


def test_a_real_direct_run_equals_the_scripted_run_fed_its_own_calls(S, gpu_keys):
    """One real circuit_run_ct (direct) at Params(64) against the scripted run whose script is that run's own call
    results, obtained by replay_ct_direct through bootstrap_batch on a clone: the same LWE outputs, and the hook's
    tail_in is what the replay hands its tail.  This ties the hook to the real path."""
    p, o, sk, eng = gpu_keys.engine(64)
    CM = S.circuit
    n, r = p.n, p.r
    c, _ = _direct_circuit(S)
    rng = np.random.default_rng(111)
    a = rng.integers(0, r, size=(2, 1, n), dtype=U64)
    b = rng.integers(0, r, size=(2, 1, n), dtype=U64)
    ref = eng.clone()
    bare = S.Engine(p)
    try:
        calls = SC.script_calls(c, n, 1, ct=True, pack=True, direct=True)
        raws, groups = [], []

        def boot_raw(call, a1, b1, a2, b2):
            raws.append(ref.bootstrap_batch(a1, b1, a2, b2, raw=True))
            return raws[-1]

        def tail(call, group):
            groups.append(np.array(group))
            return ref.pack_lwe_modq(np.ascontiguousarray(group))
        (w, v), lwe = CM.replay_ct_direct(c, a, b, p, boot_raw, tail)
        (gw, gv), glwe = eng.circuit_run_ct(c, a, b, lwe=True, direct=True)
        assert np.array_equal(glwe, lwe) and np.array_equal(gw, w) and np.array_equal(gv, v)
        assert [(len(x), True) for x in raws] == calls
        got = bare.debug_circuit_script(c, raws, (a, b), direct=True)
        assert np.array_equal(got["out"], glwe)
        assert np.array_equal(got["tail_in"][0], np.concatenate(groups))
    finally:
        ref.close()
        bare.close()
