"""TEST INFRASTRUCTURE: the scripted circuit run (sgfhe_debug_circuit_script, Engine.debug_circuit_script) -- its call
layout restated from Circuit.schedule() and CALL_ROWS, the recorder that puts one script behind the callables of
circuit.py's replay functions, and the tables of edge operands with their Python-integer arithmetic
(tests/test_gpu_circuit_script.py runs them on the device, tests/test_circuit_script_host.py checks the tables and the
layout without one).

A script is one array per scripted call, in the run's call order: per step the level calls, then -- an emitted step of a
run that packs -- the refresh call of every pack group that has one.  A call is [rows][3][n + 1] words of Z_r, or, where
the real run leaves it un-reduced, [rows][3][n + 1][2] residues mod Q as {lo, hi}."""

import numpy as np

U64 = np.uint64


def _cm():
    from sgfhe_jl_amd import circuit
    return circuit


# ---- Python integers: what the numpy helpers of circuit.py are held to ------------------------------------------------

def modred_int(x, Q, r):
    """ModRed: round-half-up(x r / Q) mod r."""
    return ((2 * x * r + Q) // (2 * Q)) % r


def lift_int(x, Q, r):
    return (x * Q + r // 2) // r


def not_q_int(row, Q, DQ_tilde):
    """NOT of one un-reduced LWE (a list of n + 1 integers) over Z_Q."""
    return [(-a) % Q for a in row[:-1]] + [(2 * DQ_tilde - row[-1]) % Q]


def not_r_int(row, r, one):
    return [(-a) % r for a in row[:-1]] + [(one - row[-1]) % r]


def to_int(res):
    """[..., 2] uint64 {lo, hi} -> an object array of Python integers."""
    res = np.asarray(res, dtype=U64)
    return res[..., 0].astype(object) + (res[..., 1].astype(object) << 64)


def from_int(values):
    """Python integers (any nesting) -> [..., 2] uint64 {lo, hi}."""
    v = np.asarray(values, dtype=object)
    flat = [int(x) for x in v.reshape(-1)]
    return np.array([[x & 0xFFFFFFFFFFFFFFFF, x >> 64] for x in flat], dtype=U64).reshape(v.shape + (2,))


# ---- the case tables -----------------------------------------------------------------------------------------------------

def modred_boundaries(Q, r, ks=None):
    """[(label, residue, ModRed of it)]: for every k the least residue that ModRed rounds to k + 1 (mod r) and the one
    below it, which rounds to k."""
    ks = (0, 1, r // 4 - 1, r // 4, r // 2 - 1, r // 2, r - 2, r - 1) if ks is None else ks
    out = []
    for k in ks:
        x = -(-Q * (2 * k + 1) // (2 * r))          # ceil(Q (2 k + 1) / (2 r)): 2 x r + Q >= 2 Q (k + 1) first holds here
        out.append(("first of %d" % ((k + 1) % r), x, (k + 1) % r))
        out.append(("last of %d" % k, x - 1, k))
    return out


def residue_edges(Q, DQ_tilde):
    """[(label, residue)]: the ends of Z_Q, the wrap of NOT's b word, and the carry between the two 64-bit words."""
    T = (2 * DQ_tilde) % Q
    out = [("0", 0), ("1", 1), ("Q-1", Q - 1), ("2DQ-1", (T - 1) % Q), ("2DQ", T), ("2DQ+1", (T + 1) % Q)]
    for label, x in (("2^64-1", (1 << 64) - 1), ("2^64", 1 << 64)):
        if x < Q:
            out.append((label, x))
    return out


def residue_table(Q, r, DQ_tilde):
    """Every residue of residue_edges and modred_boundaries, in that order: the words a scripted un-reduced row cycles
    through."""
    return [x for _, x in residue_edges(Q, DQ_tilde)] + [x for _, x, _ in modred_boundaries(Q, r)]


def sum_cases(r):
    """[(label, [(weight, word of every term's LWE)], U)]: the sums of a sum node over words chosen so that U = the sum
    of weight * word mod r hits the named value."""
    return [
        ("64 x +2 on r-1", [(2, r - 1)] * 64, (-128) % r),
        ("64 x -2 on r-1", [(-2, r - 1)] * 64, 128 % r),
        ("U = 0", [(2, r // 2), (1, r - 1), (1, 1), (-1, r // 4), (1, r // 4), (-2, 0)], 0),
        ("U = r-1", [(2, r // 2), (1, r - 1), (-1, 1), (1, 1), (-2, r // 2), (2, r // 2)], r - 1),
        ("U = r-1 of one", [(-1, 1)], r - 1),
    ]


EDGE_WORDS = lambda r: (0, 1, r // 4 - 1, r // 4, r // 2, r - 1)     # 0, 1, Dr - 1, Dr, r / 2, r - 1


def fill(wires, instances, n, r, p=(37, 11, 5), wire0=0):
    """[wires][instances][n + 1]: word e of instance t of wire w is p1 (wire0 + w) + p2 t + p3 e mod r, odd multipliers:
    a misplaced row or word shows."""
    w, t, e = np.ogrid[:wires, :instances, :n + 1]
    return ((p[0] * (w + wire0) + p[1] * t + p[2] * e) % r).astype(U64)


def cycle_words(shape, table, stride=1, start=0):
    """An array of `shape` whose flat entry i is table[(start + stride i) mod len(table)]."""
    table = np.asarray(table)
    i = (start + stride * np.arange(int(np.prod(shape)))) % len(table)
    return table[i].reshape(tuple(shape) + table.shape[1:])


# ---- the call layout, restated -------------------------------------------------------------------------------------------

def is_direct(circuit, o):
    """Output o names a gate row over Z_Q (replay_ct_direct's rule)."""
    cm = _cm()
    i = circuit.outputs[o] & ~cm.NOT_BIT & 0xFFFFFFFF
    if i == cm.FALSE_ID or i < circuit.n_inputs or circuit.output_shifts[o] != 0:
        return False
    g, w = divmod(i - circuit.n_inputs, 3)
    if g in circuit.gate_tables:
        return False
    return not (w == 2 and circuit.kind(g) != "classic")


def script_calls(circuit, n, count, ct=False, steps=None, emit=None, pack=False, direct=False, lift=False):
    """[(rows, un-reduced)] of the scripted calls of a run, as the replay functions count calls: every level of
    Circuit.schedule() in calls of CALL_ROWS rows; then, per emitted step of a run that packs, one call per pack group of
    pack_calls(n) ciphertexts that refreshes any."""
    cm = _cm()
    inst = count * n if ct else count
    pack = bool(ct and (pack or direct or lift))
    direct = pack and bool(direct or lift)
    lift = direct and bool(lift)
    named = {}                                       # node -> a direct output names one of its gate rows
    for o in range(circuit.n_outputs):
        if is_direct(circuit, o):
            named[((circuit.outputs[o] & ~cm.NOT_BIT & 0xFFFFFFFF) - circuit.n_inputs) // 3] = True
    out = []
    for s in range(1 if steps is None else steps):
        for nodes in circuit.schedule():
            rows = len(nodes) * inst
            for r0 in range(0, rows, cm.CALL_ROWS):
                cnt = min(cm.CALL_ROWS, rows - r0)
                held = nodes[r0 // inst:(r0 + cnt - 1) // inst + 1]
                out.append((cnt, direct and any(g in named for g in held)))
        if steps is not None and emit is not None and not emit[s]:
            continue
        n_ct, cpc = (circuit.n_outputs * count, cm.pack_calls(n)) if pack else (0, 1)
        for q0 in range(0, n_ct, cpc):
            qs = range(q0, min(q0 + cpc, n_ct))
            fresh = [q for q in qs if not (direct and is_direct(circuit, q // count))]
            if fresh and not lift:
                out.append((len(fresh) * n, True))
    return out


def random_script(rng, calls, n, r, Q, tables=()):
    """One result array per call: uniform words, or for an un-reduced call residues cycling through `tables` (a list of
    Python integers) mixed with uniform ones."""
    out = []
    for k, (rows, raw) in enumerate(calls):
        if not raw:
            out.append(rng.integers(0, r, size=(rows, 3, n + 1), dtype=np.uint64))
            continue
        vals = np.array([int(x) for x in rng.integers(0, 1 << 62, size=rows * 3 * (n + 1))], dtype=object)
        vals = (vals * vals + vals) % Q
        if len(tables):
            at = np.arange(len(vals)) % 3 != 2       # two words of three from the table, its entries in turn
            vals[at] = np.array(list(tables), dtype=object)[(np.arange(int(at.sum())) + 7 * k) % len(tables)]
        out.append(from_int(vals.reshape(rows, 3, n + 1)))
    return out


# ---- the recorder ----------------------------------------------------------------------------------------------------------

class Script:
    """One script behind the callables of replay_levels, replay_steps, replay_ct and replay_ct_direct: boot, boot_lut,
    boot_raw, boot_lut_raw return the scripted rows of (call, rows) and record the inputs they were given; pack and tail
    record the group they were given.  The replay counts a tail as a call of its own, the script does not: scripted
    calls are numbered in the order the replay first names them."""

    def __init__(self, params, calls, results):
        self.p, self.calls, self.results = params, calls, [np.asarray(x, dtype=U64) for x in results]
        n = params.n
        self.staged = [np.zeros((rows, 2, n + 1), dtype=U64) for rows, _ in calls]
        self.lut = [np.zeros(rows, dtype=np.uint32) for rows, _ in calls]
        self.tail_in = []
        self.index = {}

    def _k(self, call):
        return self.index.setdefault(call, len(self.index))

    def _log(self, k, sel, a1, b1, a2, b2):
        n = self.p.n
        self.staged[k][sel, 0, :n], self.staged[k][sel, 0, n] = a1, b1
        self.staged[k][sel, 1, :n], self.staged[k][sel, 1, n] = a2, b2

    def words(self, k):
        """call k as the wire table sees it: words of Z_r"""
        cm = _cm()
        return cm.modred_words(self.results[k], self.p.Q, self.p.r) if self.calls[k][1] else self.results[k]

    def residues(self, k):
        """call k over Z_Q; a reduced call as the lift of its words (ModRed of which is the words: no direct output
        names such a call's rows)"""
        cm = _cm()
        return self.results[k] if self.calls[k][1] else cm.lift_words(self.results[k], self.p.Q, self.p.r)

    def boot(self, call, a1, b1, a2, b2):
        k = self._k(call)
        self._log(k, slice(None), a1, b1, a2, b2)
        return self.words(k)

    def boot_lut(self, call, a, b, tables, idx):
        k = self._k(call)
        self._log(k, idx, a, b, 0, 0)
        self.lut[k][idx] = 0x100 | np.asarray(tables, dtype=np.uint32)
        return self.words(k)[idx]

    def boot_raw(self, call, a1, b1, a2, b2):
        k = self._k(call)
        self._log(k, slice(None), a1, b1, a2, b2)
        return self.residues(k)

    def boot_lut_raw(self, call, a, b, tables, idx):
        k = self._k(call)
        self._log(k, idx, a, b, 0, 0)
        self.lut[k][idx] = 0x100 | np.asarray(tables, dtype=np.uint32)
        return self.residues(k)[idx]

    def pack(self, call, a, b):
        """The plain pack stage of replay_ct: the group's refresh call, (TRUE, bit) per row, and its tail on gate 0."""
        k = self._k(call)
        n, m, r = self.p.n, self.p.m, self.p.r
        cnt = a.shape[0]
        self._log(k, slice(None), 0, r // 4, a.reshape(cnt * n, n), b.reshape(cnt * n))
        self.tail_in.append(self.results[k][:, 0].reshape(cnt, n, n + 1, 2))
        return np.zeros((cnt, m), dtype=U64), np.zeros((cnt, m), dtype=U64)

    def tail(self, call, group):
        self.tail_in.append(np.array(group, dtype=U64))
        z = np.zeros((len(group), self.p.m), dtype=U64)
        return z, z.copy()

    def tail_array(self):
        return np.concatenate(self.tail_in) if self.tail_in else None


def gate3_rows(circuit, instances):
    """{call: rows} of the three-input nodes of a one-shot run whose every level is one call.  replay_levels hands such
    a node to `boot` as the pair (x + y, z); the gather stages it as the sum node of three unit weights it is, (x + y + z,
    FALSE) -- the bootstrap adds its two inputs first, so both are the same call.  same_logs folds the replay's pair."""
    out = {}
    for k, nodes in enumerate(circuit.schedule()):
        rows = [np.arange(i * instances, (i + 1) * instances) for i, g in enumerate(nodes) if circuit.kind(g) == "gate3"]
        if rows:
            out[k] = np.concatenate(rows)
    return out


def same_logs(got, script, fold=None):
    """The hook's logs against the recorder's, word for word; returns the first difference as text, None for none.
    fold: {call: rows} whose recorded pair (u, v) is expected as (u + v mod r, 0) (gate3_rows)."""
    if len(script.index) != len(script.calls):
        return "the replay made %d scripted calls, the layout has %d" % (len(script.index), len(script.calls))
    for k, rows in (fold or {}).items():
        st = script.staged[k]
        st[rows, 0] = (st[rows, 0] + st[rows, 1]) & U64(script.p.r - 1)
        st[rows, 1] = 0
    for k, (rows, raw) in enumerate(script.calls):
        if not np.array_equal(got["staged"][k], script.staged[k]):
            bad = np.argwhere(got["staged"][k] != script.staged[k])[0]
            return "call %d: staged row %d input %d word %d is %d, the replay gave %d" % (
                (k,) + tuple(bad) + (got["staged"][k][tuple(bad)], script.staged[k][tuple(bad)]))
        if not np.array_equal(got["lut"][k], script.lut[k]):
            bad = int(np.flatnonzero(got["lut"][k] != script.lut[k])[0])
            return "call %d: descriptor word %d is %#x, the replay gave %#x" % (k, bad, got["lut"][k][bad], script.lut[k][bad])
    return None
