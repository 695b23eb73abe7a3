"""Gate circuits evaluated on the device level by level over many independent instances
(sgfhe_circuit_* of include/sgfhe_hip.h).

A circuit is a list of nodes; every node is one bootstrap(bkey, rng, x, y) (src/fhe.jl:608-621) and
yields AND, OR and XOR together.  NOT is linear (enc_trivial(true) - w, src/fhe.jl:221-223,669-670), so
NAND, NOR, XNOR, ANDNOT ... cost their one bootstrap.  Running one circuit over many instances makes
every level a wide batch: the throughput form of the engine.

    c = Circuit(2)
    x, y = c.inputs
    and_, or_, xor_ = c.gate(x, y)
    c.output(~and_, xor_)                         # NAND, XOR
    outs = evaluate_circuit(bkey, None, c, [[e_x0, e_x1], [e_y0, e_y1]])   # 2 instances

Lanes (sgfhe_circuit_create_lanes).  Circuit(n_inputs, group=G) partitions the instances into consecutive groups
of G lanes, and `w.lane(d)` is the reference that reads lane t + d of `w` at lane t -- FALSE where t + d leaves the
group, before `~`.  A shift costs no bootstrap.  In the ciphertext form a ciphertext of n bits then holds n / G
words of G bits, and gates can be wired between bits of one ciphertext: packed_adder(16) adds n / 16 pairs of 16-bit
numbers per ciphertext pair.

Three-input nodes (sgfhe_circuit_create3).  `gate3(x, y, z)` is ONE bootstrap, on (x + y, z): the rotation by the
phase of the sum of three bits yields MAJ (the AND row) and "one or two true" (the OR row), and XOR3 =
x + y + z - 2 MAJ over Z_r is linear.  `full_adder(x, y, c)` is therefore one node and ripple_adder(16) sixteen.
XOR3 is not bootstrapped and carries its inputs' errors on: see the noise rule in include/sgfhe_hip.h.

Weighted-sum nodes (sgfhe_circuit_create_w).  `sum_node([(w, wire), ...])` is ONE bootstrap on U = sum of w X mod r,
w in {-2, -1, 1, 2}, up to 64 terms: with s = the sum of w x mod 4 its wires are HI (s in {2, 3}), MID (s in {1, 2}) and
the linear LOW = U - 2 HI (s mod 2).  All weights 2 make HI the XOR of all terms -- `xor(*wires)` -- so a GF(2)-linear
map is one node per output bit (gf2_matvec, crc16_ccitt); one term of weight 1 makes MID a refresh (`refresh(w)`).  A
weight of 2 doubles the wire's error: use it on bootstrapped wires, not on fresh encryptions.

LUT nodes (sgfhe_circuit_create_lut).  `lut(table, x0, x1, x2)` is ONE bootstrap that evaluates ANY function of three
bits: bit s of `table` is its value at s = x0 + 2 x1 + 4 x2.  The three inputs arrive at the codewords Dr/4, Dr/2 and Dr,
so a wire has a SCALE (0: Dr, 1: Dr/2, 2: Dr/4) and position i of a LUT node reads scale 2 - i; the node returns its bit
at all three scales, (f, f_half, f_quarter), so any LUT output can feed any position of a later LUT node.  Everything
else -- inputs, the wires of the other nodes, outputs -- is scale 0; `fan(x)` brings a scale-0 wire to all three scales
in one bootstrap.  The inputs of a LUT node must be bootstrapped wires (refresh, then fan): the sum of their errors has
to stay below Dr/8 (the noise rule in include/sgfhe_hip.h).

LUT families (sgfhe_circuit_create_lut_multi).  `lut_multi(tables, x0, x1, x2)` evaluates up to 256 functions of the
same three wires on ONE bootstrap: the k-loop does not depend on the table, so every further table costs one more
extraction of the same accumulator and no row.  The first table is the family's leader, a LUT node; each other is a
SIBLING, a node with no inputs of its own whose three wires are numbered like any node's.  `shannon(c, tables, xs)`
builds any functions of k >= 3 wires this way: all cofactors on (x0, x1, x2) are one family, a mux tree follows.

Data planes (sgfhe_circuit_create_data).  Circuit(n_inputs, planes=P) has P planes of run-time data: a run takes
`data`, uint8 [P][instances], and `lut_data(p, x0, x1, x2)` is the LUT node whose truth table at instance t is
data[p][t] -- public data that differs from instance to instance, in one bootstrap, with no extra rows or inputs.
`Circuit.plane(p)` among the tables of lut_multi makes that member a data table.  `lookup(c, xs)` with
`lookup_data(tables, k)` is shannon with per-instance tables: T_t[x] for a different public table T_t at every instance.
The table never enters the k-loop: rows, calls, draws and the noise rule are those of the constant-table circuit.

Registers (sgfhe_circuit_create_seq).  Circuit(n_inputs, registers=R) makes the first R inputs REGISTERS and the others
STREAM inputs; `next_state(*wires)` names the wire every register takes after a step, and a STEPPED run
(evaluate_circuit_steps, Engine.circuit_run_steps) evaluates the circuit `steps` times in one queued run with the
registers fed back on the device: stream inputs, planes and outputs are per step, and memory does not grow with the
steps.  serial_adder() adds numbers of any width with one bootstrap per bit; crc16_stream(8) is the CRC-16 of a message
of any length, a byte per step.  Feed a register from a bootstrapped wire (a gate row, HI / MID, a LUT wire): an XOR3 /
LOW wire or a stream input fed back adds its error every step.

Lane routes (sgfhe_circuit_create_routed).  `w.route(table)` is the reference that reads lane table[t] of `w` at lane t
of every group -- any public lane map, FALSE where table[t] is ROUTE_FALSE, before `~` -- at no bootstrap, no row and no
draw: Circuit.rot (rotation inside a word), Circuit.swap (partner t ^ k), Circuit.bcast (one lane to the whole group),
Circuit.reverse.  Routes compose with each other and with lane shifts and are normalised, so the identity is nothing
and a pure shift is the shift.  Terms, outputs and next states may be routed; a routed output is refreshed or lifted,
never direct.  bitonic_sort(width, G) sorts the G numbers of every group with routes alone between its nodes.

Lane masks (sgfhe_circuit_create_masked).  `lanes=` on gate / gate3 / sum_node / xor / refresh / lut / lut_data / fan /
full_adder makes the node bootstrap only the lanes named -- an iterable of lane indices or a 0/1 sequence of length G.
On the other lanes every wire of the node is the constant FALSE (TRUE under `~`), wherever it is read, and the node takes
no row there: a run's cost is its rows, `Circuit.info()["rows_per_group"]`.  All lanes is no mask at all.  lane_reduce
folds a wire over the lanes of a word in G - 1 rows a group, packed_equal(width) compares two packed words in
2 width - 1, and bitonic_sort(width, G, masked=True) evaluates every comparator chain at its decision lanes only.  An
output naming a masked node's wire is refreshed or lifted, never direct; a LUT node that leads siblings takes no mask.
"""

import ctypes

import numpy as np

from . import _lib
from .scheme import LWE, RLWE, Ciphertext, EncryptedBit, PackedCiphertext, _set_flatten_mode, split_ciphertext_array

FALSE_ID = 0x7FFFFFFF      # SGFHE_CIRCUIT_FALSE
NONE_ID = 0x7FFFFFFE       # SGFHE_CIRCUIT_NONE: the third reference of a two-input node
NOT_BIT = 0x80000000       # SGFHE_CIRCUIT_NOT
MAX_TERMS = 64             # SGFHE_CIRCUIT_MAX_TERMS
MAX_PLANES = 65536         # SGFHE_CIRCUIT_MAX_PLANES
MAX_ROUTES = 65536         # SGFHE_CIRCUIT_MAX_ROUTES
MAX_MASKS = 65536          # SGFHE_CIRCUIT_MAX_MASKS
ROUTE_FALSE = -1           # SGFHE_CIRCUIT_ROUTE_FALSE: entry of a route table, the constant FALSE at that lane
LUT_MAX_TABLES = 256       # SGFHE_LUT_MAX_TABLES
CALL_ROWS = 8192           # SGFHE_CIRCUIT_CALL_ROWS


def shift_table(d, group):
    """The lane shift d as a route table of `group` entries: lane t reads lane t + d, ROUTE_FALSE where that leaves
    the group."""
    return tuple(t + d if 0 <= t + d < group else ROUTE_FALSE for t in range(group))


def normal_route(table):
    """A route table in its normal form, (shift, route): the identity is (0, None), a table that is a pure shift with
    FALSE fill (shift_table) is (d, None) with the smallest such |d|, anything else (0, the table as a tuple)."""
    table = tuple(int(x) for x in table)
    G = len(table)
    if any(not ROUTE_FALSE <= x < G for x in table):
        raise ValueError("a route entry is a lane 0 .. %d or ROUTE_FALSE (-1): %r" % (G - 1, table))
    for d in sorted(range(-G + 1, G), key=abs):
        if table == shift_table(d, G):
            return d, None
    return 0, table


class Wire:
    """A wire reference: the wire id, plus bit 31 for its negation (`~w`), and a lane shift (`w.lane(d)`) or a lane
    route (`w.route(table)`), never both."""

    __slots__ = ("ref", "shift", "table")

    def __init__(self, ref, shift=0, table=None):
        self.ref = int(ref) & 0xFFFFFFFF
        self.shift = int(shift)
        self.table = None if table is None else tuple(int(x) for x in table)

    def __invert__(self):
        return Wire(self.ref ^ NOT_BIT, self.shift, self.table)

    def lane(self, d):
        """The reference that reads lane t + d of this one at lane t of every group (FALSE, or TRUE for a negated
        reference, where t + d leaves the group).  Shifts add up; on a routed reference the shift composes with the
        route as route(shift_table(d, G)) does."""
        if self.table is not None:
            return self.route(shift_table(int(d), len(self.table)))
        return Wire(self.ref, self.shift + int(d))

    def route(self, table):
        """The reference that reads lane table[t] of this one at lane t of every group of G = len(table) lanes, and
        FALSE (TRUE for a negated reference) where table[t] is ROUTE_FALSE.  It costs no bootstrap.  It composes with an
        earlier shift or route -- w.route(A).route(B) reads w at lane A[B[t]], and a fill stays a fill -- and the result
        is normalised (normal_route): the identity is no route at all, a pure shift with FALSE fill is that shift."""
        table = tuple(int(x) for x in table)
        G = len(table)
        if G < 1 or any(not ROUTE_FALSE <= x < G for x in table):
            raise ValueError("a route entry is a lane 0 .. %d or ROUTE_FALSE (-1): %r" % (G - 1, table))
        if self.table is not None and len(self.table) != G:
            raise ValueError("route: a table of %d lanes on a reference routed over %d" % (G, len(self.table)))
        if self.table is None and abs(self.shift) >= G:
            raise ValueError("route: the reference's lane shift %+d is outside a group of %d" % (self.shift, G))
        inner = self.table if self.table is not None else shift_table(self.shift, G)
        shift, table = normal_route(ROUTE_FALSE if x < 0 else inner[x] for x in table)
        return Wire(self.ref, shift, table)

    @property
    def lanes(self):
        """How the reference reads its group: the route table (a tuple) of a routed reference, the lane shift otherwise."""
        return self.shift if self.table is None else self.table

    @property
    def id(self):
        return self.ref & ~NOT_BIT & 0xFFFFFFFF

    @property
    def negated(self):
        return bool(self.ref & NOT_BIT)

    def __eq__(self, other):
        return isinstance(other, Wire) and other.ref == self.ref and other.shift == self.shift and other.table == self.table

    def __hash__(self):
        return hash((self.ref, self.shift, self.table))

    def __repr__(self):
        return "%sWire(%s)%s" % ("~" if self.negated else "", "FALSE" if self.id == FALSE_ID else self.id,
                                 ".route(%r)" % (self.table,) if self.table is not None else
                                 (".lane(%+d)" % self.shift if self.shift else ""))


class Plane:
    """A data plane among the tables of Circuit.lut_multi: that member's truth table is run-time data (Circuit.plane)."""

    __slots__ = ("index",)

    def __init__(self, index):
        self.index = int(index)

    def __repr__(self):
        return "Plane(%d)" % self.index


class Circuit:
    """Builder of a gate circuit: `n_inputs` input wires, nodes added with gate(), outputs set with
    output().  `group`: the lane group size (instances form consecutive groups of `group` lanes; a reference may be
    shifted by |d| < group lanes, Wire.lane).  The C plan (sgfhe_circuit_create, sgfhe_circuit_create_lanes when
    the group is above 1, sgfhe_circuit_create3 when a gate3 exists, sgfhe_circuit_create_w when a sum node exists that
    is no three-input node, sgfhe_circuit_create_lut when a LUT node exists, sgfhe_circuit_create_lut_multi when a LUT
    sibling exists, sgfhe_circuit_create_data when the circuit has planes, sgfhe_circuit_create_seq when it has
    registers, sgfhe_circuit_create_routed when a reference carries a lane route that normalisation leaves a route,
    sgfhe_circuit_create_masked when a node carries a lane mask that normalisation leaves a mask) is made on first use
    and freed with the object.
    `planes`: the number of data planes a run brings (lut_data, Circuit.plane), uint8 [planes][instances].
    `registers`: the first `registers` inputs are registers (`c.registers`), fed back by a stepped run from the wires
    given to next_state; the others are the stream inputs (`c.stream_inputs`).  `reg_scales`: the scale of every
    register (0, 1 or 2; default all 0): a register of scale 2 can be read at position 0 of a LUT node."""

    FALSE = Wire(FALSE_ID)
    TRUE = Wire(FALSE_ID | NOT_BIT)

    def __init__(self, n_inputs, group=1, planes=0, registers=0, reg_scales=None):
        if not 0 <= int(n_inputs) < FALSE_ID:
            raise ValueError("n_inputs out of range")
        if not 1 <= int(group) <= 0xFFFFFFFF:
            raise ValueError("group out of range")
        if not 0 <= int(planes) <= MAX_PLANES:
            raise ValueError("planes out of range (at most %d)" % MAX_PLANES)
        if not 0 <= int(registers) <= int(n_inputs):
            raise ValueError("registers out of range (at most n_inputs)")
        reg_scales = [0] * int(registers) if reg_scales is None else [int(k) for k in reg_scales]
        if len(reg_scales) != int(registers) or any(k not in (0, 1, 2) for k in reg_scales):
            raise ValueError("reg_scales: one scale 0, 1 or 2 per register")
        self.n_inputs = int(n_inputs)
        self.group = int(group)
        self.planes = int(planes)
        self.n_regs = int(registers)
        self.reg_scales = reg_scales
        self.inputs = [Wire(i) for i in range(self.n_inputs)]
        self.registers = self.inputs[:self.n_regs]
        self.stream_inputs = self.inputs[self.n_regs:]
        self.next_refs = [FALSE_ID] * self.n_regs   # [ref]: the next state of every register (next_state); FALSE until set
        self.next_shifts = [0] * self.n_regs
        self.gates = []            # [(x ref, y ref)], or (x ref, y ref, z ref) for a three-input node
        self.outputs = []          # [ref]
        self.gate_shifts = []      # [(x lane shift, y lane shift)] or (x, y, z lane shift), beside gates; in place of a
                                   # shift, here and in output_shifts and next_shifts, a routed reference has its
                                   # route table (a tuple of `group` entries: Wire.lanes)
        self.gate_weights = {}     # node -> (weight, ...) beside its references: the sum nodes (sum_node)
        self.gate_tables = {}      # node -> truth table: the LUT nodes (lut) and their siblings (lut_multi)
        self.gate_leader = {}      # sibling -> its leader, a LUT node: no inputs of its own, () in gates and gate_shifts
        self.gate_planes = {}      # data LUT node or data sibling -> its plane (its entry of gate_tables is None)
        self.output_shifts = []    # [lane shift], beside outputs
        self.gate_masks = {}       # node -> its lane mask, a tuple of `group` entries 0 / 1 (never all 1: that is no mask)
        self._plan = None
        self._L = None

    def scale(self, w):
        """The scale of a wire: 0 (codeword Dr) but for wires +1 and +2 of a LUT node (1: Dr/2, 2: Dr/4); None for the
        constant, which fits every scale; a register has the scale it was given (Circuit(reg_scales=...))."""
        if w.id == FALSE_ID:
            return None
        if w.id < self.n_inputs:
            return self.reg_scales[w.id] if w.id < self.n_regs else 0
        g, k = divmod(w.id - self.n_inputs, 3)
        return k if g in self.gate_tables else 0

    def _ref(self, w, scale=0):
        if not isinstance(w, Wire):
            raise TypeError("expected a Wire, got %r" % (w,))
        if abs(w.shift) >= self.group:
            raise ValueError("%r: a lane shift must be inside the group of %d" % (w, self.group))
        if w.table is not None and len(w.table) != self.group:
            raise ValueError("%r: a route table has one entry per lane of the group of %d" % (w, self.group))
        if self.scale(w) not in (None, scale):
            raise ValueError("%r has scale %d where scale %d is read (Circuit.lut, Circuit.fan)" % (w, self.scale(w), scale))
        return w.ref

    def _lanes(self, lanes):
        """`lanes=` of a node in its normal form: None for no mask (None, or every lane), else a tuple of `group` entries
        0 / 1.  lanes: an iterable of lane indices, or a 0/1 sequence of length `group` (a sequence of length `group`
        whose entries are all 0 or 1 is read as 0/1 flags; in a group of 1 or 2 lanes write the flags)."""
        if lanes is None:
            return None
        lanes = [int(l) for l in lanes]
        G = self.group
        if G == 1:
            raise ValueError("lanes=: a circuit without lane groups (group 1) takes no lane mask")
        if len(lanes) == G and all(l in (0, 1) for l in lanes):
            mask = tuple(lanes)
        else:
            if any(not 0 <= l < G for l in lanes):
                raise ValueError("lanes=: a lane is 0 .. %d: %r" % (G - 1, lanes))
            mask = tuple(1 if t in set(lanes) else 0 for t in range(G))
        if not any(mask):
            raise ValueError("lanes=: a node must take a row on at least one lane")
        return None if all(mask) else mask

    @property
    def mask_tables(self):
        """The distinct lane masks of the circuit's nodes, in order of first use."""
        seen = {}
        for g in sorted(self.gate_masks):
            seen.setdefault(self.gate_masks[g], len(seen))
        return list(seen)

    def lanes_on(self, g):
        """The lanes node g takes a row on, ascending (all of them without a mask)."""
        m = self.gate_masks.get(g)
        return list(range(self.group)) if m is None else [t for t in range(self.group) if m[t]]

    def gate(self, x, y, lanes=None):
        """One node: bootstrap(x, y).  Returns its (AND, OR, XOR) wires.  lanes: the lanes the node bootstraps (all);
        its wires are FALSE on the others (the module's text on lane masks)."""
        mask = self._lanes(lanes)
        self.gates.append((self._ref(x), self._ref(y)))
        self.gate_shifts.append((x.lanes, y.lanes))
        if mask is not None:
            self.gate_masks[len(self.gates) - 1] = mask
        self._invalidate()
        base = self.n_inputs + 3 * (len(self.gates) - 1)
        return Wire(base), Wire(base + 1), Wire(base + 2)

    def gate3(self, x, y, z, lanes=None):
        """One three-input node: bootstrap(x + y, z).  Returns its (MAJ, ONE_OR_TWO, XOR3) wires: the majority, "one
        or two of the inputs true" (not all equal), and the parity x + y + z - 2 MAJ over Z_r, which is linear and
        carries the errors of x, y and z on.  lanes: as in gate."""
        mask = self._lanes(lanes)
        self.gates.append((self._ref(x), self._ref(y), self._ref(z)))
        self.gate_shifts.append((x.lanes, y.lanes, z.lanes))
        if mask is not None:
            self.gate_masks[len(self.gates) - 1] = mask
        self._invalidate()
        base = self.n_inputs + 3 * (len(self.gates) - 1)
        return Wire(base), Wire(base + 1), Wire(base + 2)

    def sum_node(self, terms, lanes=None):
        """One weighted-sum node: ONE bootstrap on U = the sum of weight * wire over Z_r.  terms: [(weight, wire), ...],
        1 to 64 of them, weight in {-2, -1, 1, 2}; TRUE with weight c adds the constant c Dr.  Returns its (HI, MID, LOW)
        wires: with s = the sum of weight * bit mod 4, HI is s in {2, 3} (the AND row), MID is s in {1, 2} (the OR row)
        and LOW is s mod 2 = U - 2 HI over Z_r, which is linear and carries the error of the sum on.  Weights (1, 1, 1)
        are gate3.  lanes: as in gate."""
        terms = list(terms)
        mask = self._lanes(lanes)
        if not 1 <= len(terms) <= MAX_TERMS:
            raise ValueError("a sum node has 1 to %d terms" % MAX_TERMS)
        if any(int(w) not in (-2, -1, 1, 2) for w, _ in terms):
            raise ValueError("the weights of a sum node are -2, -1, 1 or 2")
        self.gates.append(tuple(self._ref(x) for _, x in terms))
        self.gate_shifts.append(tuple(x.lanes for _, x in terms))
        self.gate_weights[len(self.gates) - 1] = tuple(int(w) for w, _ in terms)
        if mask is not None:
            self.gate_masks[len(self.gates) - 1] = mask
        self._invalidate()
        base = self.n_inputs + 3 * (len(self.gates) - 1)
        return Wire(base), Wire(base + 1), Wire(base + 2)

    def lut(self, table, x0, x1, x2, lanes=None):
        """One LUT node: ONE bootstrap for any function of three bits.  Bit s of `table` (0 .. 255) is the value at
        s = x0 + 2 x1 + 4 x2.  x0 must be a wire of scale 2 (codeword Dr/4), x1 of scale 1, x2 of scale 0, or the
        constants.  Returns (f, f_half, f_quarter): the result at scales 0, 1 and 2.  lanes: as in gate (FALSE at all three
        scales on the other lanes); not for the leader of lut_multi."""
        if not 0 <= int(table) < 256:
            raise ValueError("a LUT node's table has 8 entries: 0 .. 255")
        mask = self._lanes(lanes)
        self.gates.append((self._ref(x0, 2), self._ref(x1, 1), self._ref(x2, 0)))
        self.gate_shifts.append((x0.lanes, x1.lanes, x2.lanes))
        self.gate_tables[len(self.gates) - 1] = int(table)
        if mask is not None:
            self.gate_masks[len(self.gates) - 1] = mask
        self._invalidate()
        base = self.n_inputs + 3 * (len(self.gates) - 1)
        return Wire(base), Wire(base + 1), Wire(base + 2)

    @staticmethod
    def plane(p):
        """Plane p as a member of lut_multi's tables: the member's truth table at instance t is data[p][t]."""
        return Plane(p)

    def _plane(self, p):
        if not 0 <= int(p) < self.planes:
            raise ValueError("plane %r is not below the circuit's %d planes (Circuit(planes=...))" % (p, self.planes))
        return int(p)

    def lut_data(self, plane, x0, x1, x2, lanes=None):
        """One DATA LUT node: lut(table, x0, x1, x2) whose table at instance t is the byte data[plane][t] of the run's
        data (evaluate_circuit(..., data=...)), read at the node's own instance whatever lane shifts its inputs carry.
        Scales, wires, cost and lanes are those of lut."""
        plane = self._plane(plane)
        out = self.lut(0, x0, x1, x2, lanes=lanes)
        self.gate_tables[len(self.gates) - 1] = None
        self.gate_planes[len(self.gates) - 1] = plane
        return out

    def lut_multi(self, tables, x0, x1, x2):
        """A LUT family: 1 to 256 functions of the same three wires on ONE bootstrap.  tables[0] is the table of the
        LUT node lut(tables[0], x0, x1, x2), the family's leader; every further table is a sibling -- a node that takes
        no row of its level, whose wires are extracted from the leader's accumulator.  A member may be Circuit.plane(p)
        in place of a table: its table is run-time data (lut_data); planes are not de-duplicated.  Returns one (f,
        f_half, f_quarter) triple per table, the leader's first."""
        tables = [t if isinstance(t, Plane) else int(t) for t in tables]
        if not 1 <= len(tables) <= LUT_MAX_TABLES:
            raise ValueError("a LUT family has 1 to %d tables" % LUT_MAX_TABLES)
        if any(not isinstance(t, Plane) and not 0 <= t < 256 for t in tables):
            raise ValueError("a LUT node's table has 8 entries: 0 .. 255")
        for t in tables:
            if isinstance(t, Plane):
                self._plane(t.index)
        if isinstance(tables[0], Plane):
            out = [self.lut_data(tables[0].index, x0, x1, x2)]
        else:
            out = [self.lut(tables[0], x0, x1, x2)]
        leader = len(self.gates) - 1
        for t in tables[1:]:
            self.gates.append(())
            self.gate_shifts.append(())
            if isinstance(t, Plane):
                self.gate_tables[len(self.gates) - 1] = None
                self.gate_planes[len(self.gates) - 1] = t.index
            else:
                self.gate_tables[len(self.gates) - 1] = t
            self.gate_leader[len(self.gates) - 1] = leader
            base = self.n_inputs + 3 * (len(self.gates) - 1)
            out.append((Wire(base), Wire(base + 1), Wire(base + 2)))
        self._invalidate()
        return out

    def node_tables(self, g, instances, data=None):
        """The truth table of LUT node or sibling g at every instance, uint8 [instances]: its constant table, or its
        plane of `data` ([planes][instances])."""
        if g in self.gate_planes:
            if data is None:
                raise ValueError("a circuit with data planes needs data [planes=%d][instances]" % self.planes)
            return np.asarray(data)[self.gate_planes[g]].astype(np.uint8)
        return np.full(instances, self.gate_tables[g], dtype=np.uint8)

    def siblings(self, g):
        """The siblings of LUT node g (constant or data), in ascending index."""
        out, h = [], g + 1
        while self.gate_leader.get(h) == g:
            out.append(h)
            h += 1
        return out

    @property
    def has_sibling(self):
        return bool(self.gate_leader)

    def fan(self, x, lanes=None):
        """A scale-0 wire at all three scales in one bootstrap: lut(0xF0, FALSE, FALSE, x).  lanes: as in gate."""
        return self.lut(0xF0, Circuit.FALSE, Circuit.FALSE, x, lanes=lanes)

    @property
    def has_lut(self):
        return bool(self.gate_tables)

    # ---- lane routes: any public lane map inside a group, at no bootstrap (Wire.route) --------------
    def rot(self, w, d):
        """`w` rotated inside every group: lane t reads lane (t + d) mod group.  lane(d) with the lanes that leave the
        group coming back in at the other end."""
        return w.route([(t + int(d)) % self.group for t in range(self.group)])

    def swap(self, w, k):
        """Partner exchange: lane t reads lane t ^ k (butterflies, sorting networks, transposes); FALSE where t ^ k is
        no lane of the group."""
        return w.route([t ^ int(k) if (t ^ int(k)) < self.group else ROUTE_FALSE for t in range(self.group)])

    def bcast(self, w, lane):
        """Lane `lane` of `w` at every lane of its group (a flag or a carry-out every lane needs)."""
        if not 0 <= int(lane) < self.group:
            raise ValueError("bcast: lane %r is outside the group of %d" % (lane, self.group))
        return w.route([int(lane)] * self.group)

    def reverse(self, w):
        """`w` with the lanes of every group in reverse order."""
        return w.route([self.group - 1 - t for t in range(self.group)])

    @property
    def route_tables(self):
        """The distinct route tables of the circuit's references, in order of first use (terms, outputs, next states)."""
        seen = {}
        for d in [d for x in self.gate_shifts for d in x] + list(self.output_shifts) + list(self.next_shifts):
            if isinstance(d, tuple):
                seen.setdefault(d, len(seen))
        return list(seen)

    def xor(self, *wires, lanes=None):
        """The XOR of any number of wires (up to 64) in ONE bootstrap: HI of the sum node with every weight 2.  The
        wires should be bootstrapped ones (gate rows, refreshed wires): the node doubles their errors.  No wire at
        all is the constant FALSE.  lanes: as in gate."""
        if not wires:
            return Circuit.FALSE
        return self.sum_node([(2, w) for w in wires], lanes=lanes)[0]

    def refresh(self, w, lanes=None):
        """A bootstrapped copy of `w`: MID of the sum node with the one term (1, w).  lanes: as in gate."""
        return self.sum_node([(1, w)], lanes=lanes)[1]

    def kind(self, g):
        """Node g: "classic" (gate), "gate3", "sum" (sum_node), "lut" or "sibling" (a further table of a LUT node,
        lut_multi), "data" (lut_data) or "data_sibling" (a Circuit.plane member of lut_multi)."""
        if g in self.gate_leader:
            return "data_sibling" if g in self.gate_planes else "sibling"
        if g in self.gate_tables:
            return "data" if g in self.gate_planes else "lut"
        return "sum" if g in self.gate_weights else ("gate3" if len(self.gates[g]) == 3 else "classic")

    def weights(self, g):
        """The weights of node g's inputs (all 1 for gate and gate3 nodes)."""
        return self.gate_weights.get(g, (1,) * len(self.gates[g]))

    def _wide(self, g):
        """Node g is a sum node that sgfhe_circuit_create3 cannot express: not two or three unit weights."""
        return g in self.gate_weights and not (len(self.gates[g]) in (2, 3) and set(self.gate_weights[g]) == {1})

    @property
    def has_wsum(self):
        return any(self._wide(g) for g in self.gate_weights)

    def full_adder(self, x, y, c, lanes=None):
        """x + y + c in one bootstrap: returns (sum, carry) = (XOR3, MAJ) of gate3(x, y, c).  lanes: as in gate."""
        maj, _, xor3 = self.gate3(x, y, c, lanes=lanes)
        return xor3, maj

    @property
    def has_gate3(self):
        return any(len(g) == 3 for i, g in enumerate(self.gates) if i not in self.gate_weights and i not in self.gate_tables)

    def output(self, *wires):
        """Set the circuit's outputs (wire references: inputs, constants and negated wires allowed)."""
        self.outputs = [self._ref(w) for w in wires]
        self.output_shifts = [w.lanes for w in wires]
        self._invalidate()

    def next_state(self, *wires):
        """Set the next state of every register: after a step register i takes the value of wires[i] (any wire
        reference -- a node wire, an input, a register, a constant, negated or lane-shifted -- of the register's
        scale), read before any register changes."""
        if len(wires) != self.n_regs:
            raise ValueError("next_state: one wire per register (%d)" % self.n_regs)
        self.next_refs = [self._ref(w, k) for w, k in zip(wires, self.reg_scales)]
        self.next_shifts = [w.lanes for w in wires]
        self._invalidate()

    def step_plan(self):
        """The feed-forward circuit one step is: the same nodes, no registers, outputs = outputs ++ next states.  A step
        of a stepped run is, byte for byte, a run of it (registers of scale 0 only: an output has scale 0)."""
        if any(self.reg_scales):
            raise ValueError("step_plan: a register of scale 1 or 2 has no step plan (outputs are scale 0)")
        c = Circuit(self.n_inputs, group=self.group, planes=self.planes)
        c.gates, c.gate_shifts = list(self.gates), list(self.gate_shifts)
        c.gate_weights, c.gate_tables = dict(self.gate_weights), dict(self.gate_tables)
        c.gate_leader, c.gate_planes = dict(self.gate_leader), dict(self.gate_planes)
        c.gate_masks = dict(self.gate_masks)
        c.outputs = list(self.outputs) + list(self.next_refs)
        c.output_shifts = list(self.output_shifts) + list(self.next_shifts)
        return c

    @property
    def n_gates(self):
        return len(self.gates)

    @property
    def n_outputs(self):
        return len(self.outputs)

    # ---- the C plan -----------------------------------------------------------------------------
    def _invalidate(self):
        if self._plan is not None:
            self._L.sgfhe_circuit_destroy(self._plan)
            self._plan = None

    def handle(self):
        """The sgfhe_circuit* of this circuit (created on first use)."""
        if self._plan is None:
            from .engine import SgfheError
            L = _lib.lib()
            arr = lambda x, t: np.ascontiguousarray(np.array(x, dtype=t))
            vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            routes = self.route_tables
            index = {t: k + 1 for k, t in enumerate(routes)}   # route index: 0 none, k = table k - 1
            shifts = lambda ds: arr([0 if isinstance(d, tuple) else d for d in ds], np.int32)   # (a routed reference: 0)
            route_of = lambda ds: arr([index.get(d, 0) for d in ds], np.uint32)
            # The entry: the first whose feature the circuit has, so every circuit keeps the creator it always took
            masks = self.mask_tables
            mask_index = {m: k + 1 for k, m in enumerate(masks)}   # mask index: 0 every lane, k = table k - 1
            entry = next(name for name, has in (
                ("_masked", masks), ("_routed", routes), ("_seq", self.n_regs), ("_data", self.planes),
                ("_lut_multi", self.has_lut and self.has_sibling), ("_lut", self.has_lut), ("_w", self.has_wsum),
                ("3", self.has_gate3 or self.gate_weights),
                ("_lanes", self.group > 1 or any(d for x in self.gate_shifts for d in x) or any(self.output_shifts)),
                ("", True)) if has)
            n, terms = len(self.gates), [d for x in self.gate_shifts for d in x]
            o, os_ = arr(self.outputs, np.uint32), shifts(self.output_shifts)
            outs = (vp(o), vp(os_), len(self.outputs), self.group)
            if entry in ("", "_lanes", "3"):
                # [n_gates][arity]; for sgfhe_circuit_create3 two-input nodes are padded with SGFHE_CIRCUIT_NONE (and a
                # shift of 0), and a sum node of two unit weights is the three-input node (x, y, FALSE)
                arity = 3 if entry == "3" else 2
                pad = lambda i, x: (FALSE_ID if i in self.gate_weights else NONE_ID,) * (arity - len(x))
                g = arr([tuple(x) + pad(i, x) for i, x in enumerate(self.gates)], np.uint32).reshape(-1, arity)
                gs = arr([tuple(x) + (0,) * (arity - len(x)) for x in self.gate_shifts], np.int32).reshape(-1, arity)
                args = (self.n_inputs, vp(g), vp(gs), n) + outs   # (sgfhe_circuit_create: no shifts, no group)
                if not entry:
                    args = (self.n_inputs, vp(g), n, vp(o), len(self.outputs))
            else:
                # CSR: every node's terms, kind 1 for gate3 and sum nodes, 2 for LUT nodes, 3 for their siblings, 4 and 5
                # for those whose table is a data plane; the table array from sgfhe_circuit_create_lut on, the planes
                # from _data on, the registers from _seq on, the routes in _routed
                kind = arr([{"classic": 0, "lut": 2, "sibling": 3, "data": 4, "data_sibling": 5}.get(self.kind(g), 1)
                            for g in range(n)], np.uint32)
                start = np.cumsum([0] + [len(x) for x in self.gates]).astype(np.uint32)
                tr, ts = arr([ref for x in self.gates for ref in x], np.uint32), shifts(terms)
                tw = arr([w for g in range(n) for w in self.weights(g)], np.int32)
                tb = arr([self.gate_planes[g] if g in self.gate_planes else self.gate_tables.get(g, 0) for g in range(n)],
                         np.uint32)
                nr, ns, rs = arr(self.next_refs, np.uint32), shifts(self.next_shifts), arr(self.reg_scales, np.uint32)
                rt = arr(routes, np.int32).reshape(len(routes), self.group)
                tt, ot, nt = route_of(terms), route_of(self.output_shifts), route_of(self.next_shifts)
                data = entry in ("_data", "_seq", "_routed", "_masked")
                mt = arr(masks, np.uint8).reshape(len(masks), self.group)
                nm = arr([mask_index.get(self.gate_masks.get(g), 0) for g in range(n)], np.uint32)
                args = ((self.n_inputs,) + ((self.planes,) if data else ()) + (vp(kind), vp(start), vp(tr), vp(ts), vp(tw)) +
                        ((vp(tb),) if entry != "_w" else ()) + (n,) + outs +
                        ((self.n_regs, vp(nr), vp(ns), vp(rs)) if entry in ("_seq", "_routed", "_masked") else ()) +
                        ((len(routes), vp(rt), vp(tt), vp(ot), vp(nt)) if entry in ("_routed", "_masked") else ()) +
                        ((len(masks), vp(mt), vp(nm)) if entry == "_masked" else ()))
            h = ctypes.c_void_p()
            rc = getattr(L, "sgfhe_circuit_create" + entry)(*args, ctypes.byref(h))
            if rc != 0:
                raise SgfheError(rc, "sgfhe_circuit_create: %s" % (
                    "malformed circuit (ids, topological order, at least one output, lane shifts inside the group, no "
                    "lane mask on a LUT node that leads a live sibling)"
                    if rc == -1 else "out of memory"))
            self._L, self._plan = L, h
        return self._plan

    def info(self):
        """dict(levels, nodes (bootstraps per instance: the live nodes that take a row, so no LUT sibling), widest (such
        nodes in the widest level), slots (those of sibling wires included)) -- none of which sees lane masks -- and, for
        a circuit with lane masks, rows_per_group (Circuit.rows_per_group; without masks it is nodes * group, and the
        dict stays the four entries it always was)."""
        info = (ctypes.c_uint64 * 4)()
        h = self.handle()
        rc = self._L.sgfhe_circuit_info(h, info)
        assert rc == 0
        out = dict(levels=int(info[0]), nodes=int(info[1]), widest=int(info[2]), slots=int(info[3]))
        if self.gate_masks:
            out["rows_per_group"] = self.rows_per_group()
        return out

    def rows_per_group(self):
        """The level-call rows one group of `group` instances costs (sgfhe_circuit_masks): the lanes a node takes a row
        on, summed over the live nodes that take a row -- nodes * group for a circuit without lane masks."""
        n_masks, rows = ctypes.c_uint32(), ctypes.c_uint64()
        h = self.handle()
        rc = self._L.sgfhe_circuit_masks(h, ctypes.byref(n_masks), ctypes.byref(rows))
        assert rc == 0
        return int(rows.value)

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    # ---- host statements of the model -------------------------------------------------------------
    def node_levels(self):
        """The level of every node, 0 for a pruned one (the C planner's rule, in Python): a node is live when an output
        reaches it, a leader also when one of its siblings is live; a sibling has its leader's level."""
        def node(ref):   # producing node of a wire, -1 for inputs and the constant
            i = ref & ~NOT_BIT & 0xFFFFFFFF
            return -1 if i == FALSE_ID or i < self.n_inputs else (i - self.n_inputs) // 3

        live = [False] * len(self.gates)
        for ref in self.outputs + self.next_refs:   # (a next state is a reader, as an output is)
            if node(ref) >= 0:
                live[node(ref)] = True
        for g in range(len(self.gates) - 1, -1, -1):
            if live[g]:
                if g in self.gate_leader:
                    live[self.gate_leader[g]] = True
                for ref in self.gates[g]:
                    if node(ref) >= 0:
                        live[node(ref)] = True
        level = [0] * len(self.gates)
        for g, refs in enumerate(self.gates):
            if live[g] and g in self.gate_leader:
                level[g] = level[self.gate_leader[g]]
            elif live[g]:
                level[g] = 1 + max(level[node(ref)] if node(ref) >= 0 else 0 for ref in refs)
        return level

    def live_siblings(self, g):
        """The siblings of node g that an output reaches, in ascending index."""
        level = self.node_levels()
        return [h for h in self.siblings(g) if level[h]]

    def schedule(self):
        """The levels the planner runs: a list (level 1, 2, ...) of lists of node indices in ascending
        order, after pruning the nodes no output depends on -- the nodes that take a row: a LUT sibling rides on its
        leader's row and is not listed (live_siblings)."""
        level = self.node_levels()
        levels = [[] for _ in range(max(level, default=0))]
        for g in range(len(self.gates)):
            if level[g] and g not in self.gate_leader:
                levels[level[g] - 1].append(g)
        return levels

    def evaluate_plain(self, bits, data=None, _next=False):
        """The circuit in clear: bits [n_inputs][instances] (bool) -> [n_outputs][instances] (bool).  data: the planes
        of a circuit that has any, uint8 [planes][instances].  (One step of a circuit with registers, whose values are
        the first rows of `bits`; evaluate_plain_steps feeds them back.)"""
        bits = np.asarray(bits, dtype=bool).reshape(self.n_inputs, -1)
        inst = bits.shape[1]
        data = check_data(self, data, inst)
        wires = {}

        def val(ref, d):
            i = ref & ~NOT_BIT & 0xFFFFFFFF
            v = np.zeros(inst, dtype=bool) if i == FALSE_ID else (bits[i] if i < self.n_inputs else wires[i])
            v = lane_shift(v, d, self.group)
            return ~v if ref & NOT_BIT else v

        if self.gate_masks and inst % self.group:
            raise ValueError("the instances (%d) must be a multiple of the lane group (%d)" % (inst, self.group))
        on = {g: np.asarray(m, dtype=bool)[np.arange(inst) % self.group] for g, m in self.gate_masks.items()}
        for levelnodes in self.schedule():
            for g in levelnodes:
                base = self.n_inputs + 3 * g
                self._plain_node(g, base, val, wires, inst, data)
                for w in range(3 if g in on else 0):   # a masked node (it leads no sibling): FALSE on its off lanes
                    wires[base + w] = wires[base + w] & on[g]
        if not self.outputs:
            raise ValueError("circuit has no outputs")
        out = np.stack([val(ref, d) for ref, d in zip(self.outputs, self.output_shifts)])
        if not _next:
            return out
        return out, np.array([val(ref, d) for ref, d in zip(self.next_refs, self.next_shifts)], dtype=bool).reshape(self.n_regs, inst)

    def _plain_node(self, g, base, val, wires, inst, data):
        """The three wires of node g (and of its siblings) in clear, into `wires`: evaluate_plain's step for one node."""
        if g in self.gate_tables:
            x = [val(ref, d).astype(np.int64) for ref, d in zip(self.gates[g], self.gate_shifts[g])]
            for h in [g] + self.siblings(g):   # (a sibling: its own table at the leader's inputs)
                f = ((self.node_tables(h, inst, data).astype(np.int64) >> (x[0] + 2 * x[1] + 4 * x[2])) & 1).astype(bool)
                hb = self.n_inputs + 3 * h
                wires[hb], wires[hb + 1], wires[hb + 2] = f, f, f
            return
        if g in self.gate_weights:
            s = sum(w * val(ref, d).astype(np.int64)
                    for w, ref, d in zip(self.gate_weights[g], self.gates[g], self.gate_shifts[g])) % 4
            wires[base], wires[base + 1], wires[base + 2] = s >= 2, (s == 1) | (s == 2), s % 2 == 1
            return
        if len(self.gates[g]) == 3:
            x, y, z = (val(ref, d) for ref, d in zip(self.gates[g], self.gate_shifts[g]))
            wires[base], wires[base + 1], wires[base + 2] = (x & y) | (z & (x | y)), (x | y | z) & ~(x & y & z), \
                x ^ y ^ z
            return
        x, y = (val(ref, d) for ref, d in zip(self.gates[g], self.gate_shifts[g]))
        wires[base], wires[base + 1], wires[base + 2] = x & y, x | y, x ^ y

    def evaluate_plain_steps(self, state_bits, stream_bits, data=None):
        """A stepped run in clear: state_bits [registers][instances] (None: all FALSE), stream_bits
        [steps][stream inputs][instances], data [steps][planes][instances] for a circuit with planes ->
        (outputs [steps][n_outputs][instances], state [registers][instances] after the last step).  A step's outputs
        are taken before the registers change."""
        stream = np.asarray(stream_bits, dtype=bool)
        if stream.ndim != 3 or stream.shape[1] != self.n_inputs - self.n_regs:
            raise ValueError("stream_bits must be [steps][stream inputs=%d][instances]" % (self.n_inputs - self.n_regs))
        steps, inst = stream.shape[0], stream.shape[2]
        state = np.zeros((self.n_regs, inst), dtype=bool) if state_bits is None else \
            np.asarray(state_bits, dtype=bool).reshape(self.n_regs, inst).copy()
        data = check_step_data(self, data, steps, inst)
        outs = np.zeros((steps, len(self.outputs), inst), dtype=bool)
        for s in range(steps):
            outs[s], state = self.evaluate_plain(np.concatenate([state, stream[s]]), None if data is None else data[s],
                                                 _next=True)
        return outs, state


def check_data(circuit, data, instances):
    """The planes of a run, checked: uint8 [circuit.planes][instances] (ValueError otherwise, and for a circuit with
    planes and no data); None for a circuit without planes."""
    if not circuit.planes:
        if data is not None:
            raise ValueError("data given for a circuit without data planes")
        return None
    if data is None:
        raise ValueError("a circuit with data planes needs data [planes=%d][instances]" % circuit.planes)
    d = np.asarray(data)
    if d.dtype != np.uint8 or d.shape != (circuit.planes, instances):
        raise ValueError("data must be uint8 [planes=%d][instances=%d], got %s %r"
                         % (circuit.planes, instances, d.dtype, d.shape))
    return d


def check_step_data(circuit, data, steps, instances):
    """The planes of a stepped run, checked: uint8 [steps][circuit.planes][instances]; None for a circuit without."""
    if not circuit.planes or data is None:
        return check_data(circuit, data, instances)
    d = np.asarray(data)
    if d.dtype != np.uint8 or d.shape != (steps, circuit.planes, instances):
        raise ValueError("data must be uint8 [steps=%d][planes=%d][instances=%d], got %s %r"
                         % (steps, circuit.planes, instances, d.dtype, d.shape))
    return d


def lane_shift(v, d, group):
    """The lane-shifted read of a wire: v [instances, ...] -> the array whose entry t is v[t + d] where
    0 <= t % group + d < group, and zero (the constant FALSE, the trivial LWE (0, 0)) elsewhere.  d a route table (a
    tuple of `group` entries, Wire.route): entry t is v[t - t % group + d[t % group]], and zero where that entry of the
    table is ROUTE_FALSE."""
    if not isinstance(d, tuple) and d == 0:
        return v
    if v.shape[0] % group:
        raise ValueError("the instances (%d) must be a multiple of the lane group (%d)" % (v.shape[0], group))
    t = np.arange(v.shape[0])
    if isinstance(d, tuple):
        if len(d) != group:
            raise ValueError("a route table of %d entries in a group of %d" % (len(d), group))
        src = np.asarray(d, dtype=np.int64)[t % group]
        ok = src >= 0
        out = np.zeros_like(v)
        out[ok] = v[(t - t % group + src)[ok]]
        return out
    ok = (t % group + d >= 0) & (t % group + d < group)
    out = np.zeros_like(v)
    out[ok] = v[t[ok] + d]
    return out


def packed_adder(width):
    """A Kogge-Stone adder over lanes: Circuit(2, group=width) whose two input wires hold words of `width` bits,
    LSB at lane 0 of each group.  Level 1 is one node (x, y) giving generate g = AND and propagate p = XOR; each of
    the ceil(log2(width)) prefix stages s = 1, 2, 4 ... is two levels -- the nodes (p, g.lane(-s)) and
    (p, p.lane(-s)), then g = g OR (p AND g.lane(-s)) -- and the last node is p XOR carry.lane(-1).  Outputs: the sum
    word, and the carry wire, whose lane width - 1 is the carry-out of the word.  1 + 3 stages nodes per instance
    (the last stage's (p, p) node is pruned), 2 + 2 stages levels."""
    if int(width) < 1:
        raise ValueError("width must be at least 1")
    c = Circuit(2, group=int(width))
    x, y = c.inputs
    g, _, p0 = c.gate(x, y)
    p, s = p0, 1
    while s < width:
        pg = c.gate(p, g.lane(-s))[0]
        pp = c.gate(p, p.lane(-s))[0]
        g, p = c.gate(g, pg)[1], pp
        s *= 2
    c.output(c.gate(p0, g.lane(-1))[2], g)
    return c


def ripple_adder(width):
    """A bit-sliced ripple-carry adder of full adders: Circuit(2 * width) whose inputs are x_0 .. x_{width-1} then
    y_0 .. y_{width-1} (LSB first), one full_adder -- one bootstrap -- per bit, the first carry-in FALSE.  Outputs:
    the width sum bits, then the carry-out.  width nodes in width levels.  Only MAJ is carried on; every sum bit
    (XOR3) is an output, so no node reads a wire that was not bootstrapped or freshly encrypted."""
    if int(width) < 1:
        raise ValueError("width must be at least 1")
    width = int(width)
    c = Circuit(2 * width)
    carry, sums = Circuit.FALSE, []
    for i in range(width):
        s, carry = c.full_adder(c.inputs[i], c.inputs[width + i], carry)
        sums.append(s)
    c.output(*(sums + [carry]))
    return c


def gf2_matvec(M, refresh_inputs=True):
    """y = M x over GF(2) with ONE sum node per output bit: Circuit(columns of M) whose output i is the XOR of the inputs
    j with M[i][j] = 1 (Circuit.xor: HI of all weights 2; an empty row is the constant FALSE).  refresh_inputs: every
    input some row uses is first refreshed (Circuit.refresh, one bootstrap each), as it must be when the inputs are
    fresh encryptions -- a weight of 2 doubles the error, and a split encrypt_private bit is already at the limit;
    False for inputs that are gate rows or packed outputs.  Rows of at most 64 ones.  Two levels (one without the
    refreshes); every output is a gate row, so SGFHE_CIRCUIT_PACK_DIRECT packs them all without a refresh."""
    M = np.asarray(M)
    if M.ndim != 2 or not np.isin(M, (0, 1)).all():
        raise ValueError("gf2_matvec: a two-dimensional 0/1 matrix is expected")
    M = M.astype(bool)
    if M.sum(axis=1).max(initial=0) > MAX_TERMS:
        raise ValueError("gf2_matvec: a row has more than %d ones" % MAX_TERMS)
    c = Circuit(M.shape[1])
    src = {j: (c.refresh(c.inputs[j]) if refresh_inputs else c.inputs[j]) for j in range(M.shape[1]) if M[:, j].any()}
    c.output(*[c.xor(*[src[j] for j in np.flatnonzero(row)]) for row in M])
    return c


def crc16_matrix(message_bits):
    """The 16 x message_bits 0/1 matrix of CRC-16/XMODEM (polynomial 0x1021, initial value 0: binascii.crc_hqx(msg, 0)),
    which is GF(2)-linear in the message.  Column j is message bit j, the bits in the order the CRC consumes them (bit 7
    of byte 0 first); row k is bit k of the CRC (LSB first).  message_bits: a multiple of 8."""
    import binascii
    if message_bits < 8 or message_bits % 8:
        raise ValueError("crc16: the message is a whole number of bytes")
    M = np.zeros((16, message_bits), dtype=np.uint8)
    for j in range(message_bits):
        msg = bytearray(message_bits // 8)
        msg[j // 8] = 0x80 >> (j % 8)
        crc = binascii.crc_hqx(bytes(msg), 0)
        M[:, j] = [(crc >> k) & 1 for k in range(16)]
    return M


def crc16_ccitt(message_bits, refresh_inputs=True):
    """CRC-16 (CCITT polynomial 0x1021, initial value 0: binascii.crc_hqx(msg, 0)) of a message of `message_bits` bits
    as gf2_matvec(crc16_matrix(message_bits)): 16 sum nodes, plus one refresh per message bit when asked.  Inputs and
    outputs in the bit orders of crc16_matrix."""
    return gf2_matvec(crc16_matrix(message_bits), refresh_inputs=refresh_inputs)


def serial_adder():
    """A bit-serial adder: Circuit(3, registers=1) whose register is the carry and whose stream inputs are one bit of
    x and one of y per step, LSB first.  One full_adder -- one bootstrap -- per step: the output is the sum bit (XOR3),
    the next state the carry (MAJ, a gate row, so nothing accumulates over the steps).  Numbers of any width in a wire
    table of one step; the carry-out is the state after the last step."""
    c = Circuit(3, registers=1)
    s, carry = c.full_adder(c.stream_inputs[0], c.stream_inputs[1], c.registers[0])
    c.output(s)
    c.next_state(carry)
    return c


def crc16_stream_matrix(chunk_bits):
    """The 16 x (16 + chunk_bits) 0/1 matrix of one CRC-16/XMODEM step, crc' = binascii.crc_hqx(chunk, crc), which is
    GF(2)-linear in (crc, chunk): columns 0 .. 15 are the bits of the running CRC (LSB first), the others the chunk's
    bits in the order the CRC consumes them; rows as crc16_matrix.  From binascii.crc_hqx on unit vectors."""
    import binascii
    if chunk_bits < 8 or chunk_bits % 8:
        raise ValueError("crc16: a chunk is a whole number of bytes")
    M = np.zeros((16, 16 + chunk_bits), dtype=np.uint8)
    zero = bytes(chunk_bits // 8)
    for j in range(16):
        crc = binascii.crc_hqx(zero, 1 << j)
        M[:, j] = [(crc >> k) & 1 for k in range(16)]
    M[:, 16:] = crc16_matrix(chunk_bits)
    return M


def crc16_stream(chunk_bits):
    """CRC-16 (binascii.crc_hqx) of a message of any whole number of chunks, one chunk of `chunk_bits` bits per step:
    Circuit(16 + chunk_bits, registers=16) whose registers hold the running CRC (bit k in register k) and whose stream
    inputs are the chunk's bits in the order the CRC consumes them (bit 7 of byte 0 first).  The state update is
    gf2_matvec's construction over (state ++ refreshed chunk): the chunk bits, fresh encryptions, are refreshed first;
    the registers are HI wires already.  Next state = the 16 HI wires = the outputs: after the last chunk the outputs
    are the CRC of the whole message (registers that start FALSE: initial value 0).  chunk_bits + 16 bootstraps a step."""
    M = crc16_stream_matrix(chunk_bits).astype(bool)
    c = Circuit(16 + int(chunk_bits), registers=16)
    src = list(c.registers) + [c.refresh(w) for w in c.stream_inputs]
    hi = [c.xor(*[src[j] for j in np.flatnonzero(row)]) for row in M]
    c.output(*hi)
    c.next_state(*hi)
    return c


def bitonic_stages(G):
    """The compare-exchange stages of the bitonic sorting network on G = 2^k lanes, ascending: a list of (k, table) --
    the partner of lane t is lane t ^ k, and table[t] in {t, t ^ k} is the lane whose [own > partner] decides the swap
    at lane t: the lane itself where it keeps the smaller element when it is the larger (the low partner of an ascending
    block, the high partner of a descending one), its partner otherwise.  Both partners read the same decision."""
    G = int(G)
    if G < 1 or G & (G - 1):
        raise ValueError("bitonic sort: the group must be a power of two")
    stages, block = [], 2
    while block <= G:
        k = block // 2
        while k >= 1:
            stages.append((k, tuple(t if ((t & k) == 0) == ((t & block) == 0) else t ^ k for t in range(G))))
            k //= 2
        block *= 2
    return stages


def bitonic_sort(width, G, refresh_inputs=True, masked=False):
    """Sorts the G numbers of `width` bits of every lane group ascending: Circuit(width, group=G), bit-sliced -- input
    wire i holds bit i (LSB first) of every number, lane = element -- and outputs laid out the same way, lane 0 the
    smallest.  The bitonic network's log2(G) (log2(G) + 1) / 2 stages (bitonic_stages), each one compare-exchange at a
    distance k built from lane routes (Circuit.swap, Wire.route), so no input is per lane and nothing but the nodes
    below costs a bootstrap:
      * g = [own > partner] is the carry out of own + ~partner: a chain of `width` gate3 nodes, carry' = MAJ(x_i,
        ~swap(x_i, k), carry) from the LSB up, the first carry FALSE;
      * the swap decision s = g.route(table) of bitonic_stages -- g at the lane itself or at its partner;
      * the new bit i is the mux (s ? partner : own) as ONE LUT node, lut(0xCA, x_i at Dr/4, swap(x_i, k) at Dr/2, s).
    The LUT mux is the cheapest the noise rules allow: it reads bootstrapped wires only (the rule of LUT nodes), and a
    mux from two-input nodes takes three bootstraps a bit.  It needs every bit at the scales 2 and 1, which a LUT node
    returns itself; before the first stage one fan per bit brings the inputs there.  refresh_inputs: every input is
    refreshed first (Circuit.refresh, one bootstrap each), as it must be when the inputs are fresh encryptions -- the fan
    is a LUT node, and a split encrypt_private bit is already at the limit of its rule; False for inputs that are gate
    rows or packed outputs.
    masked=True: the comparator chain carries lanes=sorted(set(table)), the decision lanes of the stage -- G / 2 of them,
    the only lanes of g the swap decision reads, and the chain reads its own carry at those lanes only -- so a stage costs
    width G / 2 + width G rows a group in place of 2 width G: bitonic_sort(3, 8) 264 rows a group in place of 336.
    Nodes: width refreshes and width fans, then 2 width per stage -- 2 width + width log2(G) (log2(G) + 1); levels:
    2 + (width + 1) per stage (one node and one level less per bit without the refreshes)."""
    width, G = int(width), int(G)
    if width < 1:
        raise ValueError("bitonic sort: width must be at least 1")
    stages = bitonic_stages(G)
    c = Circuit(width, group=G)
    x = [c.fan(c.refresh(w) if refresh_inputs else w) for w in c.inputs]   # per bit: (scale 0, scale 1, scale 2)
    for k, table in stages:
        carry, lanes = Circuit.FALSE, sorted(set(table)) if masked else None
        for i in range(width):
            carry = c.gate3(x[i][0], ~c.swap(x[i][0], k), carry, lanes=lanes)[0]
        s = carry.route(table)
        x = [c.lut(0xCA, x[i][2], c.swap(x[i][1], k), s) for i in range(width)]
    c.output(*[xi[0] for xi in x])
    return c


def lane_reduce(c, w, which, G=None):
    """`w` folded over the lanes of every group with `which` (0 AND, 1 OR, 2 XOR: the index of the wire in gate()'s
    triple), G = c.group a power of two: stage k = 1, 2, 4 ... < G is c.gate(acc, acc.lane(k), lanes=range(0, G, 2 k))
    [which] -- lane t takes (acc[t], acc[t + k]) at the lanes that are multiples of 2 k, which are on in stage k / 2.  The
    result sits at lane 0 and is FALSE at every other lane (Circuit.bcast brings it to all).  G - 1 rows a group, in
    log2(G) levels, where a tree on all lanes costs G log2(G)."""
    G = c.group if G is None else int(G)
    if G != c.group or G < 2 or G & (G - 1):
        raise ValueError("lane_reduce: G must be the circuit's lane group, a power of two above 1")
    if which not in (0, 1, 2):
        raise ValueError("lane_reduce: which is 0 (AND), 1 (OR) or 2 (XOR)")
    acc, k = w, 1
    while k < G:
        acc = c.gate(acc, acc.lane(k), lanes=range(0, G, 2 * k))[which]
        k *= 2
    return acc


def packed_equal(width):
    """Are two packed words equal: Circuit(2, group=width) whose input wires hold words of `width` bits (a power of two),
    one bit a lane.  One XNOR node on all lanes, then lane_reduce with AND: the output is [x == y] at lane 0 of every
    group and FALSE at the other lanes.  2 width - 1 rows a group."""
    width = int(width)
    c = Circuit(2, group=width)
    x, y = c.inputs
    c.output(lane_reduce(c, ~c.gate(x, y)[2], 0))
    return c


def _at_scale(circuit, w, want):
    """w at scale `want`: as it is, or through one LUT node at its own position (the table of "the input at position p")."""
    have = circuit.scale(w)
    if have in (None, want):
        return w
    p = 2 - have
    args = [Circuit.FALSE] * 3
    args[p] = w
    return circuit.lut((0xAA, 0xCC, 0xF0)[p], *args)[want]


def shannon(circuit, tables, xs, refresh=False, family=True):
    """Any functions of k >= 3 wires by Shannon expansion.  tables: one integer per function, bit s of which is its value
    at s = x_0 + 2 x_1 + ... + 2^(k-1) x_(k-1); xs: the k wires, bootstrapped ones (refresh=True refreshes each first,
    as fresh encryptions need: the noise rule in include/sgfhe_hip.h).  The 2^(k-3) cofactors of every function on
    (x_0, x_1, x_2) are 8-entry tables: all of them, equal ones merged and the constants left out, form ONE family
    (Circuit.lut_multi) -- one bootstrap, whatever their number, as there are only 256 tables.  A mux tree of LUT nodes
    follows, lut(0xCA, lo[2], hi[1], x_j) for j = 3 .. k - 1, equal nodes merged and a mux of two equal halves left out.
    The wires are brought to the scale they are read at only where needed: x_0 and x_1 through one LUT node each (fan,
    for a scale-0 wire), x_2 and the selectors only if they are not of scale 0.  family=False builds one LUT node per
    cofactor table instead, for comparison.  Returns one scale-0 wire per function (a constant function: the constant)."""
    xs = list(xs)
    k = len(xs)
    if k < 3:
        raise ValueError("shannon: at least three wires")
    tables = [int(t) for t in tables]
    if any(not 0 <= t < 1 << (1 << k) for t in tables):
        raise ValueError("shannon: a function of %d wires has a table of %d bits" % (k, 1 << k))
    if refresh:
        xs = [circuit.refresh(x) for x in xs]
    at_scale = lambda w, want: _at_scale(circuit, w, want)
    const = {0x00: (Circuit.FALSE,) * 3, 0xFF: (Circuit.TRUE,) * 3}
    cof = [[(t >> (8 * h)) & 0xFF for h in range(1 << (k - 3))] for t in tables]
    distinct = sorted({c for row in cof for c in row if c not in const})
    triple = dict(const)
    if distinct:
        x0, x1, x2 = at_scale(xs[0], 2), at_scale(xs[1], 1), at_scale(xs[2], 0)
        if family:
            triple.update(zip(distinct, circuit.lut_multi(distinct, x0, x1, x2)))
        else:
            triple.update((c, circuit.lut(c, x0, x1, x2)) for c in distinct)
    layer = [[triple[c] for c in row] for row in cof]
    for j in range(3, k):
        sel, muxes = None, {}
        nxt = []
        for row in layer:
            out = []
            for lo, hi in zip(row[0::2], row[1::2]):
                if lo == hi:
                    out.append(lo)
                    continue
                if (lo, hi) not in muxes:
                    sel = at_scale(xs[j], 0) if sel is None else sel
                    muxes[(lo, hi)] = circuit.lut(0xCA, lo[2], hi[1], sel)
                out.append(muxes[(lo, hi)])
            nxt.append(out)
        layer = nxt
    return [row[0][0] for row in layer]


def lookup(circuit, xs, count=1, plane0=0, refresh=False):
    """`count` functions of k = len(xs) >= 3 wires whose tables are run-time data: shannon with per-instance tables.
    Function f's cofactor h -- the value of x_3 .. x_(k-1) -- on (x_0, x_1, x_2) is the data table of plane
    plane0 + f 2^(k-3) + h (lookup_data lays a run's planes out this way).  All these tables are members of LUT families on
    (x_0, x_1, x_2), one family -- one bootstrap -- per 256 members; shannon's mux tree follows, lut(0xCA, lo[2], hi[1],
    x_j) for j = 3 .. k - 1, with nothing merged, as the tables are unknown when the circuit is built.  Scales and
    refresh as in shannon.  Returns one scale-0 wire per function."""
    xs = list(xs)
    k = len(xs)
    if k < 3:
        raise ValueError("lookup: at least three wires")
    count, plane0 = int(count), int(plane0)
    H = 1 << (k - 3)
    if count < 1 or plane0 < 0 or plane0 + count * H > circuit.planes:
        raise ValueError("lookup: planes %d .. %d are needed, the circuit has %d" % (plane0, plane0 + count * H - 1,
                                                                                   circuit.planes))
    if refresh:
        xs = [circuit.refresh(x) for x in xs]
    x0, x1, x2 = _at_scale(circuit, xs[0], 2), _at_scale(circuit, xs[1], 1), _at_scale(circuit, xs[2], 0)
    members = [Circuit.plane(plane0 + i) for i in range(count * H)]
    triples = []
    for i in range(0, len(members), LUT_MAX_TABLES):
        triples += circuit.lut_multi(members[i:i + LUT_MAX_TABLES], x0, x1, x2)
    layer = [triples[f * H:(f + 1) * H] for f in range(count)]
    for j in range(3, k):
        sel = _at_scale(circuit, xs[j], 0)
        layer = [[circuit.lut(0xCA, lo[2], hi[1], sel) for lo, hi in zip(row[0::2], row[1::2])] for row in layer]
    return [row[0][0] for row in layer]


def lookup_data(tables, k):
    """The planes of lookup: tables [count][instances] of integers of 2^k bits (bit s of tables[f][t] is function f's
    value at s = x_0 + 2 x_1 + ... at instance t) -> uint8 [count 2^(k-3)][instances], plane f 2^(k-3) + h holding
    bits 8 h .. 8 h + 7 of every table of function f."""
    k = int(k)
    if k < 3:
        raise ValueError("lookup_data: at least three wires")
    rows = [[int(t) for t in row] for row in tables]
    if any(len(row) != len(rows[0]) for row in rows):
        raise ValueError("lookup_data: ragged tables")
    if any(not 0 <= t < 1 << (1 << k) for row in rows for t in row):
        raise ValueError("lookup_data: a function of %d wires has a table of %d bits" % (k, 1 << k))
    H = 1 << (k - 3)
    out = np.zeros((len(rows) * H, len(rows[0]) if rows else 0), dtype=np.uint8)
    for f, row in enumerate(rows):
        for t, tab in enumerate(row):
            out[f * H:(f + 1) * H, t] = np.frombuffer(tab.to_bytes(H, "little"), dtype=np.uint8)
    return out


def lwe_not(words, r, one=None):
    """NOT of LWEs [..., n + 1] over Z_r: enc_trivial(true) - w (a -> -a, b -> Dr - b, mod r).  one: the codeword of
    the wire in place of Dr (positions 0 and 1 of a LUT node read wires at Dr/4 and Dr/2)."""
    words = np.asarray(words, dtype=np.uint64)
    t = np.zeros(words.shape[-1], dtype=np.uint64)
    t[-1] = r // 4 if one is None else one
    return (t + np.uint64(r) - words) & np.uint64(r - 1)


def level_row_map(circuit, nodes, inst):
    """The rows of a level whose nodes are `nodes` (one list of Circuit.schedule) over `inst` instances, as two arrays
    (rank of the row's node in `nodes`, instance of the row).  A circuit without lane masks: row = rank * instances +
    instance.  A circuit with any (the masked plan): the level's (node, lane) pairs -- nodes ascending, the lanes a node
    takes a row on ascending (Circuit.lanes_on) -- each over the instances / group groups, row = pair * per + group."""
    if not circuit.gate_masks:
        return np.repeat(np.arange(len(nodes)), inst), np.tile(np.arange(inst), len(nodes))
    if inst % circuit.group:
        raise ValueError("the instances (%d) must be a multiple of the lane group (%d)" % (inst, circuit.group))
    grp = np.arange(inst // circuit.group) * circuit.group
    pairs = [(k, l) for k, g in enumerate(nodes) for l in circuit.lanes_on(g)]
    rank = np.repeat(np.array([k for k, _ in pairs], dtype=np.int64), len(grp))
    at = np.concatenate([grp + l for _, l in pairs]) if pairs else np.zeros(0, dtype=np.int64)
    return rank, at


def replay_levels(circuit, inputs, r, boot, boot_lut=None, data=None, call0=0, _next=False):
    """The circuit composed on the host from whole-level bootstrap calls, in the row and call order of
    sgfhe_circuit_run: inputs [n_inputs][instances][n + 1] -> outputs [n_outputs][instances][n + 1].
    `boot(call, a1, b1, a2, b2)` runs one call (rows of at most CALL_ROWS) and returns [rows][3][n + 1];
    `call` counts the calls from 0.  A three-input node is the row (x + y mod r, z); its third wire is
    x + y + z - 2 * (row 0 of the result) mod r.  A sum node is the row (U, FALSE), U = the sum of weight * term mod r
    -- the bootstrap adds its two inputs first, so this is also what (x + y, z) gives for unit weights -- and its third
    wire U - 2 * (row 0 of the result) mod r.  A LUT node is the row (X0 + X1 + X2, FALSE); the LUT rows of a call
    are run by `boot_lut(call, a, b, tables, idx)` -- their rows, their tables and their indices within the call, so
    that a test can drive them from a second oracle -- which returns [rows][3][n + 1], the node's three wires; `boot`
    sees every row of a call that holds other rows too (its results for the LUT rows are dropped) and is not called
    for a call of LUT rows only.  The wires of a live LUT sibling are boot_lut of its leader's rows and indices with the
    sibling's table -- boot_lut is a function of (call, row, index, table) --, all siblings of a call in one further
    boot_lut(call, ...) whose rows and indices repeat.  data: the planes of a circuit that has any, uint8
    [planes][instances]; the row of a data node or data sibling at instance t goes to boot_lut with the table
    data[plane][t].  call0: the number of the first call (replay_steps counts on from step to step).  A circuit with lane
    masks runs its levels in the row order of the masked plan (level_row_map), and the wires of a masked node are the
    trivial LWE (0, 0) on its off lanes.  A checking and measuring aid: the engine's circuit path does this on the
    device (Engine.circuit_run)."""
    inputs = np.asarray(inputs, dtype=np.uint64)
    inst, row = inputs.shape[1], inputs.shape[2]
    data = check_data(circuit, data, inst)
    n = row - 1
    wires = {}

    def val(ref, d, one=None):
        i = ref & ~NOT_BIT & 0xFFFFFFFF
        v = np.zeros((inst, row), dtype=np.uint64) if i == FALSE_ID else \
            (inputs[i] if i < circuit.n_inputs else wires[i])
        v = lane_shift(v, d, circuit.group)
        return lwe_not(v, r, one) if ref & NOT_BIT else v

    call = call0
    for nodes in circuit.schedule():
        # row = rank * instances + instance, or the pairs of a masked plan: row j is node rk[j] at instance ri[j]
        mask = np.uint64(r - 1)
        rk, ri = level_row_map(circuit, nodes, inst)

        def pair(g):   # the bootstrap inputs of node g: (x, y), (x + y mod r, z) of a three-input node, (U, FALSE)
            if circuit.kind(g) in ("lut", "data"):   # position p reads a wire at the codeword Dr >> (2 - p)
                vals = [val(ref, d, (r // 4) >> (2 - p))
                        for p, (ref, d) in enumerate(zip(circuit.gates[g], circuit.gate_shifts[g]))]
                return (vals[0] + vals[1] + vals[2]) & mask, np.zeros_like(vals[0])
            vals = [val(ref, d) for ref, d in zip(circuit.gates[g], circuit.gate_shifts[g])]
            if circuit.kind(g) == "sum":
                u = sum(w * v.astype(np.int64) for w, v in zip(circuit.gate_weights[g], vals)) % r
                return u.astype(np.uint64), np.zeros_like(vals[0])
            if len(vals) == 3:
                return (vals[0] + vals[1]) & mask, vals[2]
            return vals[0], vals[1]

        pairs = [pair(g) for g in nodes]
        x = np.stack([p[0] for p in pairs])[rk, ri]
        y = np.stack([p[1] for p in pairs])[rk, ri]
        res = np.zeros((len(x), 3, row), dtype=np.uint64)
        tables = np.stack([circuit.node_tables(g, inst, data).astype(np.int64) if g in circuit.gate_tables
                           else np.full(inst, -1, dtype=np.int64) for g in nodes])[rk, ri]
        sibs = [(k, h) for k, g in enumerate(nodes) for h in circuit.live_siblings(g)]   # (rank of the leader, sibling)
        for _, h in sibs:
            for w in range(3):
                wires[circuit.n_inputs + 3 * h + w] = np.zeros((inst, row), dtype=np.uint64)
        for r0 in range(0, len(x), CALL_ROWS):
            sl = slice(r0, r0 + CALL_ROWS)
            idx = np.flatnonzero(tables[sl] >= 0)
            if len(idx) < len(tables[sl]):
                res[sl] = boot(call, x[sl, :n], x[sl, n], y[sl, :n], y[sl, n])
            if len(idx):
                res[r0 + idx] = boot_lut(call, x[sl, :n][idx], x[sl, n][idx], tables[sl][idx].astype(np.uint8), idx)
            part = [(k, h, np.flatnonzero(rk[sl] == k)) for k, h in sibs]   # the leader's rows of this call
            part = [(k, h, sel) for k, h, sel in part if len(sel)]
            if part:
                sel = np.concatenate([s_ for _, _, s_ in part])
                tab = np.concatenate([circuit.node_tables(h, inst, data)[ri[r0 + s_]] for k, h, s_ in part])
                got = boot_lut(call, x[sl, :n][sel], x[sl, n][sel], tab, sel)
                at = 0
                for k, h, s_ in part:
                    for w in range(3):
                        wires[circuit.n_inputs + 3 * h + w][ri[r0 + s_]] = got[at:at + len(s_), w]
                    at += len(s_)
            call += 1
        for k, g in enumerate(nodes):
            sl = np.flatnonzero(rk == k)   # (every instance in order, or those of a masked node's lanes)
            for w in range(3):
                wires[circuit.n_inputs + 3 * g + w] = np.zeros((inst, row), dtype=np.uint64)
                wires[circuit.n_inputs + 3 * g + w][ri[sl]] = res[sl, w]
            if circuit.kind(g) not in ("classic", "lut", "data"):
                wires[circuit.n_inputs + 3 * g + 2][ri[sl]] = (x[sl] + y[sl] - np.uint64(2) * res[sl, 0]) & mask
    out = np.stack([val(ref, d) for ref, d in zip(circuit.outputs, circuit.output_shifts)]) if circuit.outputs \
        else np.zeros((0, inst, row), np.uint64)
    if not _next:
        return out
    # the registers' next states: NOT at the register's own codeword Dr >> scale
    nxt = [val(ref, d, (r // 4) >> k) for ref, d, k in zip(circuit.next_refs, circuit.next_shifts, circuit.reg_scales)]
    return out, np.array(nxt, dtype=np.uint64).reshape(circuit.n_regs, inst, row), call


def replay_steps(circuit, state, stream, r, boot, boot_lut=None, data=None, emit=None):
    """A stepped run (sgfhe_circuit_run_steps) composed on the host from replay_levels: state [registers][instances][n + 1]
    (None: every register FALSE), stream [steps][stream inputs][instances][n + 1], data [steps][planes][instances],
    emit [steps] (None: every step) -> (outputs [emitted steps][n_outputs][instances][n + 1], the state after the last
    step).  Step s is replay_levels on (state ++ stream[s]) with data[s]; `call` goes on counting from step to step; the
    outputs are taken before the feedback.  boot, boot_lut: as in replay_levels.  A checking aid, like replay_levels."""
    stream = np.asarray(stream, dtype=np.uint64)
    steps, inst, row = stream.shape[0], stream.shape[2], stream.shape[3]
    state = np.zeros((circuit.n_regs, inst, row), dtype=np.uint64) if state is None else \
        np.asarray(state, dtype=np.uint64).reshape(circuit.n_regs, inst, row)
    data = check_step_data(circuit, data, steps, inst)
    outs, call = [], 0
    for s in range(steps):
        out, state, call = replay_levels(circuit, np.concatenate([state, stream[s]]), r, boot, boot_lut,
                                         data=None if data is None else data[s], call0=call, _next=True)
        if emit is None or emit[s]:
            outs.append(out)
    return (np.stack(outs) if outs else np.zeros((0, circuit.n_outputs, inst, row), np.uint64)), state


def pack_calls(n):
    """Ciphertexts per pack call of sgfhe_circuit_run_ct: max(1, CALL_ROWS / n)."""
    return max(1, CALL_ROWS // n)


def replay_ct(circuit, a, b, params, boot, pack, boot_lut=None, data=None):
    """sgfhe_circuit_run_ct composed on the host: a, b [n_inputs][blocks][N] (N = n or m) -> ((w, v), lwe) with
    w, v [n_outputs][blocks][m] and lwe [n_outputs][blocks * n][n + 1].  The inputs are split with
    scheme.split_ciphertext_array (instance block * n + i = bit i of the block's ciphertext), the levels run
    through replay_levels and `boot`, and the ciphertexts q = output * blocks + block are packed in ascending
    order, pack_calls(n) at a time, by `pack(call, a, b)` (a [count][n][n], b [count][n] -> (w, v), each
    [count][m]); `call` goes on counting after the levels' calls.  boot_lut, data: as in replay_levels.  A checking and
    measuring aid."""
    n, m = params.n, params.m
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    blocks = a.shape[1]
    inputs = split_ciphertext_array(a, b, n, params.r).reshape(circuit.n_inputs, blocks * n, n + 1)
    calls = [0]

    def counted(call, *args):
        calls[0] = call + 1
        return boot(call, *args)

    def counted_lut(call, *args):
        calls[0] = call + 1
        return boot_lut(call, *args)

    lwe = replay_levels(circuit, inputs, params.r, counted, counted_lut, data=data)
    groups = lwe.reshape(circuit.n_outputs * blocks, n, n + 1)
    w = np.zeros((len(groups), m), dtype=np.uint64)
    v = np.zeros((len(groups), m), dtype=np.uint64)
    cpc, call = pack_calls(n), calls[0]
    for q0 in range(0, len(groups), cpc):
        g = groups[q0:q0 + cpc]
        w[q0:q0 + cpc], v[q0:q0 + cpc] = pack(call, np.ascontiguousarray(g[:, :, :n]), np.ascontiguousarray(g[:, :, n]))
        call += 1
    shape = (circuit.n_outputs, blocks, m)
    return (w.reshape(shape), v.reshape(shape)), lwe


# ---- residues mod Q as [..., 2] uint64 {lo, hi}: the few operations the direct replay needs, vectorised --------

def _split128(x):
    x = np.asarray(x, dtype=np.uint64)
    return x[..., 0], x[..., 1]


def _const128(v):
    return np.uint64(v & 0xFFFFFFFFFFFFFFFF), np.uint64(v >> 64)


def _ge128(al, ah, bl, bh):
    return (ah > bh) | ((ah == bh) & (al >= bl))


def _sub128(al, ah, bl, bh):
    return al - bl, ah - bh - (al < bl).astype(np.uint64)


def _add128(al, ah, bl, bh):
    lo = al + bl
    return lo, ah + bh + (lo < al).astype(np.uint64)


def modred_words(x, Q, r):
    """ModRed (src/fhe.jl:616-618,644-648; rescale, utils.jl:78-92) of residues [..., 2] uint64 {lo, hi} in [0, Q),
    Q < 2^94, to words of [0, r), r a power of two up to 2^15: round(x r / Q) mod r, halves up."""
    lo, hi = _split128(x)
    logr = np.uint64(r.bit_length() - 1)
    nl, nh = lo << logr, (hi << logr) | (lo >> (np.uint64(64) - logr))            # x r < 2^109
    # the quotient to within one from doubles, then the exact remainder x r - q Q in 128-bit wrap-around words
    q = np.floor((hi.astype(np.float64) * 2.0 ** 64 + lo.astype(np.float64)) * (float(r) / float(Q))).astype(np.uint64)
    Ql, Qh = _const128(Q)
    t0, t1 = q * (Ql & np.uint64(0xFFFFFFFF)), q * (Ql >> np.uint64(32))           # q < 2^16: below 2^48 each
    pl, ph = _add128(t0, q * Qh, t1 << np.uint64(32), t1 >> np.uint64(32))
    rl, rh = _sub128(nl, nh, pl, ph)
    neg = rh >> np.uint64(63) != 0                                                 # q one too large
    al, ah = _add128(rl, rh, Ql, Qh)
    rl, rh, q = np.where(neg, al, rl), np.where(neg, ah, rh), np.where(neg, q - np.uint64(1), q)
    big = _ge128(rl, rh, Ql, Qh)                                                   # q one too small
    sl, sh = _sub128(rl, rh, Ql, Qh)
    rl, rh, q = np.where(big, sl, rl), np.where(big, sh, rh), np.where(big, q + np.uint64(1), q)
    q = q + _ge128(rl, rh, *_const128(Q // 2 + (Q & 1))).astype(np.uint64)         # utils.jl:84
    return q & np.uint64(r - 1)                                                    # utils.jl:86-88


def lift_words(x, Q, r):
    """The lift of words of Z_r to residues of Z_Q by exact scaling (sgfhe_lwe_lift_modq, k_circ_lift): x [...] uint64
    in [0, r), r a power of two up to 2^15, Q < 2^94 -> floor((x Q + r/2) / r) as [..., 2] uint64 {lo, hi}.  It maps a
    wrap of r to a wrap of Q and Dr to Q/4, and modred_words of it is x; the error of an LWE is carried on."""
    x = np.asarray(x, dtype=np.uint64)
    logr = np.uint64(r.bit_length() - 1)
    Ql, Qh = _const128(Q)
    t0, t1 = x * (Ql & np.uint64(0xFFFFFFFF)), x * (Ql >> np.uint64(32))           # x < 2^15: below 2^47 each
    pl, ph = _add128(t0, x * Qh, t1 << np.uint64(32), t1 >> np.uint64(32))         # x Q < 2^109
    pl, ph = _add128(pl, ph, np.uint64(r // 2), np.uint64(0))
    return np.stack([(pl >> logr) | (ph << (np.uint64(64) - logr)), ph >> logr], axis=-1)


def lwe_not_modq(x, Q, DQ_tilde):
    """NOT of un-reduced LWEs [..., n + 1][2] over Z_Q: enc_trivial(true) - w with true = (0, 2 DQ_tilde):
    a -> -a, b -> 2 DQ_tilde - b, mod Q."""
    lo, hi = _split128(x)
    Ql, Qh = _const128(Q)
    ml, mh = _sub128(Ql, Qh, lo, hi)                                               # Q - a, 0 stays 0
    zero = (lo == 0) & (hi == 0)
    out = np.stack([np.where(zero, lo, ml), np.where(zero, hi, mh)], axis=-1)
    Tl, Th = _const128((2 * DQ_tilde) % Q)
    bl, bh = lo[..., -1], hi[..., -1]
    dl, dh = _sub128(Tl, Th, bl, bh)
    under = ~_ge128(Tl, Th, bl, bh)
    el, eh = _add128(dl, dh, Ql, Qh)
    out[..., -1, 0], out[..., -1, 1] = np.where(under, el, dl), np.where(under, eh, dh)
    return out


def replay_ct_direct(circuit, a, b, params, boot_raw, tail, lift=False, boot_lut_raw=None, data=None):
    """sgfhe_circuit_run_ct_ex with SGFHE_CIRCUIT_PACK_DIRECT composed on the host: a, b [n_inputs][blocks][N] ->
    ((w, v), lwe) as replay_ct.  `boot_raw(call, a1, b1, a2, b2)` runs one call un-reduced and returns
    [rows][3][n + 1][2] residues mod Q; the levels run through it in the row and call order of replay_levels, their
    ModRed (modred_words) being what the next level reads and what `lwe` holds.  The pack stage takes the
    ciphertexts q = output * blocks + block in ascending order, pack_calls(n) at a time: a group's refreshed
    ciphertexts (outputs that name an input wire, the constant, an XOR3 wire or the LOW wire of a sum node, or carry a
    lane shift or route, or name a wire of a node with a lane mask) are bootstrapped as one call -- trivial 1 paired
    with every bit, row = rank among them * n + bit, AND rows kept -- and then `tail(call, lwe_q)` (lwe_q
    [count][n][n + 1][2] -> (w, v), each [count][m]) packs the group: the gate's own rows for a direct output, NOT
    over Z_Q applied (lwe_not_modq).  `call` counts every call from 0.  lift=True (SGFHE_CIRCUIT_PACK_LIFT): the
    ciphertexts that are not direct take lift_words of their `lwe` rows instead -- no `boot_raw` call in the pack stage,
    one call number per group.  boot_lut_raw(call, a, b, tables, idx): the LUT rows of a call as in replay_levels,
    un-reduced ([rows][3][n + 1][2]); an output naming wire +0 of a LUT node is refreshed or lifted.  data: as in
    replay_levels.  A checking and measuring aid."""
    n, m, r, Q = params.n, params.m, params.r, params.Q
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    blocks = a.shape[1]
    inst = blocks * n
    inputs = split_ciphertext_array(a, b, n, r).reshape(circuit.n_inputs, inst, n + 1)
    raws = {}           # by call: a call of LUT rows only has none (and no direct output names its rows)

    def reduced(call, *args):
        raws[call] = np.asarray(boot_raw(call, *args), dtype=np.uint64)
        return modred_words(raws[call], Q, r)

    def reduced_lut(call, *args):
        return modred_words(np.asarray(boot_lut_raw(call, *args), dtype=np.uint64), Q, r)

    lwe = replay_levels(circuit, inputs, r, reduced, reduced_lut, data=data)
    call, k, raw_wire = 0, 0, {}
    for nodes in circuit.schedule():                        # the calls of a level, back into the level's rows
        rk, ri = level_row_map(circuit, nodes, inst)
        rows = len(rk)
        calls = -(-rows // CALL_ROWS)
        level = np.concatenate([raws[k + j] if k + j in raws else
                                np.zeros((min(CALL_ROWS, rows - j * CALL_ROWS), 3, n + 1, 2), dtype=np.uint64)
                                for j in range(calls)])
        k += calls
        call = k
        for rank, g in enumerate(nodes):
            sl = np.flatnonzero(rk == rank)
            for w in range(3):
                raw_wire[circuit.n_inputs + 3 * g + w] = np.zeros((inst, n + 1, 2), dtype=np.uint64)
                raw_wire[circuit.n_inputs + 3 * g + w][ri[sl]] = level[sl, w]

    def is_direct(o):
        i = circuit.outputs[o] & ~NOT_BIT & 0xFFFFFFFF
        if i == FALSE_ID or i < circuit.n_inputs or circuit.output_shifts[o] != 0:
            return False
        g, w = divmod(i - circuit.n_inputs, 3)
        if g in circuit.gate_tables or g in circuit.gate_masks:   # wire +0 of a LUT node, a wire of a masked node:
            return False                                            # refreshed or lifted
        return not (w == 2 and circuit.kind(g) != "classic")   # XOR3 / LOW is linear over Z_r: no gate row over Z_Q

    n_ct, cpc = circuit.n_outputs * blocks, pack_calls(n)
    w = np.zeros((n_ct, m), dtype=np.uint64)
    v = np.zeros((n_ct, m), dtype=np.uint64)
    for q0 in range(0, n_ct, cpc):
        qs = range(q0, min(q0 + cpc, n_ct))
        group = np.zeros((len(qs), n, n + 1, 2), dtype=np.uint64)
        fresh = [q for q in qs if not is_direct(q // blocks)]
        if lift:
            for q in fresh:
                group[q - q0] = lift_words(lwe[q // blocks, (q % blocks) * n:(q % blocks + 1) * n], Q, r)
        elif fresh:
            y = np.concatenate([lwe[q // blocks, (q % blocks) * n:(q % blocks + 1) * n] for q in fresh])
            one = np.zeros_like(y)
            one[:, n] = r // 4
            res = np.asarray(boot_raw(call, one[:, :n], one[:, n], y[:, :n], y[:, n]), dtype=np.uint64)
            call += 1
            for rank, q in enumerate(fresh):
                group[q - q0] = res[rank * n:(rank + 1) * n, 0]
        for q in qs:
            o, t = q // blocks, q % blocks
            if is_direct(o):
                ref = circuit.outputs[o]
                rows = raw_wire[ref & ~NOT_BIT & 0xFFFFFFFF][t * n:(t + 1) * n]
                group[q - q0] = lwe_not_modq(rows, Q, params.DQ_tilde) if ref & NOT_BIT else rows
        w[q0:q0 + cpc], v[q0:q0 + cpc] = tail(call, group)
        call += 1
    shape = (circuit.n_outputs, blocks, m)
    return (w.reshape(shape), v.reshape(shape)), lwe


def evaluate_circuit_ct(bkey, rng, circuit, cts, direct=False, lift=False, data=None):
    """The circuit on RLWE ciphertexts, the reference's user flow (encrypt -> split_ciphertext -> gates ->
    pack_encrypted_bits -> decrypt) with the split and the pack on the device (Engine.circuit_run_ct).
    cts: [n_inputs][blocks] of PackedCiphertext or Ciphertext (all of one kind); bit i of a ciphertext is
    instance i of its block.  rng as in evaluate_circuit.  direct=True: outputs that name a gate wire are packed
    from the gate's LWEs over Z_Q without the refresh bootstraps (SGFHE_CIRCUIT_PACK_DIRECT); they decrypt alike.
    lift=True: that, and every other output is lifted from Z_r instead of refreshed (SGFHE_CIRCUIT_PACK_LIFT): no
    bootstrap in the pack stage, but such an output carries its wire's error on -- meant for inputs that are themselves
    packed outputs, not for sums of freshly encrypted bits (the noise rule in include/sgfhe_hip.h).
    A circuit with lane groups needs n to be a multiple of its group: a ciphertext then holds n / group words.
    data: the planes of a circuit that has any, uint8 [planes][blocks * n] (instance block * n + i is bit i of a block).
    Returns [n_outputs][blocks] of Ciphertext."""
    p = bkey.params
    if len(cts) != circuit.n_inputs:
        raise ValueError("evaluate_circuit_ct: one row of ciphertexts per input wire")
    blocks = len(cts[0]) if cts else 0
    flat = [ct for row in cts for ct in row]
    if any(len(row) != blocks for row in cts):
        raise ValueError("ragged inputs: every input needs one ciphertext per block")
    if not flat:
        raise ValueError("evaluate_circuit_ct: at least one input ciphertext is needed (it fixes the blocks)")
    kind = type(flat[0])
    if kind not in (PackedCiphertext, Ciphertext) or any(type(ct) is not kind for ct in flat):
        raise TypeError("evaluate_circuit_ct: PackedCiphertext or Ciphertext, all of one kind")
    N = p.n if kind is PackedCiphertext else p.m
    a = np.stack([np.asarray(ct.rlwe.a, dtype=np.uint64) for ct in flat]).reshape(circuit.n_inputs, blocks, -1)
    b = np.stack([np.asarray(ct.rlwe.b, dtype=np.uint64) for ct in flat]).reshape(circuit.n_inputs, blocks, -1)
    if a.shape[2] != N or b.shape[2] != N:
        raise ValueError("evaluate_circuit_ct: ciphertext polynomials of length %d expected" % N)
    with bkey.engine.lock:                       # mode and run stay together (threads sharing a key)
        _set_flatten_mode(bkey, rng)
        w, v = bkey.engine.circuit_run_ct(circuit, a, b, direct=direct, lift=lift, data=data)
    return [[Ciphertext(p, RLWE(w[o, t], v[o, t])) for t in range(blocks)] for o in range(circuit.n_outputs)]


def _input_array(circuit, inputs, n):
    """[n_inputs][instances] of EncryptedBit -> the array form [n_inputs][instances][n + 1] uint64."""
    arr = np.zeros((circuit.n_inputs, len(inputs[0]) if circuit.n_inputs else 0, n + 1), dtype=np.uint64)
    for i, row in enumerate(inputs):
        if len(row) != arr.shape[1]:
            raise ValueError("ragged inputs: every input needs one EncryptedBit per instance")
        for t, e in enumerate(row):
            arr[i, t, :n] = e.lwe.a
            arr[i, t, n] = e.lwe.b
    return arr


def probe_circuit(bkey, key, rng, circuit, inputs, bits, data=None):
    """evaluate_circuit that also measures the LWE error of every wire on the device (Engine.circuit_probe,
    sgfhe_circuit_run_probe).  A DIAGNOSTIC for parameter studies and tests: `key` is the PrivateKey, and its
    bits cross the library boundary.  inputs as evaluate_circuit; bits [n_inputs][instances]: the plaintext of
    every input; data as evaluate_circuit.  Returns (outputs, stats): outputs as evaluate_circuit (the same bytes), stats a list of
    engine.NoiseStats by wire id (noise_report formats it)."""
    n = bkey.params.n
    as_bits = not isinstance(inputs, np.ndarray)
    if as_bits:
        inputs = _input_array(circuit, inputs, n)
    bits = np.asarray(bits).astype(np.uint8).reshape(circuit.n_inputs, -1)
    with bkey.engine.lock:                       # mode and run stay together (threads sharing a key)
        _set_flatten_mode(bkey, rng)
        out, stats = bkey.engine.circuit_probe(circuit, inputs, key.key, bits, data=data)
    if as_bits:
        out = [[EncryptedBit(LWE(out[o, t, :n], out[o, t, n])) for t in range(out.shape[1])]
               for o in range(out.shape[0])]
    return out, stats


def noise_report(circuit, stats):
    """The records of probe_circuit by wire: a list of dicts (wire, kind: "input" / "AND" / "OR" / "XOR", or "MAJ" /
    "ONE_OR_TWO" / "XOR3" for the wires of a three-input node, "HI" / "MID" / "LOW" for those of a sum node, node,
    level (0 for inputs), rows, wrong, max_abs, mean, rms, margin), the wires of pruned nodes left out, sorted
    by max |e| (largest first), then level."""
    level = {}
    for L, nodes in enumerate(circuit.schedule(), start=1):
        for g in nodes:
            level[g] = L
            for h in circuit.siblings(g):
                level[h] = L
    rows = []
    for wire, st in enumerate(stats):
        if st.rows == 0:
            continue
        g = (wire - circuit.n_inputs) // 3 if wire >= circuit.n_inputs else None
        names = ("AND", "OR", "XOR") if g is None else \
            {"classic": ("AND", "OR", "XOR"), "gate3": ("MAJ", "ONE_OR_TWO", "XOR3"), "sum": ("HI", "MID", "LOW"),
             "lut": ("F", "F_HALF", "F_QUARTER"), "sibling": ("F", "F_HALF", "F_QUARTER"),
             "data": ("F", "F_HALF", "F_QUARTER"), "data_sibling": ("F", "F_HALF", "F_QUARTER")}[circuit.kind(g)]
        kind = "input" if g is None else names[(wire - circuit.n_inputs) % 3]
        rows.append(dict(wire=wire, kind=kind, node=g, level=0 if g is None else level[g], rows=st.rows,
                         wrong=st.wrong, max_abs=st.max_abs, mean=st.sum / st.rows,
                         rms=(st.sum_sq / st.rows) ** 0.5, margin=st.margin))
    rows.sort(key=lambda d: (-d["max_abs"], d["level"], d["wire"]))
    return rows


def evaluate_circuit(bkey, rng, circuit, inputs, data=None):
    """The circuit over many instances on the HIP engine.  rng = None: deterministic flatten; a numpy
    Generator: randomised flatten (its ChaCha8 key drawn from `rng`, call counter from 0).
    inputs: [n_inputs][instances] of EncryptedBit, or the array form [n_inputs][instances][n + 1] uint64.
    data: the planes of a circuit that has any (Circuit(planes=P)), uint8 [P][instances].
    Returns [n_outputs][instances] of EncryptedBit (the array form when given the array form)."""
    n = bkey.params.n
    as_bits = not isinstance(inputs, np.ndarray)
    if as_bits:
        inputs = _input_array(circuit, inputs, n)
    with bkey.engine.lock:                       # mode and run stay together (threads sharing a key)
        _set_flatten_mode(bkey, rng)
        out = bkey.engine.circuit_run(circuit, inputs, data=data)
    if not as_bits:
        return out
    return [[EncryptedBit(LWE(out[o, t, :n], out[o, t, n])) for t in range(out.shape[1])]
            for o in range(out.shape[0])]


def evaluate_circuit_steps(bkey, rng, circuit, state, stream, data=None, emit=None):
    """A circuit with registers over many instances and many steps on the HIP engine (Engine.circuit_run_steps): one
    queued run, the registers fed back on the device.  rng as in evaluate_circuit.
    state: [registers][instances] of EncryptedBit, the array form [registers][instances][n + 1], or None (every register
    FALSE); stream: [steps][stream inputs][instances] of EncryptedBit or the array form [steps][stream inputs]
    [instances][n + 1]; data: uint8 [steps][planes][instances] for a circuit with planes; emit: [steps] of bool, the steps
    whose outputs are wanted (None: all).
    Returns (outputs [emitted steps][n_outputs][instances], state [registers][instances] after the last step), of
    EncryptedBit -- in the array form when `stream` came in the array form."""
    n = bkey.params.n
    as_bits = not isinstance(stream, np.ndarray)

    def arr(rows, count):   # [count][instances] of EncryptedBit -> [count][instances][n + 1]
        out = np.zeros((count, len(rows[0]) if count else 0, n + 1), dtype=np.uint64)
        for i, row_ in enumerate(rows):
            if len(row_) != out.shape[1]:
                raise ValueError("ragged inputs: one EncryptedBit per instance")
            for t, e in enumerate(row_):
                out[i, t, :n] = e.lwe.a
                out[i, t, n] = e.lwe.b
        return out

    def bits(a):
        return [[EncryptedBit(LWE(row_[t, :n], row_[t, n])) for t in range(row_.shape[0])] for row_ in a]

    if as_bits:
        stream = np.stack([arr(step, circuit.n_inputs - circuit.n_regs) for step in stream])
    if state is not None and not isinstance(state, np.ndarray):
        state = arr(state, circuit.n_regs)
    with bkey.engine.lock:                       # mode and run stay together (threads sharing a key)
        _set_flatten_mode(bkey, rng)
        out, st = bkey.engine.circuit_run_steps(circuit, state, stream, data=data, emit=emit)
    if not as_bits:
        return out, st
    return [bits(step) for step in out], bits(st)


def evaluate_circuit_steps_ct(bkey, rng, circuit, state_cts, stream_cts, direct=False, lift=False, data=None, emit=None):
    """A stepped run on RLWE ciphertexts (Engine.circuit_run_steps_ct): every step's stream ciphertexts are split on
    the device, every emitted step's outputs packed on the device; the registers stay on the device in between.
    state_cts: [registers][blocks] of PackedCiphertext or Ciphertext, or None (every register FALSE); stream_cts:
    [steps][stream inputs][blocks], all of one kind; direct, lift: as evaluate_circuit_ct; data: uint8
    [steps][planes][blocks * n]; emit: as evaluate_circuit_steps.  Registers of scale 0 only.
    Returns (outputs [emitted steps][n_outputs][blocks] of Ciphertext, state): the state after the last step as the
    LWE array [registers][blocks * n][n + 1] (feed it to evaluate_circuit_steps, or pack it)."""
    p = bkey.params
    flat = [ct for step in stream_cts for row_ in step for ct in row_] + [ct for row_ in (state_cts or []) for ct in row_]
    if not flat:
        raise ValueError("evaluate_circuit_steps_ct: at least one ciphertext is needed (it fixes the blocks)")
    kind = type(flat[0])
    if kind not in (PackedCiphertext, Ciphertext) or any(type(ct) is not kind for ct in flat):
        raise TypeError("evaluate_circuit_steps_ct: PackedCiphertext or Ciphertext, all of one kind")
    N = p.n if kind is PackedCiphertext else p.m

    def ab(rows, lead):   # nested lists of ciphertexts -> a, b [lead..][blocks][N]
        cts = np.array([[np.asarray(ct.rlwe.a, dtype=np.uint64), np.asarray(ct.rlwe.b, dtype=np.uint64)] for ct in rows],
                       dtype=np.uint64).reshape(lead + (-1, 2, N))
        return np.ascontiguousarray(cts[..., 0, :]), np.ascontiguousarray(cts[..., 1, :])

    n_stream = circuit.n_inputs - circuit.n_regs
    a, b = ab([ct for step in stream_cts for row_ in step for ct in row_], (len(stream_cts), n_stream))
    sa = sb = None
    if state_cts is not None:
        sa, sb = ab([ct for row_ in state_cts for ct in row_], (circuit.n_regs,))
    with bkey.engine.lock:                       # mode and run stay together (threads sharing a key)
        _set_flatten_mode(bkey, rng)
        (w, v), st = bkey.engine.circuit_run_steps_ct(circuit, sa, sb, a, b, N=N, direct=direct, lift=lift, data=data,
                                                      emit=emit)
    return [[[Ciphertext(p, RLWE(w[s, o, t], v[s, o, t])) for t in range(w.shape[2])] for o in range(w.shape[1])]
            for s in range(w.shape[0])], st
