// Host-side planner of sgfhe_circuit_* (include/sgfhe_hip.h): validates a gate
// graph, prunes the nodes no output depends on, levels the rest ASAP, gives every wire that is read a
// slot of the device wire table by liveness, and fixes the row and call numbering of a run; circuit_plain_bits
// evaluates a planned circuit in clear for the noise probe.  Plain C++, no HIP: tests/native/circuit_plan_sanitized.cpp,
// circuit_bits_sanitized.cpp, circuit_lanes_sanitized.cpp, circuit_gate3_sanitized.cpp and circuit_wsum_sanitized.cpp
// drive it under ASan / UBSan on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <new>
#include <queue>
#include <vector>

#include "../../include/sgfhe_hip.h"

namespace sgfhe {

// A wire id below 2^31 - 1 (0x7FFFFFFF is the constant FALSE), bit 31 = NOT.  Slot references in the
// device tables use the same encoding with slot numbers in place of wire ids.
constexpr uint32_t CIRC_FALSE = SGFHE_CIRCUIT_FALSE;
constexpr uint32_t CIRC_NOT = SGFHE_CIRCUIT_NOT;
constexpr uint32_t CIRC_NONE = 0xFFFFFFFFu;     // out_slot of a gate output nothing reads
constexpr uint32_t CIRC_NO_INPUT = SGFHE_CIRCUIT_NONE;   // third reference of a two-input node (never a wire id)

struct CircuitPlan {
    uint32_t n_inputs = 0, n_gates = 0, n_outputs = 0;
    uint32_t levels = 0, widest = 0, slots = 0;
    uint32_t group = 1;                 // lane group size G (sgfhe_circuit_create_lanes); 1: no reference is shifted
    std::vector<uint32_t> level;        // [n_gates]: level of every node, 0 = pruned
    std::vector<uint32_t> order;        // live nodes, level by level, ascending index within a level
    std::vector<uint32_t> level_start;  // [levels + 2]: level L's nodes are order[level_start[L] .. level_start[L + 1])
                                        // (level 0 holds none: level_start[0] == level_start[1] == 0)
    std::vector<uint32_t> input_slot;   // [n_inputs]: slot of every input wire, CIRC_NONE if nothing reads it
    // Device tables, one entry per live node in `order`, uploaded once per run:
    std::vector<uint32_t> in_ref;       // [live][2]: the node's inputs as slot references (CIRC_NOT, CIRC_FALSE)
    std::vector<uint32_t> out_slot;     // [live][3]: slot of its AND / OR / XOR wire, CIRC_NONE if unread
                                        // (MAJ / ONE_OR_TWO / XOR3 of a three-input node)
    std::vector<uint32_t> out_ref;      // [n_outputs]: the circuit's outputs as slot references
    // Lane shifts, beside in_ref / out_ref (uploaded when lanes()): the reference reads instance t + d of its slot
    // where 0 <= t % group + d < group, the constant FALSE elsewhere; 0 on every reference to the constant
    std::vector<int32_t> in_shift;      // [live][2]
    std::vector<int32_t> out_shift;     // [n_outputs]
    // Three-input nodes (sgfhe_circuit_create3), beside in_ref / in_shift / in_row and uploaded when three > 0: the
    // third reference of every live node, CIRC_NO_INPUT for a two-input node (its shift and probe row are then 0 and
    // CIRC_NO_INPUT)
    uint32_t three = 0;                 // live three-input nodes
    std::vector<uint32_t> in_ref3;      // [live]
    std::vector<int32_t> in_shift3;     // [live]
    std::vector<uint32_t> in_row3;      // [live]
    std::vector<uint32_t> three_before; // [live + 1]: three-input nodes among order[0 .. k)
    // Weighted-sum nodes (sgfhe_circuit_create_w).  A sum node of two or three unit weights IS a three-input node
    // (x, y, FALSE) or (x, y, z) and is planned as one.  Every other sum node is a WIDE node: in_ref / in_shift /
    // in_row name the constant FALSE twice and in_ref3 names it once -- any reference but CIRC_NO_INPUT marks the
    // node for the XOR3 kernels, which compute its LOW wire -- and its terms are in the CSR tables below.  Those
    // exist when wide > 0 and then cover EVERY live node, a classic or three-input one with its two or three unit
    // terms, so that one gather (k_circ_gather_w) serves a whole level.
    uint32_t wide = 0;                  // live wide nodes
    std::vector<uint32_t> w_start;      // [live + 1]: node k's terms are w_ref[w_start[k] .. w_start[k + 1])
    std::vector<uint32_t> w_ref;        // [terms]: slot references
    std::vector<int32_t> w_shift;       // [terms]
    std::vector<int32_t> w_weight;      // [terms]: -2, -1, 1, 2
    std::vector<uint32_t> w_row;        // [terms], host only: the terms as probe rows (as in_row)
    // Host only (SGFHE_CIRCUIT_PACK_DIRECT): where an output that names a gate wire is produced
    std::vector<uint32_t> out_node;     // [n_outputs]: index in `order` of the producing node, CIRC_NONE for an input
                                        // wire, the constant, a lane-shifted reference or the XOR3 wire of a
                                        // three-input node (the LOW wire of a sum node), which is no gate row over
                                        // Z_Q (those are refreshed)
    std::vector<uint32_t> out_gate;     // [n_outputs]: 0 AND, 1 OR, 2 XOR (0 where out_node is CIRC_NONE)
    // Host only (sgfhe_circuit_run_probe): the node's inputs as PROBE ROWS -- row i < n_inputs is input wire i, row
    // n_inputs + 3 k + w is wire w of the k-th live node in `order` -- with CIRC_NOT and CIRC_FALSE as in a reference
    std::vector<uint32_t> in_row;       // [live][2]

    size_t live() const { return order.size(); }
    // the run takes the lane kernels (group 1 admits no shift but 0)
    bool lanes() const { return group > 1; }
    // the run takes the three-reference gather and the XOR3 kernels
    bool gate3() const { return three > 0; }
    // the levels of the run take the CSR gather
    bool wsum() const { return wide > 0; }
    // live nodes order[ka .. kb] hold a three-input node
    bool gate3_in(uint32_t ka, uint32_t kb) const { return three && three_before[kb + 1] != three_before[ka]; }
    // rows of level L in a run over `instances`; row = rank_in_level * instances + instance
    uint64_t level_rows(uint32_t L, uint64_t instances) const {
        return (uint64_t)(level_start[L + 1] - level_start[L]) * instances;
    }
};

namespace circuit_detail {
inline uint32_t wire_id(uint32_t ref) { return ref & ~CIRC_NOT; }
}  // namespace circuit_detail

// One view of the nodes' inputs behind every entry.  `arity` 2 or 3: the [n_gates][arity] arrays of
// sgfhe_circuit_create_lanes / sgfhe_circuit_create3 (a third reference CIRC_NO_INPUT leaves a two-input node; with
// one, the node is the sum node of three unit weights).  `arity` 0: the CSR arrays of sgfhe_circuit_create_w.  Term i
// of the circuit is refs[i], shifts[i] (NULL: 0), weights[i] (NULL: 1); node g's terms are first(g) .. first(g) +
// count(g).
struct CircuitNodes {
    int arity;
    const uint32_t *refs;
    const int32_t *shifts;
    const uint32_t *kind = nullptr, *start = nullptr;
    const int32_t *weights = nullptr;

    size_t first(size_t g) const { return arity ? (size_t)arity * g : start[g]; }
    size_t count(size_t g) const {
        if (!arity) return (size_t)start[g + 1] - start[g];
        return arity == 3 && refs[3 * g + 2] != CIRC_NO_INPUT ? 3 : 2;
    }
    bool classic(size_t g) const { return arity ? count(g) == 2 : kind[g] == 0; }
    int32_t weight(size_t i) const { return weights ? weights[i] : 1; }
    // a sum node that is no three-input node: something other than two or three unit weights
    bool wide(size_t g) const {
        if (classic(g)) return false;
        const size_t n = count(g);
        if (n != 2 && n != 3) return true;
        for (size_t i = first(g); i < first(g) + n; i++)
            if (weight(i) != 1) return true;
        return false;
    }
};

// Builds `P` from the nodes `N` (gate shifts / out_shift NULL: all 0).  Returns SGFHE_OK, SGFHE_ERR_INVALID_ARG for a
// malformed circuit, SGFHE_ERR_OOM when an allocation fails.  Nothing throws out of it, and a refused circuit costs no
// allocation.
inline int32_t circuit_plan_nodes(uint32_t n_inputs, const CircuitNodes &N, size_t n_gates, const uint32_t *outputs,
                                  const int32_t *out_shift, size_t n_outputs, uint32_t group, CircuitPlan &P) noexcept {
    using circuit_detail::wire_id;
    const uint32_t *refs = N.refs;
    const int32_t *gate_shift = N.shifts;
    // ---- validate: every size below 2^31, wire ids below the constant, inputs name earlier wires only,
    // every shift inside the group (in 64 bits: -INT32_MIN does not exist).  CIRC_NO_INPUT is above every wire id, so
    // anywhere but beside a two-input node of the [n_gates][3] arrays it fails the id checks below.
    if (n_outputs < 1 || !outputs || (n_gates && !refs) || group < 1) return SGFHE_ERR_INVALID_ARG;
    auto shift_ok = [&](int32_t d) { return (d < 0 ? -(int64_t)d : (int64_t)d) < (int64_t)group; };
    if (n_inputs >= 0x80000000u || n_gates >= 0x80000000u || n_outputs >= 0x80000000u) return SGFHE_ERR_INVALID_ARG;
    const uint64_t n_wires = (uint64_t)n_inputs + 3 * (uint64_t)n_gates;
    if (n_wires >= CIRC_FALSE) return SGFHE_ERR_INVALID_ARG;
    if (!N.arity) {   // the CSR itself, node by node, before a term of the node is read
        if (n_gates && (!N.kind || !N.start || !N.weights || N.start[0] != 0)) return SGFHE_ERR_INVALID_ARG;
        for (size_t g = 0; g < n_gates; g++) {
            if (N.kind[g] > 1 || N.start[g + 1] < N.start[g]) return SGFHE_ERR_INVALID_ARG;
            const size_t nj = N.count(g);
            if (N.kind[g] == 0 ? nj != 2 : (nj < 1 || nj > SGFHE_CIRCUIT_MAX_TERMS)) return SGFHE_ERR_INVALID_ARG;
            for (size_t i = N.first(g); i < N.first(g) + nj; i++) {
                const int32_t w = N.weights[i];
                if (N.kind[g] == 0 ? w != 1 : (w == 0 || w < -2 || w > 2)) return SGFHE_ERR_INVALID_ARG;
            }
        }
    }
    for (size_t g = 0; g < n_gates; g++)
        for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
            const uint32_t id = wire_id(refs[i]);
            if (id == CIRC_FALSE || id < n_inputs) continue;
            if (id >= n_wires || (id - n_inputs) / 3 >= g) return SGFHE_ERR_INVALID_ARG;   // own or later node
        }
    for (size_t o = 0; o < n_outputs; o++) {
        const uint32_t id = wire_id(outputs[o]);
        if (id != CIRC_FALSE && id >= n_wires) return SGFHE_ERR_INVALID_ARG;
    }
    for (size_t g = 0; gate_shift && g < n_gates; g++)   // (the shift beside CIRC_NO_INPUT is ignored)
        for (size_t i = N.first(g), end = i + N.count(g); i < end; i++)
            if (!shift_ok(gate_shift[i])) return SGFHE_ERR_INVALID_ARG;
    for (size_t o = 0; out_shift && o < n_outputs; o++)
        if (!shift_ok(out_shift[o])) return SGFHE_ERR_INVALID_ARG;
    try {
        P = CircuitPlan();
        P.n_inputs = n_inputs;
        P.n_gates = (uint32_t)n_gates;
        P.n_outputs = (uint32_t)n_outputs;
        P.group = group;
        const uint32_t NG = (uint32_t)n_gates;
        auto node_of = [&](uint32_t id) -> int64_t {   // producing node of a wire, -1 for inputs and the constant
            return (id == CIRC_FALSE || id < n_inputs) ? -1 : (int64_t)((id - n_inputs) / 3);
        };
        // ---- prune: a node is live when an output reaches it (walk back from the outputs, last node first)
        std::vector<uint8_t> live(NG, 0);
        for (size_t o = 0; o < n_outputs; o++) {
            const int64_t g = node_of(wire_id(outputs[o]));
            if (g >= 0) live[g] = 1;
        }
        for (uint32_t g = NG; g-- > 0;) {
            if (!live[g]) continue;
            for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
                const int64_t h = node_of(wire_id(refs[i]));
                if (h >= 0) live[h] = 1;
            }
        }
        // ---- level ASAP: 1 + the largest level of its input nodes (inputs and the constant: 0)
        P.level.assign(NG, 0);
        for (uint32_t g = 0; g < NG; g++) {
            if (!live[g]) continue;
            uint32_t L = 0;
            for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
                const int64_t h = node_of(wire_id(refs[i]));
                if (h >= 0) L = std::max(L, P.level[h]);
            }
            P.level[g] = L + 1;
            P.levels = std::max(P.levels, L + 1);
        }
        // ---- order: level by level, ascending node index within a level (counting sort)
        P.level_start.assign((size_t)P.levels + 2, 0);
        for (uint32_t g = 0; g < NG; g++)
            if (P.level[g]) P.level_start[P.level[g] + 1]++;
        for (uint32_t L = 1; L <= P.levels; L++) {
            P.widest = std::max(P.widest, P.level_start[L + 1]);
            P.level_start[L + 1] += P.level_start[L];
        }
        P.order.resize(P.level_start[P.levels + 1]);
        {
            std::vector<uint32_t> fill(P.level_start.begin(), P.level_start.end() - 1);
            for (uint32_t g = 0; g < NG; g++)
                if (P.level[g]) P.order[fill[P.level[g]]++] = g;
        }
        // ---- liveness: the last level that reads each wire (outputs: beyond the last level)
        const uint32_t END = P.levels + 1;
        constexpr uint32_t UNREAD = 0;   // no wire is read at level 0
        std::vector<uint32_t> last_read((size_t)n_wires, UNREAD);
        for (uint32_t g : P.order)
            for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
                const uint32_t id = wire_id(refs[i]);
                if (id != CIRC_FALSE) last_read[id] = std::max(last_read[id], P.level[g]);
            }
        for (size_t o = 0; o < n_outputs; o++) {
            const uint32_t id = wire_id(outputs[o]);
            if (id != CIRC_FALSE) last_read[id] = END;
        }
        // ---- slots: a wire written at level L takes the lowest free slot; a slot is free again after the
        // last level that reads its wire (so no call of level L overwrites what a later call of L gathers)
        std::vector<uint32_t> slot_of((size_t)n_wires, CIRC_NONE);
        std::vector<std::vector<uint32_t>> release((size_t)END + 1);   // slots freed after level L
        std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_slots;
        auto take = [&](uint32_t id) {
            uint32_t s;
            if (free_slots.empty()) s = P.slots++;
            else { s = free_slots.top(); free_slots.pop(); }
            slot_of[id] = s;
            release[last_read[id]].push_back(s);
        };
        P.input_slot.assign(n_inputs, CIRC_NONE);
        for (uint32_t i = 0; i < n_inputs; i++)
            if (last_read[i] != UNREAD) { take(i); P.input_slot[i] = slot_of[i]; }
        for (uint32_t L = 1; L <= P.levels; L++) {
            for (uint32_t s : release[L - 1]) free_slots.push(s);
            for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++)
                for (uint32_t w = 0; w < 3; w++) {
                    const uint32_t id = n_inputs + 3 * P.order[k] + w;
                    if (last_read[id] != UNREAD) take(id);
                }
        }
        // ---- device tables.  The term a table entry comes from: term j of node g, or none (SIZE_MAX: the constant
        // FALSE) -- both entries of a wide node, whose terms are in the CSR tables alone
        auto term_of = [&](size_t g, int j) -> size_t {
            return N.wide(g) || (size_t)j >= N.count(g) ? SIZE_MAX : N.first(g) + (size_t)j;
        };
        auto slot_ref = [&](uint32_t ref) -> uint32_t {
            const uint32_t id = wire_id(ref);
            return (id == CIRC_FALSE ? CIRC_FALSE : slot_of[id]) | (ref & CIRC_NOT);
        };
        P.in_ref.resize(2 * P.live());
        P.out_slot.resize(3 * P.live());
        for (size_t k = 0; k < P.live(); k++) {
            const uint32_t g = P.order[k];
            for (int j = 0; j < 2; j++) {
                const size_t i = term_of(g, j);
                P.in_ref[2 * k + j] = i == SIZE_MAX ? CIRC_FALSE : slot_ref(refs[i]);
            }
            for (uint32_t w = 0; w < 3; w++) P.out_slot[3 * k + w] = slot_of[n_inputs + 3 * g + w];
        }
        P.out_ref.resize(n_outputs);
        for (size_t o = 0; o < n_outputs; o++) P.out_ref[o] = slot_ref(outputs[o]);
        // ---- lane shifts.  A shifted reference reads other ROWS of the slot it names, nothing else: the wire is of
        // an earlier level (or an input), so all its rows are written before the reading level's first call in stream
        // order, and its slot is held until the last level that reads the wire ends, whichever instance is read.  The
        // slot rule above therefore needs no change.
        auto shift_of = [&](uint32_t ref, const int32_t *tab, size_t i) -> int32_t {
            return tab && wire_id(ref) != CIRC_FALSE ? tab[i] : 0;
        };
        P.in_shift.resize(2 * P.live());
        for (size_t k = 0; k < P.live(); k++)
            for (int j = 0; j < 2; j++) {
                const size_t i = term_of(P.order[k], j);
                P.in_shift[2 * k + j] = i == SIZE_MAX ? 0 : shift_of(refs[i], gate_shift, i);
            }
        P.out_shift.resize(n_outputs);
        for (size_t o = 0; o < n_outputs; o++) P.out_shift[o] = shift_of(outputs[o], out_shift, o);
        std::vector<uint32_t> rank_of(NG, CIRC_NONE);   // node -> index in `order`
        for (size_t k = 0; k < P.live(); k++) rank_of[P.order[k]] = (uint32_t)k;
        auto row_ref = [&](uint32_t ref) -> uint32_t {
            const uint32_t id = wire_id(ref);
            const int64_t g = node_of(id);
            return (g < 0 ? id : n_inputs + 3 * rank_of[g] + (id - n_inputs) % 3) | (ref & CIRC_NOT);
        };
        P.in_row.resize(2 * P.live());
        for (size_t k = 0; k < P.live(); k++)
            for (int j = 0; j < 2; j++) {
                const size_t i = term_of(P.order[k], j);
                P.in_row[2 * k + j] = i == SIZE_MAX ? CIRC_FALSE : row_ref(refs[i]);
            }
        // ---- three-input nodes: the third reference in tables of their own, so that in_ref, in_shift and in_row keep
        // the layout the two-input kernels read.  Every sum node has one: its third term, or the constant FALSE
        P.in_ref3.assign(P.live(), CIRC_NO_INPUT);
        P.in_shift3.assign(P.live(), 0);
        P.in_row3.assign(P.live(), CIRC_NO_INPUT);
        P.three_before.assign(P.live() + 1, 0);
        size_t terms = 0;
        for (size_t k = 0; k < P.live(); k++) {
            const size_t g = P.order[k];
            if (!N.classic(g)) {
                const size_t i = term_of(g, 2);
                P.in_ref3[k] = i == SIZE_MAX ? CIRC_FALSE : slot_ref(refs[i]);
                P.in_shift3[k] = i == SIZE_MAX ? 0 : shift_of(refs[i], gate_shift, i);
                P.in_row3[k] = i == SIZE_MAX ? CIRC_FALSE : row_ref(refs[i]);
                P.three++;
            }
            P.three_before[k + 1] = P.three;
            P.wide += N.wide(g);
            terms += N.count(g);
        }
        // ---- wide nodes: the terms of every live node as CSR tables of their own
        if (P.wide) {
            P.w_start.reserve(P.live() + 1);
            P.w_ref.reserve(terms);
            P.w_shift.reserve(terms);
            P.w_weight.reserve(terms);
            P.w_row.reserve(terms);
            for (size_t k = 0; k < P.live(); k++) {
                const size_t g = P.order[k];
                P.w_start.push_back((uint32_t)P.w_ref.size());
                for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
                    P.w_ref.push_back(slot_ref(refs[i]));
                    P.w_shift.push_back(shift_of(refs[i], gate_shift, i));
                    P.w_weight.push_back(N.weight(i));
                    P.w_row.push_back(row_ref(refs[i]));
                }
            }
            P.w_start.push_back((uint32_t)P.w_ref.size());
        }
        P.out_node.assign(n_outputs, CIRC_NONE);
        P.out_gate.assign(n_outputs, 0);
        for (size_t o = 0; o < n_outputs; o++) {
            const uint32_t id = wire_id(outputs[o]);
            const int64_t g = node_of(id);
            if (g < 0 || P.out_shift[o] != 0) continue;
            if ((id - n_inputs) % 3 == 2 && !N.classic((size_t)g)) continue;   // XOR3 / LOW: linear over Z_r, no gate row
            P.out_node[o] = rank_of[g];
            P.out_gate[o] = (id - n_inputs) % 3;
        }
    } catch (...) {   // std::bad_alloc, std::length_error: nothing else allocates or throws here
        P = CircuitPlan();
        return SGFHE_ERR_OOM;
    }
    return SGFHE_OK;
}

// The arrays of sgfhe_circuit_create3 (`arity` 3: gates and gate_shift are [n_gates][3], and a third reference
// CIRC_NO_INPUT makes the node a two-input node) or of sgfhe_circuit_create_lanes (`arity` 2: [n_gates][2], every node
// a two-input node).
inline int32_t circuit_plan_arity(uint32_t n_inputs, const uint32_t *gates, const int32_t *gate_shift, size_t n_gates,
                                  int arity, const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs,
                                  uint32_t group, CircuitPlan &P) noexcept {
    const CircuitNodes N = {arity, gates, gate_shift};
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create_w.
inline int32_t circuit_plan_w(uint32_t n_inputs, const uint32_t *node_kind, const uint32_t *node_start,
                              const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                              size_t n_gates, const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs,
                              uint32_t group, CircuitPlan &P) noexcept {
    const CircuitNodes N = {0, term_ref, term_shift, node_kind, node_start, term_weight};
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create_lanes.
inline int32_t circuit_plan(uint32_t n_inputs, const uint32_t *gates, const int32_t *gate_shift, size_t n_gates,
                            const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                            CircuitPlan &P) noexcept {
    return circuit_plan_arity(n_inputs, gates, gate_shift, n_gates, 2, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create3.
inline int32_t circuit_plan3(uint32_t n_inputs, const uint32_t *gates, const int32_t *gate_shift, size_t n_gates,
                             const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                             CircuitPlan &P) noexcept {
    return circuit_plan_arity(n_inputs, gates, gate_shift, n_gates, 3, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create: no shifts, group 1.
inline int32_t circuit_plan(uint32_t n_inputs, const uint32_t *gates, size_t n_gates, const uint32_t *outputs,
                            size_t n_outputs, CircuitPlan &P) noexcept {
    return circuit_plan(n_inputs, gates, nullptr, n_gates, outputs, nullptr, n_outputs, 1u, P);
}

// The circuit in clear over `instances`, for the noise probe (sgfhe_circuit_run_probe): the plaintext bit of every
// probe row -- the n_inputs input wires, then AND, OR, XOR of every live node in `order` -- as a bit table of
// circuit_probe_rows(P) rows of circuit_bit_words(instances) uint64 words each: bit (t & 63) of word t / 64 of a row
// is instance t (the bits past `instances` in a row's last word are unspecified).  in_bits [n_inputs][instances],
// bit 0 of each byte.  Word-parallel: three operations per (live node, 64 instances); a lane-shifted input is first
// laid out as a row of its own, instance by instance (instance t reads bit t + d where its lane allows, 0 elsewhere;
// `instances` must be a multiple of P.group, SGFHE_ERR_INVALID_ARG otherwise).  A three-input node's rows are MAJ,
// ONE_OR_TWO (one or two of its inputs true) and XOR3; a sum node's are HI, MID and LOW of s = sum of w x mod 4.  SGFHE_ERR_OOM when the table cannot be allocated; nothing
// throws out of it.
inline size_t circuit_probe_rows(const CircuitPlan &P) { return (size_t)P.n_inputs + 3 * P.live(); }
inline size_t circuit_bit_words(size_t instances) { return (instances + 63) / 64; }
// wire id of a probe row (the inverse of CircuitPlan::in_row's numbering)
inline uint32_t circuit_probe_wire(const CircuitPlan &P, size_t row) {
    if (row < P.n_inputs) return (uint32_t)row;
    const size_t k = (row - P.n_inputs) / 3, w = (row - P.n_inputs) % 3;
    return (uint32_t)(P.n_inputs + 3 * (size_t)P.order[k] + w);
}
inline int32_t circuit_plain_bits(const CircuitPlan &P, const uint8_t *in_bits, size_t instances,
                                  std::vector<uint64_t> &table) noexcept {
    if (!in_bits && P.n_inputs && instances) return SGFHE_ERR_INVALID_ARG;
    if (instances % P.group) return SGFHE_ERR_INVALID_ARG;
    const size_t wpr = circuit_bit_words(instances);
    std::vector<uint64_t> shifted[3];
    try {
        table.assign(circuit_probe_rows(P) * wpr, 0);
        if (P.lanes())
            for (auto &s : shifted) s.assign(wpr, 0);
    } catch (...) {
        return SGFHE_ERR_OOM;
    }
    for (size_t i = 0; i < P.n_inputs; i++)
        for (size_t t = 0; t < instances; t++)
            table[i * wpr + t / 64] |= (uint64_t)(in_bits[i * instances + t] & 1u) << (t % 64);
    const int64_t G = P.group;
    // the row a reference reads, before NOT: the table's own row, or that row shifted by d inside every group
    auto source = [&](uint32_t ref, int32_t d, std::vector<uint64_t> &tmp) -> const uint64_t * {
        const uint32_t row = circuit_detail::wire_id(ref);
        if (row == CIRC_FALSE) return nullptr;
        const uint64_t *src = table.data() + (size_t)row * wpr;
        if (d == 0) return src;
        std::fill(tmp.begin(), tmp.end(), 0ull);
        for (size_t t = 0; t < instances; t++) {
            const int64_t lane = (int64_t)(t % (size_t)G) + d;
            if (lane < 0 || lane >= G) continue;
            const size_t u = (size_t)((int64_t)t + d);   // same group: 0 <= u < instances
            tmp[t / 64] |= (src[u / 64] >> (u % 64) & 1ull) << (t % 64);
        }
        return tmp.data();
    };
    auto word = [&](const uint64_t *src, uint32_t ref, size_t w) -> uint64_t {
        const uint64_t v = src ? src[w] : 0ull;
        return ref & CIRC_NOT ? ~v : v;
    };
    for (size_t k = 0; k < P.live(); k++) {   // `order` is a topological order: inputs are rows filled before
        uint64_t *o = table.data() + ((size_t)P.n_inputs + 3 * k) * wpr;
        if (P.wsum() && P.in_ref3[k] != CIRC_NO_INPUT) {
            // a sum node: s = sum of w x mod 4 as two bit planes, (lo, hi) = (o[2 wpr ..], o[0 ..]), term by term
            // (-1 = 3 and -2 = 2 mod 4); then HI = s in {2, 3} = hi, MID = s in {1, 2} = lo ^ hi, LOW = s mod 2 = lo
            uint64_t *hi = o, *lo = o + 2 * wpr;
            for (uint32_t i = P.w_start[k]; i < P.w_start[k + 1]; i++) {
                const uint64_t *sx = source(P.w_row[i], P.w_shift[i], shifted[0]);
                const int32_t wt = P.w_weight[i];
                for (size_t w = 0; w < wpr; w++) {
                    const uint64_t x = word(sx, P.w_row[i], w);
                    if (wt & 1) {
                        hi[w] ^= (lo[w] & x) ^ (wt < 0 ? x : 0ull);
                        lo[w] ^= x;
                    } else {
                        hi[w] ^= x;
                    }
                }
            }
            for (size_t w = 0; w < wpr; w++) o[wpr + w] = lo[w] ^ hi[w];
            continue;
        }
        const uint32_t rx = P.in_row[2 * k], ry = P.in_row[2 * k + 1];
        const uint64_t *sx = source(rx, P.in_shift[2 * k], shifted[0]), *sy = source(ry, P.in_shift[2 * k + 1], shifted[1]);
        const uint32_t rz = P.in_row3[k];
        if (rz != CIRC_NO_INPUT) {
            const uint64_t *sz = source(rz, P.in_shift3[k], shifted[2]);
            for (size_t w = 0; w < wpr; w++) {
                const uint64_t x = word(sx, rx, w), y = word(sy, ry, w), z = word(sz, rz, w);
                o[w] = (x & y) | (z & (x | y));
                o[wpr + w] = (x | y | z) & ~(x & y & z);
                o[2 * wpr + w] = x ^ y ^ z;
            }
            continue;
        }
        for (size_t w = 0; w < wpr; w++) {
            const uint64_t x = word(sx, rx, w), y = word(sy, ry, w);
            o[w] = x & y;
            o[wpr + w] = x | y;
            o[2 * wpr + w] = x ^ y;
        }
    }
    return SGFHE_OK;
}

}  // namespace sgfhe

// The opaque handle of the C ABI: a plan is host data, independent of any ctx.
struct sgfhe_circuit {
    sgfhe::CircuitPlan plan;
};
