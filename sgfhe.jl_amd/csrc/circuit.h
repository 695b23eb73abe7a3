// Host-side planner of sgfhe_circuit_* (include/sgfhe_hip.h): validates a gate
// graph, prunes the nodes no output depends on, levels the rest ASAP, gives every wire that is read a
// slot of the device wire table by liveness, fixes the row and call numbering of a run, and writes every node's inputs
// -- whichever entry the arrays came through -- into one CSR node table, which it lays with the other device tables
// into the one image a run uploads; circuit_plain_bits evaluates a planned circuit in clear for the noise probe.
// The call arithmetic of a run lives here too (at the end): circuit_level_call, circuit_job_chunk, circuit_pack_runs and
// circuit_run_sizes say which rows, nodes and jobs a call covers and what the buffers hold; the engine only launches.
// Plain C++, no HIP: tests/native/circuit_plan_sanitized.cpp, circuit_bits_sanitized.cpp, circuit_lanes_sanitized.cpp,
// circuit_gate3_sanitized.cpp, circuit_wsum_sanitized.cpp, circuit_lut_sanitized.cpp, circuit_lut_multi_sanitized.cpp,
// circuit_data_sanitized.cpp, circuit_calls_sanitized.cpp, circuit_steps_sanitized.cpp and circuit_routes_sanitized.cpp
// drive it under ASan / UBSan on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <new>
#include <queue>
#include <stdexcept>
#include <vector>

#include "../../include/sgfhe_hip.h"

namespace sgfhe {

// A wire id below 2^31 - 1 (0x7FFFFFFF is the constant FALSE), bit 31 = NOT.  Slot references in the
// device tables use the same encoding with slot numbers in place of wire ids.
constexpr uint32_t CIRC_FALSE = SGFHE_CIRCUIT_FALSE;
constexpr uint32_t CIRC_NOT = SGFHE_CIRCUIT_NOT;
constexpr uint32_t CIRC_NONE = 0xFFFFFFFFu;     // out_slot of a gate output nothing reads
constexpr uint32_t CIRC_NO_INPUT = SGFHE_CIRCUIT_NONE;   // third reference of a two-input node (never a wire id)
// A table that is run-time data (sgfhe_circuit_create_data): bit 24 of a LUT node's kind word, whose bits 8..23 then hold
// the plane, and of fam_entry[4 i], whose low bits then hold the plane (kernels.h CIRC_TABLE_DATA)
constexpr uint32_t CIRC_DATA = 0x01000000u;
constexpr int32_t CIRC_ROUTE_FALSE = SGFHE_CIRCUIT_ROUTE_FALSE;   // entry of a route table: the constant FALSE at that lane

// Word offsets of the device tables in CircuitPlan::image (int32_t tables by bit pattern); `words` is its length.
struct CircuitImage {
    uint32_t node_kind = 0, term_start = 0, term_ref = 0, term_shift = 0, term_weight = 0;
    uint32_t out_slot = 0, out_ref = 0, out_shift = 0, input_slot = 0, jobs = 0, words = 0;
    uint32_t fam_start = 0, fam_entry = 0;   // behind `jobs`, and only in a plan that has live siblings
    // behind those, and only in a plan with registers (sgfhe_circuit_create_seq); the registers' slots are the first
    // n_regs entries of input_slot
    uint32_t next_ref = 0, next_shift = 0, next_scale = 0, reg_index = 0;
    // behind every other table, and only in a plan with route tables (sgfhe_circuit_create_routed, n_routes > 0);
    // next_route only when the plan has registers as well
    uint32_t routes = 0, term_route = 0, out_route = 0, next_route = 0;
};

struct CircuitPlan {
    uint32_t n_inputs = 0, n_gates = 0, n_outputs = 0;
    uint32_t levels = 0, widest = 0, slots = 0;
    uint32_t group = 1;                 // lane group size G (sgfhe_circuit_create_lanes); 1: no reference is shifted
    uint32_t n_planes = 0;              // data planes of a run (sgfhe_circuit_create_data); 0: every table is the plan's
    uint32_t n_regs = 0;                // registers (sgfhe_circuit_create_seq): input wires 0 .. n_regs, fed back by a
                                        // stepped run; 0: a feed-forward plan
    uint32_t n_routes = 0;              // route tables (sgfhe_circuit_create_routed); 0: every reference reads by its shift
    std::vector<uint32_t> level;        // [n_gates]: level of every node, 0 = pruned
    std::vector<uint32_t> order;        // live nodes, level by level, ascending index within a level
    std::vector<uint32_t> level_start;  // [levels + 2]: level L's nodes are order[level_start[L] .. level_start[L + 1])
                                        // (level 0 holds none: level_start[0] == level_start[1] == 0)
    std::vector<uint32_t> input_slot;   // [n_inputs]: slot of every input wire, CIRC_NONE if nothing reads it
    // The node table: one CSR over the live nodes in `order`, then the n_outputs nodes of the pack stage's
    // pseudo-level (node live() + o is the classic node (TRUE, output o)).  A term is a slot reference (CIRC_NOT,
    // CIRC_FALSE), a lane shift -- the term reads instance t + d of its slot where 0 <= t % group + d < group, the
    // constant FALSE elsewhere; 0 on every reference to the constant -- and a weight.  A three-input node is the sum
    // node of its three unit weights.
    std::vector<uint32_t> node_kind;    // [live + n_outputs]: bits 0..7 the kind -- 0 classic (two unit terms), 1 sum
                                        // node, 2 LUT node (sgfhe_circuit_create_lut) -- and for a LUT node bits 8..15
                                        // its truth table, or CIRC_DATA and in bits 8..23 its plane
    std::vector<uint32_t> term_start;   // [live + n_outputs + 1]: node k's terms are term_start[k] .. term_start[k + 1]
    std::vector<uint32_t> term_ref;     // [terms + 2 n_outputs]
    std::vector<int32_t> term_shift;    // [terms + 2 n_outputs]
    std::vector<int32_t> term_weight;   // [terms + 2 n_outputs]: -2, -1, 1, 2
    std::vector<uint32_t> out_slot;     // [live][3]: slot of the node's AND / OR / XOR wire, CIRC_NONE if unread
                                        // (HI / MID / LOW of a sum node)
    std::vector<uint32_t> out_ref;      // [n_outputs]: the circuit's outputs as slot references
    std::vector<int32_t> out_shift;     // [n_outputs]
    // SGFHE_CIRCUIT_PACK_DIRECT: where an output that names a gate wire is produced
    std::vector<uint32_t> out_node;     // [n_outputs], host only: index in `order` of the producing node, CIRC_NONE for
                                        // an input wire, the constant, a lane-shifted reference or the LOW wire of a sum
                                        // node, which is no gate row over Z_Q (those are refreshed)
    std::vector<uint32_t> out_gate;     // [n_outputs], host only: 0 AND, 1 OR, 2 XOR (0 where out_node is CIRC_NONE)
    // the direct outputs by producing node (ascending index in `order`, so the jobs of one level call are a run of the
    // table): job = {output, rank of the node in its level, gate | CIRC_NOT of the output}
    std::vector<uint32_t> jobs;         // [direct outputs][3]
    std::vector<uint32_t> job_k;        // [direct outputs], host only: the producing node's index in `order`
    // Host only (sgfhe_circuit_run_probe): the live nodes' terms as PROBE ROWS -- row i < n_inputs is input wire i, row
    // n_inputs + 3 k + w is wire w of the k-th live node in `order` -- with CIRC_NOT and CIRC_FALSE as in a reference
    std::vector<uint32_t> term_row;     // [terms]
    std::vector<uint32_t> sum_before;   // [live + 1], host only: sum nodes among order[0 .. k)
    std::vector<uint32_t> lut_before;   // [live + 1], host only: LUT nodes among order[0 .. k)
    // LUT families (sgfhe_circuit_create_lut_multi): a SIBLING (kind 3) is a further table on its leader's bootstrap.
    // It takes no row and is not in `order`; the live siblings of the live node k are entries fam_start[k] ..
    // fam_start[k + 1] of one CSR (empty in a plan without live siblings, and then not in the image).
    std::vector<uint32_t> fam_start;    // [live + 1]
    std::vector<uint32_t> fam_entry;    // [live siblings][4]: truth table (or CIRC_DATA | plane), then the slots of its
                                        // three wires (CIRC_NONE if unread)
    std::vector<uint32_t> fam_node;     // [live siblings], host only: the sibling's node index; its wires are the probe
                                        // rows n_inputs + 3 live() + 3 i + w
    // Registers (sgfhe_circuit_create_seq): after a step register i takes the value of next_ref[i] (a slot reference)
    // read at the lane shift next_shift[i]; NOT on it is taken at the codeword Dr >> reg_scale[i].  reg_index is 0, 1, ..
    // (the "slots" of the state buffer, for the split of state ciphertexts).  All empty in a plan without registers.
    std::vector<uint32_t> next_ref;     // [n_regs]
    std::vector<int32_t> next_shift;    // [n_regs]
    std::vector<uint32_t> reg_scale;    // [n_regs]: 0, 1, 2
    std::vector<uint32_t> reg_index;    // [n_regs]
    // Lane routes (sgfhe_circuit_create_routed): a reference whose route index is k >= 1 reads, at lane l of its group,
    // lane routes[(k - 1) * group + l] of the same group -- the constant FALSE where that is CIRC_ROUTE_FALSE -- and has
    // shift 0; index 0: the shift applies.  0 on every reference to the constant.  All empty in a plan without tables.
    std::vector<int32_t> routes;        // [n_routes][group]
    std::vector<uint32_t> term_route;   // [terms + 2 n_outputs], beside term_shift
    std::vector<uint32_t> out_route;    // [n_outputs], beside out_shift
    std::vector<uint32_t> next_route;   // [n_regs], beside next_shift
    // Every device table above in one array, uploaded once per run: node_kind, term_start, term_ref, term_shift,
    // term_weight, out_slot, out_ref, out_shift, input_slot, jobs (then fam_start, fam_entry; then next_ref, next_shift,
    // reg_scale, reg_index; then routes, term_route, out_route, next_route), each at its offset `at`
    std::vector<uint32_t> image;
    CircuitImage at;

    size_t live() const { return order.size(); }
    uint32_t n_stream() const { return n_inputs - n_regs; }   // the inputs a step brings
    bool lanes() const { return group > 1; }   // (group 1 admits no shift but 0)
    // the route table of a reference whose route index is `k`, NULL for none
    const int32_t *route(uint32_t k) const { return k ? routes.data() + (size_t)(k - 1) * group : nullptr; }
    const int32_t *term_route_of(size_t i) const { return n_routes ? route(term_route[i]) : nullptr; }
    // live nodes order[ka .. kb] hold a sum node: the call takes an XOR3 kernel for its LOW rows
    bool gate3_in(uint32_t ka, uint32_t kb) const { return sum_before[kb + 1] != sum_before[ka]; }
    // live nodes order[ka .. kb] hold a LUT node: the call carries a LUT descriptor
    bool lut_in(uint32_t ka, uint32_t kb) const { return lut_before[kb + 1] != lut_before[ka]; }
    // live nodes order[ka .. kb] lead a live sibling: the call extracts further tables (k_final_lut_multi)
    bool fam_in(uint32_t ka, uint32_t kb) const { return !fam_node.empty() && fam_start[kb + 1] != fam_start[ka]; }
    size_t siblings() const { return fam_node.size(); }
    uint32_t kind(size_t k) const { return node_kind[k] & 0xFFu; }
    uint32_t table(size_t k) const { return (node_kind[k] >> 8) & 0xFFu; }
    // the table of a LUT node's kind word or of a family entry at instance t of a run whose planes are `data`
    // ([n_planes][instances])
    static uint32_t table_at(uint32_t word, uint32_t plane_shift, const uint8_t *data, size_t instances, size_t t) {
        if (!(word & CIRC_DATA)) return (word >> plane_shift) & 0xFFu;
        return data[(size_t)((word >> plane_shift) & 0xFFFFu) * instances + t];
    }
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
// count(g).  `lut`: the arrays of sgfhe_circuit_create_lut, whose kind 2 marks a LUT node of table tables[g].
// `multi`: those of sgfhe_circuit_create_lut_multi, whose kind 3 marks a sibling -- no terms, table tables[g], a further
// table on the bootstrap of its LEADER, the nearest earlier kind-2 node.  `data`: those of sgfhe_circuit_create_data,
// whose kinds 4 and 5 are a LUT node and a sibling with tables[g] a plane index below `n_planes`.
struct CircuitNodes {
    int arity;
    const uint32_t *refs;
    const int32_t *shifts;
    const uint32_t *kind = nullptr, *start = nullptr;
    const int32_t *weights = nullptr;
    const uint32_t *tables = nullptr;
    bool lut = false, multi = false, data = false;
    uint32_t n_planes = 0;

    size_t first(size_t g) const { return arity ? (size_t)arity * g : start[g]; }
    size_t count(size_t g) const {
        if (!arity) return (size_t)start[g + 1] - start[g];
        return arity == 3 && refs[3 * g + 2] != CIRC_NO_INPUT ? 3 : 2;
    }
    bool classic(size_t g) const { return arity ? count(g) == 2 : kind[g] == 0; }
    bool is_sibling(size_t g) const { return !arity && (kind[g] == 3 || kind[g] == 5); }
    bool is_lut(size_t g) const { return !arity && kind[g] >= 2 && kind[g] <= 5; }   // (wires with scales 0, 1, 2)
    bool is_data(size_t g) const { return !arity && (kind[g] == 4 || kind[g] == 5); }
    // a LUT node's or sibling's table as the device tables hold it, before any shift
    uint32_t table_word(size_t g, uint32_t shift) const {
        return is_data(g) ? CIRC_DATA | tables[g] << shift : tables[g] << shift;
    }
    uint32_t kind_of(size_t g) const { return classic(g) ? 0u : (is_lut(g) ? 2u : 1u); }
    int32_t weight(size_t i) const { return weights ? weights[i] : 1; }
};

// The registers of sgfhe_circuit_create_seq: input wires 0 .. n_regs; next_ref [n_regs] wire references validated like
// outputs, next_shift [n_regs] (NULL: all 0), reg_scale [n_regs] (NULL: all 0; each 0, 1 or 2).
struct CircuitRegs {
    uint32_t n_regs;
    const uint32_t *next_ref;
    const int32_t *next_shift;
    const uint32_t *reg_scale;
    uint32_t scale(uint32_t i) const { return reg_scale ? reg_scale[i] : 0u; }
};

// The lane routes of sgfhe_circuit_create_routed: routes [n_routes][group], entries in [0, group) or CIRC_ROUTE_FALSE;
// term_route beside the term arrays, out_route [n_outputs], next_route [n_regs] (each NULL: all 0): 0 = none, k >= 1 =
// table k - 1, and then the reference's shift must be 0.
struct CircuitRoutes {
    uint32_t n_routes;
    const int32_t *routes;
    const uint32_t *term_route, *out_route, *next_route;
};

// Builds `P` from the nodes `N` (gate shifts / out_shift NULL: all 0).  `R` (NULL or n_regs 0: none): the registers; their
// next-state references count as readers exactly as outputs do -- liveness, levels, slot lifetime -- so the plan's
// order, levels and slots are those of the plan whose outputs are outputs ++ next_ref.  `T` (NULL: none): the lane routes;
// nothing but the route tables of the plan sees them, and with n_routes = 0 the plan is the plan without `T`.  Returns SGFHE_OK, SGFHE_ERR_INVALID_ARG for a
// malformed circuit, SGFHE_ERR_OOM when an allocation fails.  Nothing throws out of it, and a refused circuit costs no
// allocation.
inline int32_t circuit_plan_nodes(uint32_t n_inputs, const CircuitNodes &N, size_t n_gates, const uint32_t *outputs,
                                  const int32_t *out_shift, size_t n_outputs, uint32_t group, CircuitPlan &P,
                                  const CircuitRegs *R = nullptr, const CircuitRoutes *T = nullptr) noexcept {
    using circuit_detail::wire_id;
    const uint32_t *refs = N.refs;
    const uint32_t n_regs = R ? R->n_regs : 0u;
    const int32_t *gate_shift = N.shifts;
    // ---- validate: every size below 2^31, wire ids below the constant, inputs name earlier wires only,
    // every shift inside the group (in 64 bits: -INT32_MIN does not exist).  CIRC_NO_INPUT is above every wire id, so
    // anywhere but beside a two-input node of the [n_gates][3] arrays it fails the id checks below.
    if (n_outputs < 1 || !outputs || (n_gates && !refs) || group < 1) return SGFHE_ERR_INVALID_ARG;
    auto shift_ok = [&](int32_t d) { return (d < 0 ? -(int64_t)d : (int64_t)d) < (int64_t)group; };
    if (n_inputs >= 0x80000000u || n_gates >= 0x80000000u || n_outputs >= 0x80000000u) return SGFHE_ERR_INVALID_ARG;
    const uint64_t n_wires = (uint64_t)n_inputs + 3 * (uint64_t)n_gates;
    if (n_wires >= CIRC_FALSE) return SGFHE_ERR_INVALID_ARG;
    if (n_regs > n_inputs || (n_regs && !R->next_ref)) return SGFHE_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_regs; i++) {   // (CIRC_NO_INPUT is above every wire id)
        const uint32_t id = wire_id(R->next_ref[i]);
        if ((id != CIRC_FALSE && id >= n_wires) || R->scale(i) > 2u) return SGFHE_ERR_INVALID_ARG;
        if (R->next_shift && !shift_ok(R->next_shift[i])) return SGFHE_ERR_INVALID_ARG;
    }
    if (!N.arity) {   // the CSR itself, node by node, before a term of the node is read
        if (n_gates && (!N.kind || !N.start || !N.weights || N.start[0] != 0)) return SGFHE_ERR_INVALID_ARG;
        if (n_gates && N.lut && !N.tables) return SGFHE_ERR_INVALID_ARG;
        if (N.n_planes > SGFHE_CIRCUIT_MAX_PLANES) return SGFHE_ERR_INVALID_ARG;
        auto table_ok = [&](size_t g) { return N.tables[g] < (N.is_data(g) ? N.n_planes : 256u); };
        size_t family = 0;   // members so far of the family node g - 1 belongs to (0: it is no LUT node)
        for (size_t g = 0; g < n_gates; g++) {
            if (N.kind[g] > (N.data ? 5u : (N.multi ? 3u : (N.lut ? 2u : 1u))) || N.start[g + 1] < N.start[g])
                return SGFHE_ERR_INVALID_ARG;
            const size_t nj = N.count(g);
            if (N.is_sibling(g)) {   // a sibling: no terms, a table, behind a LUT node or a sibling, in a family that has room
                if (nj != 0 || !table_ok(g) || family == 0 || family >= SGFHE_LUT_MAX_TABLES) return SGFHE_ERR_INVALID_ARG;
                family++;
                continue;
            }
            family = N.is_lut(g) ? 1 : 0;
            if (N.is_lut(g)) {   // a LUT node: three unit terms (positions 0, 1, 2), a table of 8 entries (or a plane)
                if (nj != 3 || !table_ok(g)) return SGFHE_ERR_INVALID_ARG;
            } else if (N.kind[g] == 0 ? nj != 2 : (nj < 1 || nj > SGFHE_CIRCUIT_MAX_TERMS)) {
                return SGFHE_ERR_INVALID_ARG;
            }
            for (size_t i = N.first(g); i < N.first(g) + nj; i++) {
                const int32_t w = N.weights[i];
                if (N.kind[g] != 1 ? w != 1 : (w == 0 || w < -2 || w > 2)) return SGFHE_ERR_INVALID_ARG;
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
    bool scaled_reg = false;
    for (uint32_t i = 0; i < n_regs; i++) scaled_reg = scaled_reg || R->scale(i) != 0;
    if (N.lut || scaled_reg) {
        // ---- the scale rule: a wire carries its bit at the codeword Dr >> scale.  Scale 0: inputs, every wire of a
        // classic or sum node, wire +0 of a LUT node; wires +1 and +2 of a LUT node have scales 1 and 2.  Position i of
        // a LUT node reads the constant or a wire of scale 2 - i; every other reference reads scale 0.
        auto scale_ok = [&](uint32_t ref, uint32_t want) {
            const uint32_t id = wire_id(ref);
            if (id == CIRC_FALSE) return true;
            if (id < n_inputs) return (id < n_regs ? R->scale(id) : 0u) == want;   // a register has the scale it was given
            const uint32_t have = !N.is_lut((id - n_inputs) / 3) ? 0u : (id - n_inputs) % 3;
            return have == want;
        };
        for (size_t g = 0; g < n_gates; g++)
            for (size_t i = N.first(g), end = i + N.count(g), p = 0; i < end; i++, p++)
                if (!scale_ok(refs[i], N.is_lut(g) ? 2u - (uint32_t)p : 0u)) return SGFHE_ERR_INVALID_ARG;
        for (size_t o = 0; o < n_outputs; o++)
            if (!scale_ok(outputs[o], 0u)) return SGFHE_ERR_INVALID_ARG;
        for (uint32_t i = 0; i < n_regs; i++)   // a register is fed the constant or a wire of its own scale
            if (!scale_ok(R->next_ref[i], R->scale(i))) return SGFHE_ERR_INVALID_ARG;
    }
    for (size_t g = 0; gate_shift && g < n_gates; g++)   // (the shift beside CIRC_NO_INPUT is ignored)
        for (size_t i = N.first(g), end = i + N.count(g); i < end; i++)
            if (!shift_ok(gate_shift[i])) return SGFHE_ERR_INVALID_ARG;
    for (size_t o = 0; out_shift && o < n_outputs; o++)
        if (!shift_ok(out_shift[o])) return SGFHE_ERR_INVALID_ARG;
    // ---- the routes: every entry a lane of the group or the fill, every index a table, and never beside a shift
    const uint32_t n_routes = T ? T->n_routes : 0u;
    if (T) {
        if (n_routes > SGFHE_CIRCUIT_MAX_ROUTES || (n_routes && !T->routes)) return SGFHE_ERR_INVALID_ARG;
        for (size_t i = 0; i < (size_t)n_routes * group; i++)
            if (T->routes[i] < CIRC_ROUTE_FALSE || T->routes[i] >= (int64_t)group) return SGFHE_ERR_INVALID_ARG;
        auto route_ok = [&](const uint32_t *route, const int32_t *shift, size_t i) {
            return !route || (route[i] <= n_routes && (route[i] == 0 || !shift || shift[i] == 0));
        };
        for (size_t g = 0; g < n_gates; g++)
            for (size_t i = N.first(g), end = i + N.count(g); i < end; i++)
                if (!route_ok(T->term_route, gate_shift, i)) return SGFHE_ERR_INVALID_ARG;
        for (size_t o = 0; o < n_outputs; o++)
            if (!route_ok(T->out_route, out_shift, o)) return SGFHE_ERR_INVALID_ARG;
        for (uint32_t i = 0; i < n_regs; i++)
            if (!route_ok(T->next_route, R->next_shift, i)) return SGFHE_ERR_INVALID_ARG;
    }
    try {
        P = CircuitPlan();
        P.n_inputs = n_inputs;
        P.n_gates = (uint32_t)n_gates;
        P.n_outputs = (uint32_t)n_outputs;
        P.group = group;
        P.n_planes = N.n_planes;
        P.n_regs = n_regs;
        P.n_routes = n_routes;
        if (n_routes) P.routes.assign(T->routes, T->routes + (size_t)n_routes * group);
        const uint32_t NG = (uint32_t)n_gates;
        auto node_of = [&](uint32_t id) -> int64_t {   // producing node of a wire, -1 for inputs and the constant
            return (id == CIRC_FALSE || id < n_inputs) ? -1 : (int64_t)((id - n_inputs) / 3);
        };
        // ---- prune: a node is live when an output reaches it (walk back from the outputs, last node first); a leader
        // is live when any of its siblings is
        std::vector<uint32_t> leader(NG);
        for (uint32_t g = 0; g < NG; g++) leader[g] = N.is_sibling(g) ? leader[g - 1] : g;
        std::vector<uint8_t> live(NG, 0);
        for (size_t o = 0; o < n_outputs; o++) {
            const int64_t g = node_of(wire_id(outputs[o]));
            if (g >= 0) live[g] = 1;
        }
        for (uint32_t i = 0; i < n_regs; i++) {
            const int64_t g = node_of(wire_id(R->next_ref[i]));
            if (g >= 0) live[g] = 1;
        }
        for (uint32_t g = NG; g-- > 0;) {
            if (!live[g]) continue;
            live[leader[g]] = 1;
            for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
                const int64_t h = node_of(wire_id(refs[i]));
                if (h >= 0) live[h] = 1;
            }
        }
        // ---- level ASAP: 1 + the largest level of its input nodes (inputs and the constant: 0); a sibling has its
        // leader's level and takes no row
        P.level.assign(NG, 0);
        auto takes_row = [&](uint32_t g) { return P.level[g] && !N.is_sibling(g); };
        // the live siblings of node g, in ascending index
        auto each_sibling = [&](uint32_t g, auto &&fn) {
            for (uint32_t h = g + 1; h < NG && N.is_sibling(h); h++)
                if (live[h]) fn(h);
        };
        for (uint32_t g = 0; g < NG; g++) {
            if (!live[g]) continue;
            if (N.is_sibling(g)) { P.level[g] = P.level[leader[g]]; continue; }
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
            if (takes_row(g)) P.level_start[P.level[g] + 1]++;
        for (uint32_t L = 1; L <= P.levels; L++) {
            P.widest = std::max(P.widest, P.level_start[L + 1]);
            P.level_start[L + 1] += P.level_start[L];
        }
        P.order.resize(P.level_start[P.levels + 1]);
        {
            std::vector<uint32_t> fill(P.level_start.begin(), P.level_start.end() - 1);
            for (uint32_t g = 0; g < NG; g++)
                if (takes_row(g)) P.order[fill[P.level[g]]++] = g;
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
        for (uint32_t i = 0; i < n_regs; i++) {   // the feedback reads at the end of the step
            const uint32_t id = wire_id(R->next_ref[i]);
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
            auto take_read = [&](uint32_t g) {
                for (uint32_t w = 0; w < 3; w++) {
                    const uint32_t id = n_inputs + 3 * g + w;
                    if (last_read[id] != UNREAD) take(id);
                }
            };
            for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++) {
                take_read(P.order[k]);
                each_sibling(P.order[k], take_read);   // written by the leader's call: slots of the same level
            }
        }
        // ---- the families: every live node's live siblings, their tables and slots; a sibling's probe rows
        std::vector<uint32_t> sib_index(NG, CIRC_NONE);
        P.fam_start.assign(P.live() + 1, 0);
        for (size_t k = 0; k < P.live(); k++) {
            each_sibling(P.order[k], [&](uint32_t h) {
                sib_index[h] = (uint32_t)P.fam_node.size();
                P.fam_node.push_back(h);
                P.fam_entry.push_back(N.table_word(h, 0));
                for (uint32_t w = 0; w < 3; w++) P.fam_entry.push_back(slot_of[n_inputs + 3 * h + w]);
            });
            P.fam_start[k + 1] = (uint32_t)P.fam_node.size();
        }
        // ---- the node table: every live node's terms in the caller's order.  A shifted reference reads other ROWS of
        // the slot it names, nothing else: the wire is of an earlier level (or an input), so all its rows are written
        // before the reading level's first call in stream order, and its slot is held until the last level that reads
        // the wire ends, whichever instance is read.  The slot rule above therefore needs no change.
        auto slot_ref = [&](uint32_t ref) -> uint32_t {
            const uint32_t id = wire_id(ref);
            return (id == CIRC_FALSE ? CIRC_FALSE : slot_of[id]) | (ref & CIRC_NOT);
        };
        auto shift_of = [&](uint32_t ref, const int32_t *tab, size_t i) -> int32_t {
            return tab && wire_id(ref) != CIRC_FALSE ? tab[i] : 0;
        };
        std::vector<uint32_t> rank_of(NG, CIRC_NONE);   // node -> index in `order`
        for (size_t k = 0; k < P.live(); k++) rank_of[P.order[k]] = (uint32_t)k;
        auto row_ref = [&](uint32_t ref) -> uint32_t {
            const uint32_t id = wire_id(ref);
            const int64_t g = node_of(id);
            if (g < 0) return id | (ref & CIRC_NOT);
            const size_t node_row = N.is_sibling((size_t)g) ? P.live() + sib_index[g] : rank_of[g];
            return (uint32_t)(n_inputs + 3 * node_row + (id - n_inputs) % 3) | (ref & CIRC_NOT);
        };
        // (a route, like a shift, is dropped on a reference to the constant; no route array is kept without tables)
        auto route_of = [&](uint32_t ref, const uint32_t *tab, size_t i) -> uint32_t {
            return n_routes && tab && wire_id(ref) != CIRC_FALSE ? tab[i] : 0u;
        };
        auto term = [&](uint32_t ref, int32_t shift, int32_t weight, uint32_t route) {
            P.term_ref.push_back(ref);
            P.term_shift.push_back(shift);
            P.term_weight.push_back(weight);
            if (n_routes) P.term_route.push_back(route);
        };
        P.out_slot.resize(3 * P.live());
        P.sum_before.assign(P.live() + 1, 0);
        P.lut_before.assign(P.live() + 1, 0);
        for (size_t k = 0; k < P.live(); k++) {
            const size_t g = P.order[k];
            P.node_kind.push_back(N.kind_of(g) | (N.is_lut(g) ? N.table_word(g, 8) : 0u));
            P.term_start.push_back((uint32_t)P.term_ref.size());
            for (size_t i = N.first(g), end = i + N.count(g); i < end; i++) {
                term(slot_ref(refs[i]), shift_of(refs[i], gate_shift, i), N.weight(i),
                     route_of(refs[i], T ? T->term_route : nullptr, i));
                P.term_row.push_back(row_ref(refs[i]));
            }
            for (uint32_t w = 0; w < 3; w++) P.out_slot[3 * k + w] = slot_of[n_inputs + 3 * g + w];
            P.sum_before[k + 1] = P.sum_before[k] + (P.kind(k) == 1);
            P.lut_before[k + 1] = P.lut_before[k] + (P.kind(k) == 2);
        }
        // ---- outputs, and the pack stage's pseudo-level: node live() + o is (TRUE, output o), the pair of
        // fhe.jl:669-673
        P.out_ref.resize(n_outputs);
        P.out_shift.resize(n_outputs);
        P.out_node.assign(n_outputs, CIRC_NONE);
        P.out_gate.assign(n_outputs, 0);
        for (size_t o = 0; o < n_outputs; o++) {
            P.out_ref[o] = slot_ref(outputs[o]);
            P.out_shift[o] = shift_of(outputs[o], out_shift, o);
            P.node_kind.push_back(0u);
            P.term_start.push_back((uint32_t)P.term_ref.size());
            const uint32_t route = route_of(outputs[o], T ? T->out_route : nullptr, o);
            if (n_routes) P.out_route.push_back(route);
            term(CIRC_FALSE | CIRC_NOT, 0, 1, 0u);
            term(P.out_ref[o], P.out_shift[o], 1, route);
            const uint32_t id = wire_id(outputs[o]);
            const int64_t g = node_of(id);
            // (a routed output is no gate row in order, even under the identity table: refreshed or lifted, as a shifted one)
            if (g < 0 || P.out_shift[o] != 0 || route != 0) continue;
            if ((id - n_inputs) % 3 == 2 && !N.classic((size_t)g)) continue;   // LOW: linear over Z_r, no gate row
            if (N.is_lut((size_t)g)) continue;   // wire +0 of a LUT node: refreshed or lifted, as a LOW wire is
            P.out_node[o] = rank_of[g];
            P.out_gate[o] = (id - n_inputs) % 3;
        }
        P.term_start.push_back((uint32_t)P.term_ref.size());
        // ---- the registers' next states as slot references
        for (uint32_t i = 0; i < n_regs; i++) {
            P.next_ref.push_back(slot_ref(R->next_ref[i]));
            P.next_shift.push_back(shift_of(R->next_ref[i], R->next_shift, i));
            P.reg_scale.push_back(R->scale(i));
            P.reg_index.push_back(i);
            if (n_routes) P.next_route.push_back(route_of(R->next_ref[i], T ? T->next_route : nullptr, i));
        }
        // ---- the direct-pack jobs, by producing node
        std::vector<uint32_t> byk;
        for (uint32_t o = 0; o < n_outputs; o++)
            if (P.out_node[o] != CIRC_NONE) byk.push_back(o);
        std::sort(byk.begin(), byk.end(), [&](uint32_t x, uint32_t y) {   // (outputs of one node in ascending index)
            return P.out_node[x] != P.out_node[y] ? P.out_node[x] < P.out_node[y] : x < y;
        });
        for (uint32_t o : byk) {
            const uint32_t k = P.out_node[o], L = P.level[P.order[k]];
            P.job_k.push_back(k);
            P.jobs.insert(P.jobs.end(), {o, k - P.level_start[L], P.out_gate[o] | (P.out_ref[o] & CIRC_NOT)});
        }
        // ---- the image of the device tables
        auto place = [&](const auto &tab) -> uint32_t {
            const size_t at = P.image.size();
            if (at + tab.size() >= 0x100000000ull) throw std::length_error("circuit image");
            for (auto v : tab) P.image.push_back((uint32_t)v);
            return (uint32_t)at;
        };
        P.image.reserve(P.node_kind.size() + P.term_start.size() + 3 * P.term_ref.size() + P.out_slot.size() +
                        2 * n_outputs + n_inputs + P.jobs.size() + 4 * (size_t)n_regs + P.routes.size() +
                        P.term_route.size() + P.out_route.size() + P.next_route.size());
        P.at.node_kind = place(P.node_kind);
        P.at.term_start = place(P.term_start);
        P.at.term_ref = place(P.term_ref);
        P.at.term_shift = place(P.term_shift);
        P.at.term_weight = place(P.term_weight);
        P.at.out_slot = place(P.out_slot);
        P.at.out_ref = place(P.out_ref);
        P.at.out_shift = place(P.out_shift);
        P.at.input_slot = place(P.input_slot);
        P.at.jobs = place(P.jobs);
        if (P.siblings()) {
            P.at.fam_start = place(P.fam_start);
            P.at.fam_entry = place(P.fam_entry);
        }
        if (n_regs) {
            P.at.next_ref = place(P.next_ref);
            P.at.next_shift = place(P.next_shift);
            P.at.next_scale = place(P.reg_scale);
            P.at.reg_index = place(P.reg_index);
        }
        if (n_routes) {
            P.at.routes = place(P.routes);
            P.at.term_route = place(P.term_route);
            P.at.out_route = place(P.out_route);
            if (n_regs) P.at.next_route = place(P.next_route);
        }
        P.at.words = (uint32_t)P.image.size();
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

// The arrays of sgfhe_circuit_create_lut: those of sgfhe_circuit_create_w, kind 2 for a LUT node, and node_table.
inline int32_t circuit_plan_lut(uint32_t n_inputs, const uint32_t *node_kind, const uint32_t *node_start,
                                const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                const int32_t *out_shift, size_t n_outputs, uint32_t group, CircuitPlan &P) noexcept {
    const CircuitNodes N = {0, term_ref, term_shift, node_kind, node_start, term_weight, node_table, true};
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create_lut_multi: those of sgfhe_circuit_create_lut, and kind 3 for a sibling.
inline int32_t circuit_plan_lut_multi(uint32_t n_inputs, const uint32_t *node_kind, const uint32_t *node_start,
                                      const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                      const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                      const int32_t *out_shift, size_t n_outputs, uint32_t group, CircuitPlan &P) noexcept {
    const CircuitNodes N = {0, term_ref, term_shift, node_kind, node_start, term_weight, node_table, true, true};
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create_data: those of sgfhe_circuit_create_lut_multi, kinds 4 and 5 for a data LUT node and
// a data sibling, and the number of planes.
inline CircuitNodes circuit_nodes_data(uint32_t n_planes, const uint32_t *node_kind, const uint32_t *node_start,
                                       const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                       const uint32_t *node_table) {
    CircuitNodes N = {0, term_ref, term_shift, node_kind, node_start, term_weight, node_table, true, true};
    N.data = true;
    N.n_planes = n_planes;
    return N;
}
inline int32_t circuit_plan_data(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind, const uint32_t *node_start,
                                 const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                 const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                 const int32_t *out_shift, size_t n_outputs, uint32_t group, CircuitPlan &P) noexcept {
    const CircuitNodes N = circuit_nodes_data(n_planes, node_kind, node_start, term_ref, term_shift, term_weight, node_table);
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P);
}

// The arrays of sgfhe_circuit_create_seq: those of sgfhe_circuit_create_data, and the registers.  With n_regs = 0 the
// plan is the sgfhe_circuit_create_data plan, field for field.
inline int32_t circuit_plan_seq(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind, const uint32_t *node_start,
                                const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                const int32_t *out_shift, size_t n_outputs, uint32_t group, uint32_t n_regs,
                                const uint32_t *next_ref, const int32_t *next_shift, const uint32_t *reg_scale,
                                CircuitPlan &P) noexcept {
    const CircuitNodes N = circuit_nodes_data(n_planes, node_kind, node_start, term_ref, term_shift, term_weight, node_table);
    const CircuitRegs R = {n_regs, next_ref, next_shift, reg_scale};
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P, &R);
}

// The arrays of sgfhe_circuit_create_routed: those of sgfhe_circuit_create_seq, and the lane routes.  With n_routes = 0
// the plan is the sgfhe_circuit_create_seq plan, image word for word.
inline int32_t circuit_plan_routed(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind, const uint32_t *node_start,
                                   const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                   const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                   const int32_t *out_shift, size_t n_outputs, uint32_t group, uint32_t n_regs,
                                   const uint32_t *next_ref, const int32_t *next_shift, const uint32_t *reg_scale,
                                   uint32_t n_routes, const int32_t *routes, const uint32_t *term_route,
                                   const uint32_t *out_route, const uint32_t *next_route, CircuitPlan &P) noexcept {
    const CircuitNodes N = circuit_nodes_data(n_planes, node_kind, node_start, term_ref, term_shift, term_weight, node_table);
    const CircuitRegs R = {n_regs, next_ref, next_shift, reg_scale};
    const CircuitRoutes T = {n_routes, routes, term_route, out_route, next_route};
    return circuit_plan_nodes(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group, P, &R, &T);
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
// probe row -- the n_inputs input wires, then AND, OR, XOR of every live node in `order`, then the three wires of every
// live sibling in the order of CircuitPlan::fam_node -- as a bit table of
// circuit_probe_rows(P) rows of circuit_bit_words(instances) uint64 words each: bit (t & 63) of word t / 64 of a row
// is instance t (the bits past `instances` in a row's last word are unspecified).  in_bits [n_inputs][instances],
// bit 0 of each byte.  Word-parallel: three operations per (live node, 64 instances); a lane-shifted input is first
// laid out as a row of its own, instance by instance (instance t reads bit t + d where its lane allows, 0 elsewhere;
// `instances` must be a multiple of P.group, SGFHE_ERR_INVALID_ARG otherwise), and a routed one likewise (instance t of
// lane l reads bit t - l + route[l], 0 where the entry is CIRC_ROUTE_FALSE).  A sum node's rows are HI, MID and LOW
// of s = sum of w x mod 4: MAJ, ONE_OR_TWO (one or two of its inputs true) and XOR3 of a three-input node.
// `data` [n_planes][instances]: the planes of a run (sgfhe_circuit_run_probe_data); a data LUT node or data sibling of
// plane p has the table data[p][t] at instance t, its own instance whatever its terms' shifts (SGFHE_ERR_INVALID_ARG for
// NULL when the plan has planes and instances > 0).
// SGFHE_ERR_OOM when the table cannot be allocated; nothing throws out of it.
inline size_t circuit_probe_rows(const CircuitPlan &P) { return (size_t)P.n_inputs + 3 * (P.live() + P.siblings()); }
inline size_t circuit_bit_words(size_t instances) { return (instances + 63) / 64; }
// wire id of a probe row (the inverse of CircuitPlan::term_row's numbering)
inline uint32_t circuit_probe_wire(const CircuitPlan &P, size_t row) {
    if (row < P.n_inputs) return (uint32_t)row;
    const size_t k = (row - P.n_inputs) / 3, w = (row - P.n_inputs) % 3;
    return (uint32_t)(P.n_inputs + 3 * (size_t)(k < P.live() ? P.order[k] : P.fam_node[k - P.live()]) + w);
}
inline int32_t circuit_plain_bits(const CircuitPlan &P, const uint8_t *in_bits, size_t instances,
                                  std::vector<uint64_t> &table, const uint8_t *data = nullptr) noexcept {
    if (!in_bits && P.n_inputs && instances) return SGFHE_ERR_INVALID_ARG;
    if (!data && P.n_planes && instances) return SGFHE_ERR_INVALID_ARG;
    if (instances % P.group) return SGFHE_ERR_INVALID_ARG;
    const size_t wpr = circuit_bit_words(instances);
    std::vector<uint64_t> shifted[3];
    try {
        table.assign(circuit_probe_rows(P) * wpr, 0);
        if (P.lanes() || P.n_routes)
            for (auto &s : shifted) s.assign(wpr, 0);
    } catch (...) {
        return SGFHE_ERR_OOM;
    }
    for (size_t i = 0; i < P.n_inputs; i++)
        for (size_t t = 0; t < instances; t++)
            table[i * wpr + t / 64] |= (uint64_t)(in_bits[i * instances + t] & 1u) << (t % 64);
    const int64_t G = P.group;
    // the row term i reads, before NOT: the table's own row, or that row shifted by d or routed inside every group
    auto source = [&](size_t i, std::vector<uint64_t> &tmp) -> const uint64_t * {
        const uint32_t row = circuit_detail::wire_id(P.term_row[i]);
        const int32_t d = P.term_shift[i];
        const int32_t *rho = P.term_route_of(i);
        if (row == CIRC_FALSE) return nullptr;
        const uint64_t *src = table.data() + (size_t)row * wpr;
        if (d == 0 && !rho) return src;
        std::fill(tmp.begin(), tmp.end(), 0ull);
        for (size_t t = 0; t < instances; t++) {
            const int64_t own = (int64_t)(t % (size_t)G), lane = rho ? (int64_t)rho[own] : own + d;
            if (lane < 0 || lane >= G) continue;
            const size_t u = (size_t)((int64_t)t - own + lane);   // same group: 0 <= u < instances
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
        const uint32_t t0 = P.term_start[k], t1 = P.term_start[k + 1];
        if (P.kind(k) == 2) {
            // a LUT node: all three wires carry bit s of the table, s = x0 + 2 x1 + 4 x2 -- the OR over the set table
            // entries of their minterms; its live siblings carry their own tables' bits of the same s
            const uint64_t *sx[3];
            for (uint32_t p = 0; p < 3; p++) sx[p] = source(t0 + p, shifted[p]);
            // (`tw`, `ps`: a kind word with its table from bit 8, or a family entry with it from bit 0; a data table is
            // one mask per entry: the instances of the word whose byte has bit sv set)
            auto fill = [&](uint32_t tw, uint32_t ps, uint64_t *dst) {
                for (size_t w = 0; w < wpr; w++) {
                    uint64_t x[3], f = 0;
                    for (uint32_t p = 0; p < 3; p++) x[p] = word(sx[p], P.term_row[t0 + p], w);
                    for (uint32_t sv = 0; sv < 8; sv++) {
                        uint64_t on = 0;
                        if (!(tw & CIRC_DATA)) {
                            on = ((tw >> ps) >> sv) & 1u ? ~0ull : 0ull;
                        } else {
                            for (size_t t = 64 * w; t < std::min(instances, 64 * w + 64); t++)
                                on |= (uint64_t)((CircuitPlan::table_at(tw, ps, data, instances, t) >> sv) & 1u) << (t % 64);
                        }
                        if (on) f |= on & (sv & 1 ? x[0] : ~x[0]) & (sv & 2 ? x[1] : ~x[1]) & (sv & 4 ? x[2] : ~x[2]);
                    }
                    dst[w] = dst[wpr + w] = dst[2 * wpr + w] = f;
                }
            };
            fill(P.node_kind[k], 8, o);
            for (size_t i = P.siblings() ? P.fam_start[k] : 0, end = P.siblings() ? P.fam_start[k + 1] : 0; i < end; i++)
                fill(P.fam_entry[4 * i], 0, table.data() + ((size_t)P.n_inputs + 3 * (P.live() + i)) * wpr);
            continue;
        }
        if (P.kind(k) == 1) {
            // a sum node: s = sum of w x mod 4 as two bit planes, (lo, hi) = (o[2 wpr ..], o[0 ..]), term by term
            // (-1 = 3 and -2 = 2 mod 4); then HI = s in {2, 3} = hi, MID = s in {1, 2} = lo ^ hi, LOW = s mod 2 = lo
            // (of three unit weights: MAJ, ONE_OR_TWO, XOR3)
            uint64_t *hi = o, *lo = o + 2 * wpr;
            for (uint32_t i = t0; i < t1; i++) {
                const uint64_t *sx = source(i, shifted[0]);
                const int32_t wt = P.term_weight[i];
                for (size_t w = 0; w < wpr; w++) {
                    const uint64_t x = word(sx, P.term_row[i], w);
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
        const uint32_t rx = P.term_row[t0], ry = P.term_row[t0 + 1];
        const uint64_t *sx = source(t0, shifted[0]), *sy = source(t0 + 1, shifted[1]);
        for (size_t w = 0; w < wpr; w++) {
            const uint64_t x = word(sx, rx, w), y = word(sy, ry, w);
            o[w] = x & y;
            o[wpr + w] = x | y;
            o[2 * wpr + w] = x ^ y;
        }
    }
    return SGFHE_OK;
}

// ---- the call arithmetic of a run (sgfhe_circuit_run, _run_ct[_ex], _run_probe) ----------------------------------
// Which rows, nodes and direct-pack jobs a level call covers, how a long job range is cut into grids, which
// ciphertexts of a pack group are bootstrapped (or lifted) first, and what a run's buffers must hold.  Pure functions
// of the plan: the engine walks them in this order -- every level L = 1 .. levels in calls of SGFHE_CIRCUIT_CALL_ROWS
// rows from row 0, then the pack groups of `cpc` ciphertexts from ciphertext 0 -- and that walk is the run's call
// numbering (tests/native/circuit_calls_sanitized.cpp restates it row by row).

// The call of level L that starts at row `row0` (a multiple of SGFHE_CIRCUIT_CALL_ROWS below the level's rows).
struct CircuitCall {
    uint32_t k0;       // the level's first node in `order`
    uint32_t rows;     // rows row0 .. row0 + rows of the level
    uint32_t ka, kb;   // the live nodes order[ka .. kb] (inclusive) those rows belong to
    size_t j0, j1;     // the direct-pack jobs [j0, j1) those nodes produce: with any, a direct run leaves the call
                       // un-reduced
    bool sum;          // one of the nodes is a sum node: the call takes an XOR3 kernel for its LOW rows
    bool lut;          // one of the nodes is a LUT node: the call carries a LUT descriptor
    bool fam;          // one of the nodes leads a live sibling: the call extracts further tables into the wire table
};
inline CircuitCall circuit_level_call(const CircuitPlan &P, uint32_t L, uint64_t row0, uint64_t instances) noexcept {
    CircuitCall C;
    C.k0 = P.level_start[L];
    C.rows = (uint32_t)std::min<uint64_t>(SGFHE_CIRCUIT_CALL_ROWS, P.level_rows(L, instances) - row0);
    C.ka = C.k0 + (uint32_t)(row0 / instances);
    C.kb = C.k0 + (uint32_t)((row0 + C.rows - 1) / instances);
    C.j0 = (size_t)(std::lower_bound(P.job_k.begin(), P.job_k.end(), C.ka) - P.job_k.begin());
    C.j1 = (size_t)(std::upper_bound(P.job_k.begin(), P.job_k.end(), C.kb) - P.job_k.begin());
    C.sum = P.gate3_in(C.ka, C.kb);
    C.lut = P.lut_in(C.ka, C.kb);
    C.fam = P.fam_in(C.ka, C.kb);
    return C;
}

// The grid that takes the jobs from `j` on of a call's range [j0, j1): a grid holds CIRCUIT_GRID_Y rows of workgroups,
// one per job, and the first grid of a call one more -- the block that scatters the call's rows into the wire table
// (`wires`).  The next grid starts at j + nj.
constexpr uint32_t CIRCUIT_GRID_Y = 65535;
struct CircuitJobChunk {
    uint32_t nj, wires;   // jobs j .. j + nj; 1 when the wire block rides along: gridDim.y = nj + wires
};
inline CircuitJobChunk circuit_job_chunk(size_t j, size_t j0, size_t j1) noexcept {
    const uint32_t wires = j == j0;
    return {(uint32_t)std::min<size_t>(j1 - j, CIRCUIT_GRID_Y - wires), wires};
}

// The ciphertexts q0 .. q0 + cnt of a pack group (q = output * blocks + block) that are not direct -- their output
// has no out_node -- as maximal runs of consecutive ones, `rank` counting them from 0 within the group: they are
// bootstrapped as one call (row = rank * n + bit) or lifted, one gather or lift per run.  `all`: every ciphertext
// counts (the plain form refreshes the whole group: one run).  Returns how many ciphertexts the runs hold; `runs` may
// be NULL to count only, otherwise it is cleared first (and is what may allocate here).
struct CircuitPackRun {
    size_t q, rank, len;
};
inline size_t circuit_pack_runs(const CircuitPlan &P, size_t blocks, size_t q0, size_t cnt, bool all,
                                std::vector<CircuitPackRun> *runs) {
    if (runs) runs->clear();
    size_t rank = 0;
    for (size_t q = q0; q < q0 + cnt; q++) {
        if (!all && P.out_node[q / blocks] != CIRC_NONE) continue;
        if (runs) {
            if (!runs->empty() && runs->back().q + runs->back().len == q) runs->back().len++;
            else runs->push_back({q, rank, 1});
        }
        rank++;
    }
    return rank;
}

// What the buffers of a run over `instances` hold at most, for rows of n + 1 words.  `pack`: `blocks` ciphertexts per
// output are packed (instances = blocks * n); `direct` (with pack) and `lift` (with direct) as the flags of
// sgfhe_circuit_run_ct_ex.
struct CircuitRunSizes {
    uint64_t max_rows;    // rows of the largest level call
    size_t n_ct;          // ciphertexts packed: n_outputs * blocks, 0 without pack
    size_t cpc;           // ciphertexts of the largest pack group: min(max(1, SGFHE_CIRCUIT_CALL_ROWS / n), n_ct)
    size_t max_ref;       // the most ciphertexts any group bootstraps first (circuit_pack_runs); 0 with lift
    uint64_t work_rows;   // rows of the largest bootstrap call of the run
};
inline CircuitRunSizes circuit_run_sizes(const CircuitPlan &P, uint64_t instances, size_t n, size_t blocks, bool pack,
                                         bool direct, bool lift) noexcept {
    CircuitRunSizes S = {};
    for (uint32_t L = 1; L <= P.levels; L++)
        S.max_rows = std::max(S.max_rows, std::min<uint64_t>(P.level_rows(L, instances), SGFHE_CIRCUIT_CALL_ROWS));
    direct = direct && pack;
    S.n_ct = pack ? (size_t)P.n_outputs * blocks : 0;
    S.cpc = std::min(std::max<size_t>(1, SGFHE_CIRCUIT_CALL_ROWS / n), S.n_ct);
    for (size_t q0 = 0; !(lift && direct) && q0 < S.n_ct; q0 += S.cpc)
        S.max_ref = std::max(S.max_ref, circuit_pack_runs(P, blocks, q0, std::min(S.cpc, S.n_ct - q0), !direct, nullptr));
    S.work_rows = std::max<uint64_t>(S.max_rows, (uint64_t)S.max_ref * n);
    return S;
}

}  // namespace sgfhe

// The opaque handle of the C ABI: a plan is host data, independent of any ctx.
struct sgfhe_circuit {
    sgfhe::CircuitPlan plan;
};
