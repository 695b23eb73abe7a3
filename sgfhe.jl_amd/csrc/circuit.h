// Host-side planner of sgfhe_circuit_* (include/sgfhe_hip.h).  Every create entry describes its
// circuit as one CircuitSpec -- the node view, the outputs, the lane group, the registers and the routes, with the
// kinds the entry admits as one number (CircuitNodes::max_kind) -- and circuit_plan(spec, plan) is the only way in.  It
// runs in named stages over one working struct (circuit_detail::PlanBuild): validate (pure: a refused circuit costs no
// allocation), prune and level ASAP, order, liveness and slots of the device wire table, LUT families, the CSR node
// table, outputs and direct-pack jobs, registers, and the one image a run uploads.  The three lists of references --
// node terms, outputs, next states -- go through one view (CircuitRefs), so every per-reference rule is written once.
// circuit_plain_bits evaluates a planned circuit in clear for the noise probe.
// The call arithmetic of a run lives here too (at the end): circuit_level_call, circuit_job_chunk, circuit_pack_runs and
// circuit_run_sizes say which rows, nodes and jobs a call covers and what the buffers hold; the engine only launches.
// So do the arguments of a run: every run entry fills one CircuitRequest, and circuit_request_check is its only judge.
// Plain C++, no HIP: tests/native/circuit_plan_sanitized.cpp, circuit_bits_sanitized.cpp, circuit_lanes_sanitized.cpp,
// circuit_gate3_sanitized.cpp, circuit_wsum_sanitized.cpp, circuit_lut_sanitized.cpp, circuit_lut_multi_sanitized.cpp,
// circuit_data_sanitized.cpp, circuit_calls_sanitized.cpp, circuit_steps_sanitized.cpp, circuit_routes_sanitized.cpp,
// circuit_request_sanitized.cpp and circuit_script_sanitized.cpp drive it under ASan / UBSan on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <new>
#include <queue>
#include <stdexcept>
#include <string>
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
    // behind every other table, and only in a plan with mask tables (sgfhe_circuit_create_masked, n_masks > 0): the
    // levels' (node, lane) pairs that take a row, then those that take none
    uint32_t pair_node = 0, pair_lane = 0, off_node = 0, off_lane = 0;
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
    // Lane masks (sgfhe_circuit_create_masked): a node whose mask index is k >= 1 takes a row only at the instances whose
    // lane t % group is set in masks[(k - 1) * group ..]; on the other lanes all three of its wires are the constant FALSE.
    // Index 0: every lane.  In a plan with masks every level is a list of (node, lane) PAIRS -- nodes ascending in
    // `order`, lanes ascending, an unmasked node all `group` of them -- and with per = instances / group row R of the
    // level is pair R / per at group R % per: instance (R % per) * group + lane.  The OFF pairs of a level are the
    // (masked node, lane not set) in the same order: the rows the level's fill writes as zeros.  All empty in a plan
    // without mask tables, whose rows stay rank * instances + instance.
    uint32_t n_masks = 0;
    std::vector<uint8_t> masks;         // [n_masks][group], 0 or 1
    std::vector<uint32_t> node_mask;    // [live], host only: the mask index of every live node in `order`
    std::vector<uint32_t> pair_start;   // [levels + 2]: level L's pairs are pair_node / pair_lane[pair_start[L] ..
                                        // pair_start[L + 1]) (level 0 holds none)
    std::vector<uint32_t> pair_node;    // [pairs]: the node's rank in its level, index in `order` - level_start[L]
    std::vector<uint32_t> pair_lane;    // [pairs]
    std::vector<uint32_t> off_start;    // [levels + 2], as pair_start
    std::vector<uint32_t> off_node;     // [off pairs]: rank in the level
    std::vector<uint32_t> off_lane;     // [off pairs]
    uint64_t rows_per_group = 0;        // level-call rows one group of `group` instances costs: the pairs of all levels
                                        // (live() * group in a plan without masks)
    // Every device table above in one array, uploaded once per run: node_kind, term_start, term_ref, term_shift,
    // term_weight, out_slot, out_ref, out_shift, input_slot, jobs (then fam_start, fam_entry; then next_ref, next_shift,
    // reg_scale, reg_index; then routes, term_route, out_route, next_route; then pair_node, pair_lane, off_node,
    // off_lane), each at its offset `at`
    std::vector<uint32_t> image;
    CircuitImage at;

    size_t live() const { return order.size(); }
    uint32_t n_stream() const { return n_inputs - n_regs; }   // the inputs a step brings
    bool lanes() const { return group > 1; }   // (group 1 admits no shift but 0)
    bool masked() const { return n_masks != 0; }   // the levels' rows are (node, lane) pairs
    // whether live node k takes a row at lane l
    bool lane_on(size_t k, uint32_t l) const {
        return !masked() || !node_mask[k] || masks[(size_t)(node_mask[k] - 1) * group + l] != 0;
    }
    uint32_t level_pairs(uint32_t L) const { return pair_start[L + 1] - pair_start[L]; }
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
    // rows of level L in a run over `instances`; row = rank_in_level * instances + instance -- in a plan with masks
    // (`instances` a multiple of the group) row = pair * (instances / group) + group of the instance
    uint64_t level_rows(uint32_t L, uint64_t instances) const {
        if (masked()) return (uint64_t)level_pairs(L) * (instances / group);
        return (uint64_t)(level_start[L + 1] - level_start[L]) * instances;
    }
};

namespace circuit_detail {
inline uint32_t wire_id(uint32_t ref) { return ref & ~CIRC_NOT; }
}  // namespace circuit_detail

// One view of the nodes' inputs behind every entry.  `arity` 2 or 3: the [n_gates][arity] arrays of
// sgfhe_circuit_create_lanes / sgfhe_circuit_create3 (a third reference CIRC_NO_INPUT leaves a two-input node; with
// one, the node is the sum node of three unit weights).  `arity` 0: the CSR arrays of sgfhe_circuit_create_w and every
// later entry.  Term i of the circuit is refs[i], shifts[i] (NULL: 0), weights[i] (NULL: 1); node g's terms are
// first(g) .. first(g) + count(g).  `max_kind` is the largest kind[g] the entry admits: 1 a sum node; 2 a LUT node of
// table tables[g] (sgfhe_circuit_create_lut); 3 a sibling -- no terms, table tables[g], a further table on the bootstrap
// of its LEADER, the nearest earlier LUT node (sgfhe_circuit_create_lut_multi); 5 kinds 4 and 5, a LUT node and a
// sibling with tables[g] a plane index below `n_planes` (sgfhe_circuit_create_data and later).
struct CircuitNodes {
    int arity = 2;
    const uint32_t *refs = nullptr;
    const int32_t *shifts = nullptr;
    const uint32_t *kind = nullptr, *start = nullptr;
    const int32_t *weights = nullptr;
    const uint32_t *tables = nullptr;
    uint32_t max_kind = 1;
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
// the [n_gates][arity] arrays, arity 2 or 3
inline CircuitNodes circuit_nodes_arity(int arity, const uint32_t *gates, const int32_t *gate_shift) {
    CircuitNodes N;
    N.arity = arity, N.refs = gates, N.shifts = gate_shift;
    return N;
}
// the CSR arrays of an entry that admits kinds 0 .. max_kind (1, 2, 3 or 5; planes only at 5)
inline CircuitNodes circuit_nodes_csr(uint32_t max_kind, const uint32_t *node_kind, const uint32_t *node_start,
                                      const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                      const uint32_t *node_table = nullptr, uint32_t n_planes = 0) {
    CircuitNodes N;
    N.arity = 0, N.refs = term_ref, N.shifts = term_shift, N.kind = node_kind, N.start = node_start;
    N.weights = term_weight, N.tables = node_table, N.max_kind = max_kind, N.n_planes = n_planes;
    return N;
}

// The registers of sgfhe_circuit_create_seq: input wires 0 .. n_regs (0: none); next_ref [n_regs] wire references
// validated like outputs, next_shift [n_regs] (NULL: all 0), reg_scale [n_regs] (NULL: all 0; each 0, 1 or 2).
struct CircuitRegs {
    uint32_t n_regs = 0;
    const uint32_t *next_ref = nullptr;
    const int32_t *next_shift = nullptr;
    const uint32_t *reg_scale = nullptr;
    uint32_t scale(uint32_t i) const { return reg_scale ? reg_scale[i] : 0u; }
};

// The lane routes of sgfhe_circuit_create_routed: routes [n_routes][group] (n_routes 0: none), entries in [0, group) or
// CIRC_ROUTE_FALSE; term_route beside the term arrays, out_route [n_outputs], next_route [n_regs] (each NULL: all 0):
// 0 = none, k >= 1 = table k - 1, and then the reference's shift must be 0.
struct CircuitRoutes {
    uint32_t n_routes = 0;
    const int32_t *routes = nullptr;
    const uint32_t *term_route = nullptr, *out_route = nullptr, *next_route = nullptr;
};

// The lane masks of sgfhe_circuit_create_masked: masks [n_masks][group] (n_masks 0: none), every entry 0 or 1 and every
// table with a lane set; node_mask [n_gates] (NULL: all 0): 0 = every lane, k >= 1 = table k - 1.  No sibling carries one.
struct CircuitMasks {
    uint32_t n_masks = 0;
    const uint8_t *masks = nullptr;
    const uint32_t *node_mask = nullptr;
    uint32_t of(size_t g) const { return node_mask ? node_mask[g] : 0u; }
};

// One list of references -- a node's terms, the outputs, the registers' next states -- as the per-reference rules and
// the plan's tables read it: reference i is ref[i] at the lane shift shift[i] (NULL: 0) or through route[i] (NULL: 0).
// It may name the constant or a wire id below `wires`, of the scale want(i): position i of a LUT node's terms (`lut`)
// reads scale 2 - i, every other reference scale[i] (NULL: 0).
struct CircuitRefs {
    const uint32_t *ref;
    const int32_t *shift;
    const uint32_t *route;
    size_t count;
    uint64_t wires;
    const uint32_t *scale;
    bool lut;
    int32_t shift_of(size_t i) const { return shift ? shift[i] : 0; }
    uint32_t route_of(size_t i) const { return route ? route[i] : 0u; }
    uint32_t want(size_t i) const { return lut ? 2u - (uint32_t)i : (scale ? scale[i] : 0u); }
};

// A circuit as every entry describes it: wires 0 .. n_inputs are inputs, node g's three wires n_inputs + 3 g + 0 / 1 / 2.
// out_shift NULL: all 0.  The registers' next-state references count as readers exactly as outputs do -- liveness,
// levels, slot lifetime -- so the plan's order, levels and slots are those of the plan whose outputs are outputs ++
// next_ref.  Nothing but the route tables of the plan sees the routes, and with n_routes = 0 the plan is the plan
// without them, image word for word.
struct CircuitSpec {
    uint32_t n_inputs = 0;
    CircuitNodes nodes;
    size_t n_gates = 0;
    const uint32_t *outputs = nullptr;
    const int32_t *out_shift = nullptr;
    size_t n_outputs = 0;
    uint32_t group = 1;
    CircuitRegs regs;
    CircuitRoutes routes;
    CircuitMasks masks;   // (numbering, pruning, liveness, levels and slots do not see them)

    uint64_t n_wires() const { return (uint64_t)n_inputs + 3 * (uint64_t)n_gates; }
    // the three lists of references; node g's terms may name the wires before its own
    CircuitRefs terms(size_t g) const {
        const size_t i = nodes.first(g);
        return {nodes.refs + i, nodes.shifts ? nodes.shifts + i : nullptr, routes.term_route ? routes.term_route + i : nullptr,
                nodes.count(g), (uint64_t)n_inputs + 3 * (uint64_t)g, nullptr, nodes.is_lut(g)};
    }
    CircuitRefs outs() const { return {outputs, out_shift, routes.out_route, n_outputs, n_wires(), nullptr, false}; }
    CircuitRefs nexts() const {   // a register is fed the constant or a wire of its own scale
        return {regs.next_ref, regs.next_shift, routes.next_route, regs.n_regs, n_wires(), regs.reg_scale, false};
    }
    // The scale rule: a wire carries its bit at the codeword Dr >> scale.  Scale 0: stream inputs, every wire of a
    // classic or sum node, wire +0 of a LUT node; wires +1 and +2 of a LUT node have scales 1 and 2; a register has the
    // scale it was given.
    uint32_t scale_of(uint32_t id) const {
        if (id < n_inputs) return id < regs.n_regs ? regs.scale(id) : 0u;
        return nodes.is_lut((id - n_inputs) / 3) ? (id - n_inputs) % 3 : 0u;
    }
};

namespace circuit_detail {

// The CSR of an arity-0 entry, node by node, before a term of any node is read: kinds the entry admits, ascending
// starts, the term count and weights of every kind, tables and planes in range, siblings behind a LUT node in a family
// that has room.
inline bool csr_ok(const CircuitSpec &S) noexcept {
    const CircuitNodes &N = S.nodes;
    if (N.max_kind != 1 && N.max_kind != 2 && N.max_kind != 3 && N.max_kind != 5) return false;
    if (N.n_planes > SGFHE_CIRCUIT_MAX_PLANES || (N.n_planes && N.max_kind < 5)) return false;
    if (!S.n_gates) return true;
    if (!N.kind || !N.start || !N.weights || N.start[0] != 0 || (N.max_kind >= 2 && !N.tables)) return false;
    auto table_ok = [&](size_t g) { return N.tables[g] < (N.is_data(g) ? N.n_planes : 256u); };
    size_t family = 0;   // members so far of the family node g - 1 belongs to (0: it is no LUT node)
    for (size_t g = 0; g < S.n_gates; g++) {
        if (N.kind[g] > N.max_kind || N.start[g + 1] < N.start[g]) return false;
        const size_t nj = N.count(g);
        if (N.is_sibling(g)) {   // a sibling: no terms, a table, behind a LUT node or a sibling, in a family that has room
            if (nj != 0 || !table_ok(g) || family == 0 || family >= SGFHE_LUT_MAX_TABLES) return false;
            family++;
            continue;
        }
        family = N.is_lut(g) ? 1 : 0;
        if (N.is_lut(g)) {   // a LUT node: three unit terms (positions 0, 1, 2), a table of 8 entries (or a plane)
            if (nj != 3 || !table_ok(g)) return false;
        } else if (N.kind[g] == 0 ? nj != 2 : (nj < 1 || nj > SGFHE_CIRCUIT_MAX_TERMS)) {
            return false;
        }
        for (size_t i = N.first(g); i < N.first(g) + nj; i++) {
            const int32_t w = N.weights[i];
            if (N.kind[g] != 1 ? w != 1 : (w == 0 || w < -2 || w > 2)) return false;
        }
    }
    return true;
}

// The per-reference rules, each once, over a list `V` of a circuit whose sizes and CSR hold: the id names the constant
// or a wire the list may read (a node: earlier wires only; CIRC_NO_INPUT is above every wire id, so anywhere but beside
// a two-input node of the [n_gates][3] arrays it fails here), of the wanted scale; the shift stays inside the group (in
// 64 bits: -INT32_MIN does not exist); the route index names a table, and never beside a shift.
inline bool refs_ok(const CircuitSpec &S, const CircuitRefs &V) noexcept {
    for (size_t i = 0; i < V.count; i++) {
        const uint32_t id = wire_id(V.ref[i]), k = V.route_of(i);
        const int64_t d = V.shift_of(i);
        if (id != CIRC_FALSE && (id >= V.wires || S.scale_of(id) != V.want(i))) return false;
        if ((d < 0 ? -d : d) >= (int64_t)S.group) return false;
        if (k > S.routes.n_routes || (k != 0 && d != 0)) return false;
    }
    return true;
}

// Stage 1, validate: whether `S` is a circuit at all.  Pure -- it reads the caller's arrays and allocates nothing, so
// a refused circuit costs no allocation.  Every size below 2^31, wire ids below the constant, the registers among the
// inputs, every route entry a lane of the group or the fill, the CSR, then every reference of the three lists.
inline bool valid(const CircuitSpec &S) noexcept {
    const CircuitNodes &N = S.nodes;
    const CircuitRegs &R = S.regs;
    const CircuitRoutes &T = S.routes;
    if (S.n_outputs < 1 || !S.outputs || (S.n_gates && !N.refs) || S.group < 1) return false;
    if (S.n_inputs >= 0x80000000u || S.n_gates >= 0x80000000u || S.n_outputs >= 0x80000000u) return false;
    if (S.n_wires() >= CIRC_FALSE) return false;
    if (R.n_regs > S.n_inputs || (R.n_regs && !R.next_ref)) return false;
    for (uint32_t i = 0; i < R.n_regs; i++)
        if (R.scale(i) > 2u) return false;
    if (T.n_routes > SGFHE_CIRCUIT_MAX_ROUTES || (T.n_routes && !T.routes)) return false;
    for (size_t i = 0; i < (size_t)T.n_routes * S.group; i++)
        if (T.routes[i] < CIRC_ROUTE_FALSE || T.routes[i] >= (int64_t)S.group) return false;
    if (!N.arity && !csr_ok(S)) return false;
    const CircuitMasks &K = S.masks;
    if (K.n_masks > SGFHE_CIRCUIT_MAX_MASKS || (K.n_masks && !K.masks)) return false;
    for (uint32_t k = 0; k < K.n_masks; k++) {   // entries 0 or 1, and a lane set in every table
        bool any = false;
        for (size_t l = 0; l < S.group; l++) {
            if (K.masks[(size_t)k * S.group + l] > 1) return false;
            any = any || K.masks[(size_t)k * S.group + l];
        }
        if (!any) return false;
    }
    for (size_t g = 0; g < S.n_gates; g++)
        if (K.of(g) > K.n_masks || (K.of(g) && N.is_sibling(g))) return false;
    for (size_t g = 0; g < S.n_gates; g++)
        if (!refs_ok(S, S.terms(g))) return false;
    return refs_ok(S, S.outs()) && refs_ok(S, S.nexts());
}

// What the stages behind `valid` share: the circuit, the plan they fill, and the per-node and per-wire working tables.
// Each stage reads what the stages before it left; any of them may throw std::bad_alloc (std::length_error: `image`).
struct PlanBuild {
    const CircuitSpec &S;
    const CircuitNodes &N;
    CircuitPlan &P;
    const uint32_t NG, n_inputs;
    static constexpr uint32_t UNREAD = 0;   // (no wire is read at level 0)
    uint32_t END = 0;                       // the "level" of the readers behind the last one: outputs and next states
    std::vector<uint32_t> leader;           // [n_gates]: a sibling's leader, every other node itself
    std::vector<uint8_t> live;              // [n_gates]: an output or next state reaches the node
    std::vector<uint32_t> last_read;        // [wires]: the last level that reads the wire, UNREAD .. END
    std::vector<uint32_t> slot_of;          // [wires]: CIRC_NONE for a wire nothing reads
    std::vector<uint32_t> sib_index;        // [n_gates]: a live sibling's index in fam_node
    std::vector<uint32_t> rank_of;          // [n_gates]: a live node's index in `order`

    PlanBuild(const CircuitSpec &S, CircuitPlan &P)
        : S(S), N(S.nodes), P(P), NG((uint32_t)S.n_gates), n_inputs(S.n_inputs) {}

    // producing node of a wire, -1 for inputs and the constant
    int64_t node_of(uint32_t id) const {
        return (id == CIRC_FALSE || id < n_inputs) ? -1 : (int64_t)((id - n_inputs) / 3);
    }
    // the live siblings of node g, in ascending index
    template <class F> void each_sibling(uint32_t g, F &&fn) const {
        for (uint32_t h = g + 1; h < NG && N.is_sibling(h); h++)
            if (live[h]) fn(h);
    }
    // the wires of a list, the constant left out
    template <class F> static void each_wire(const CircuitRefs &V, F &&fn) {
        for (size_t i = 0; i < V.count; i++)
            if (wire_id(V.ref[i]) != CIRC_FALSE) fn(wire_id(V.ref[i]));
    }
    // Outputs and next states read at END: the wires both lists name (the feedback reads at the end of the step)
    template <class F> void each_end_wire(F &&fn) const {
        each_wire(S.outs(), fn);
        each_wire(S.nexts(), fn);
    }
    // Reference i of a list as the plan's tables hold it: the slot for the wire id (NOT kept); shift and route dropped
    // on a reference to the constant, and no route kept in a plan without tables.  A shifted reference reads other ROWS
    // of the slot it names, nothing else: the wire is of an earlier level (or an input), so all its rows are written
    // before the reading level's first call in stream order, and its slot is held until the last level that reads the
    // wire ends, whichever instance is read.  The slot rule therefore knows no shift.
    struct Ref {
        uint32_t ref;
        int32_t shift;
        uint32_t route;
    };
    Ref slot_ref(const CircuitRefs &V, size_t i) const {
        const uint32_t id = wire_id(V.ref[i]);
        if (id == CIRC_FALSE) return {V.ref[i], 0, 0u};
        return {slot_of[id] | (V.ref[i] & CIRC_NOT), V.shift_of(i), P.n_routes ? V.route_of(i) : 0u};
    }
    // the same reference as a probe row (CircuitPlan::term_row)
    uint32_t row_ref(uint32_t ref) const {
        const uint32_t id = wire_id(ref);
        const int64_t g = node_of(id);
        if (g < 0) return ref;
        const size_t node_row = N.is_sibling((size_t)g) ? P.live() + sib_index[g] : rank_of[g];
        return (uint32_t)(n_inputs + 3 * node_row + (id - n_inputs) % 3) | (ref & CIRC_NOT);
    }
    void term(const Ref &r, int32_t weight) {
        P.term_ref.push_back(r.ref);
        P.term_shift.push_back(r.shift);
        P.term_weight.push_back(weight);
        if (P.n_routes) P.term_route.push_back(r.route);
    }

    // Stage 2, prune and level: the plan's scalars; a node is live when an output or next state reaches it (walk back,
    // last node first), a leader when any of its siblings is; level ASAP = 1 + the largest level of the node's input
    // nodes (inputs and the constant: 0), a sibling has its leader's level.
    void prune_and_level() {
        P.n_inputs = n_inputs, P.n_gates = NG, P.n_outputs = (uint32_t)S.n_outputs;
        P.group = S.group, P.n_planes = N.n_planes, P.n_regs = S.regs.n_regs, P.n_routes = S.routes.n_routes;
        if (P.n_routes) P.routes.assign(S.routes.routes, S.routes.routes + (size_t)P.n_routes * P.group);
        P.n_masks = S.masks.n_masks;
        if (P.n_masks) P.masks.assign(S.masks.masks, S.masks.masks + (size_t)P.n_masks * P.group);
        leader.resize(NG);
        for (uint32_t g = 0; g < NG; g++) leader[g] = N.is_sibling(g) ? leader[g - 1] : g;
        live.assign(NG, 0);
        auto reach = [&](uint32_t id) {
            if (node_of(id) >= 0) live[node_of(id)] = 1;
        };
        each_end_wire(reach);
        for (uint32_t g = NG; g-- > 0;) {
            if (!live[g]) continue;
            live[leader[g]] = 1;
            each_wire(S.terms(g), reach);
        }
        P.level.assign(NG, 0);
        for (uint32_t g = 0; g < NG; g++) {
            if (!live[g]) continue;
            if (N.is_sibling(g)) { P.level[g] = P.level[leader[g]]; continue; }
            uint32_t L = 0;
            each_wire(S.terms(g), [&](uint32_t id) {
                if (node_of(id) >= 0) L = std::max(L, P.level[node_of(id)]);
            });
            P.level[g] = L + 1;
            P.levels = std::max(P.levels, L + 1);
        }
        END = P.levels + 1;
    }

    // Stage 3, order: the live nodes that take a row (no sibling does), level by level, ascending node index within a
    // level (counting sort); level_start, widest, and every live node's rank.
    void order() {
        auto takes_row = [&](uint32_t g) { return P.level[g] && !N.is_sibling(g); };
        P.level_start.assign((size_t)P.levels + 2, 0);
        for (uint32_t g = 0; g < NG; g++)
            if (takes_row(g)) P.level_start[P.level[g] + 1]++;
        for (uint32_t L = 1; L <= P.levels; L++) {
            P.widest = std::max(P.widest, P.level_start[L + 1]);
            P.level_start[L + 1] += P.level_start[L];
        }
        P.order.resize(P.level_start[P.levels + 1]);
        std::vector<uint32_t> fill(P.level_start.begin(), P.level_start.end() - 1);
        for (uint32_t g = 0; g < NG; g++)
            if (takes_row(g)) P.order[fill[P.level[g]]++] = g;
        rank_of.assign(NG, CIRC_NONE);
        for (size_t k = 0; k < P.live(); k++) rank_of[P.order[k]] = (uint32_t)k;
    }

    // Stage 4, liveness and slots: the last level that reads each wire; a wire written at level L takes the lowest free
    // slot, and a slot is free again after the last level that reads its wire (so no call of level L overwrites what a
    // later call of L gathers).  A sibling's wires are written by its leader's call: slots of the same level.
    void slots() {
        last_read.assign((size_t)S.n_wires(), UNREAD);
        for (uint32_t g : P.order)
            each_wire(S.terms(g), [&](uint32_t id) { last_read[id] = std::max(last_read[id], P.level[g]); });
        each_end_wire([&](uint32_t id) { last_read[id] = END; });
        slot_of.assign((size_t)S.n_wires(), CIRC_NONE);
        std::vector<std::vector<uint32_t>> release((size_t)END + 1);   // slots freed after level L
        std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_slots;
        auto take = [&](uint32_t id) {
            if (last_read[id] == UNREAD) return;
            uint32_t s;
            if (free_slots.empty()) s = P.slots++;
            else { s = free_slots.top(); free_slots.pop(); }
            slot_of[id] = s;
            release[last_read[id]].push_back(s);
        };
        auto take_node = [&](uint32_t g) {
            for (uint32_t w = 0; w < 3; w++) take(n_inputs + 3 * g + w);
        };
        for (uint32_t i = 0; i < n_inputs; i++) take(i);
        P.input_slot.assign(slot_of.begin(), slot_of.begin() + n_inputs);
        for (uint32_t L = 1; L <= P.levels; L++) {
            for (uint32_t s : release[L - 1]) free_slots.push(s);
            for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++) {
                take_node(P.order[k]);
                each_sibling(P.order[k], take_node);
            }
        }
    }

    // Stage 5, families: every live node's live siblings as one CSR over `order` -- their tables and slots, and their
    // numbering (fam_node, which numbers a sibling's probe rows).
    void families() {
        sib_index.assign(NG, CIRC_NONE);
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
    }

    // Stage 6, node table: every live node's kind word, its terms in the caller's order (as slot references and as
    // probe rows), the slots of its three wires, and the running counts of sum and LUT nodes.
    void node_table() {
        P.out_slot.resize(3 * P.live());
        P.sum_before.assign(P.live() + 1, 0);
        P.lut_before.assign(P.live() + 1, 0);
        for (size_t k = 0; k < P.live(); k++) {
            const size_t g = P.order[k];
            const CircuitRefs V = S.terms(g);
            P.node_kind.push_back(N.kind_of(g) | (N.is_lut(g) ? N.table_word(g, 8) : 0u));
            P.term_start.push_back((uint32_t)P.term_ref.size());
            for (size_t i = 0; i < V.count; i++) {
                term(slot_ref(V, i), N.weight(N.first(g) + i));
                P.term_row.push_back(row_ref(V.ref[i]));
            }
            for (uint32_t w = 0; w < 3; w++) P.out_slot[3 * k + w] = slot_of[n_inputs + 3 * g + w];
            P.sum_before[k + 1] = P.sum_before[k] + (P.kind(k) == 1);
            P.lut_before[k + 1] = P.lut_before[k] + (P.kind(k) == 2);
        }
    }

    // Stage 7, outputs and jobs: the outputs as slot references; the pack stage's pseudo-level behind the node table --
    // node live() + o is (TRUE, output o), the pair of fhe.jl:669-673; which outputs are gate rows of a level call
    // (out_node, out_gate), and those as direct-pack jobs by producing node.
    void outputs_and_jobs() {
        const CircuitRefs V = S.outs();
        P.out_node.assign(V.count, CIRC_NONE);
        P.out_gate.assign(V.count, 0);
        for (size_t o = 0; o < V.count; o++) {
            const Ref r = slot_ref(V, o);
            P.out_ref.push_back(r.ref);
            P.out_shift.push_back(r.shift);
            if (P.n_routes) P.out_route.push_back(r.route);
            P.node_kind.push_back(0u);
            P.term_start.push_back((uint32_t)P.term_ref.size());
            term({CIRC_FALSE | CIRC_NOT, 0, 0u}, 1);
            term(r, 1);
            const uint32_t id = wire_id(V.ref[o]);
            const int64_t g = node_of(id);
            // (a routed output is no gate row in order, even under the identity table: refreshed or lifted, as a shifted one)
            if (g < 0 || r.shift != 0 || r.route != 0) continue;
            if ((id - n_inputs) % 3 == 2 && !N.classic((size_t)g)) continue;   // LOW: linear over Z_r, no gate row
            if (N.is_lut((size_t)g)) continue;   // wire +0 of a LUT node: refreshed or lifted, as a LOW wire is
            if (S.masks.of((size_t)g)) continue;   // a masked node has no gate row on its off lanes: refreshed or lifted
            P.out_node[o] = rank_of[g];
            P.out_gate[o] = (id - n_inputs) % 3;
        }
        P.term_start.push_back((uint32_t)P.term_ref.size());
        std::vector<uint32_t> byk;
        for (uint32_t o = 0; o < V.count; o++)
            if (P.out_node[o] != CIRC_NONE) byk.push_back(o);
        std::sort(byk.begin(), byk.end(), [&](uint32_t x, uint32_t y) {   // (outputs of one node in ascending index)
            return P.out_node[x] != P.out_node[y] ? P.out_node[x] < P.out_node[y] : x < y;
        });
        for (uint32_t o : byk) {
            const uint32_t k = P.out_node[o], L = P.level[P.order[k]];
            P.job_k.push_back(k);
            P.jobs.insert(P.jobs.end(), {o, k - P.level_start[L], P.out_gate[o] | (P.out_ref[o] & CIRC_NOT)});
        }
    }

    // Stage 8, registers: the next states as slot references, each register's scale and its index in the state buffer.
    void registers() {
        const CircuitRefs V = S.nexts();
        for (uint32_t i = 0; i < V.count; i++) {
            const Ref r = slot_ref(V, i);
            P.next_ref.push_back(r.ref);
            P.next_shift.push_back(r.shift);
            P.reg_scale.push_back(S.regs.scale(i));
            P.reg_index.push_back(i);
            if (P.n_routes) P.next_route.push_back(r.route);
        }
    }

    // A masked LUT node must not lead a live sibling: the sibling's wires are written inside the bootstrap call
    // (k_final_lut_multi), which knows no off lanes.  Read after stage 2, which says which siblings are live.
    bool masked_family() const {
        for (uint32_t g = 0; g < NG; g++)
            if (live[g] && N.is_sibling(g) && S.masks.of(leader[g])) return true;
        return false;
    }

    // Stage 8b, masks: the rows a group costs; in a plan with mask tables every live node's mask index, and every
    // level's pairs -- those that take a row, and the off pairs of its masked nodes.
    void mask_pairs() {
        P.rows_per_group = (uint64_t)P.live() * P.group;
        if (!P.n_masks) return;
        P.rows_per_group = 0;
        for (size_t k = 0; k < P.live(); k++) P.node_mask.push_back(S.masks.of(P.order[k]));
        P.pair_start.assign((size_t)P.levels + 2, 0);
        P.off_start.assign((size_t)P.levels + 2, 0);
        for (uint32_t L = 1; L <= P.levels; L++) {
            for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++)
                for (uint32_t l = 0; l < P.group; l++) {
                    const bool on = P.lane_on(k, l);
                    (on ? P.pair_node : P.off_node).push_back(k - P.level_start[L]);
                    (on ? P.pair_lane : P.off_lane).push_back(l);
                }
            if (P.pair_node.size() >= 0x100000000ull) throw std::length_error("circuit pairs");
            P.pair_start[L + 1] = (uint32_t)P.pair_node.size();
            P.off_start[L + 1] = (uint32_t)P.off_node.size();
        }
        P.rows_per_group = P.pair_node.size();
    }

    // Stage 9, image: every device table in the order CircuitPlan::image states, each at its offset in P.at.
    void image() {
        auto place = [&](const auto &tab) -> uint32_t {
            const size_t at = P.image.size();
            if (at + tab.size() >= 0x100000000ull) throw std::length_error("circuit image");
            for (auto v : tab) P.image.push_back((uint32_t)v);
            return (uint32_t)at;
        };
        P.image.reserve(P.node_kind.size() + P.term_start.size() + 3 * P.term_ref.size() + P.out_slot.size() +
                        2 * (size_t)P.n_outputs + n_inputs + P.jobs.size() + 4 * (size_t)P.n_regs + P.routes.size() +
                        P.term_route.size() + P.out_route.size() + P.next_route.size() + 2 * P.pair_node.size() +
                        2 * P.off_node.size());
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
        if (P.n_regs) {
            P.at.next_ref = place(P.next_ref);
            P.at.next_shift = place(P.next_shift);
            P.at.next_scale = place(P.reg_scale);
            P.at.reg_index = place(P.reg_index);
        }
        if (P.n_routes) {
            P.at.routes = place(P.routes);
            P.at.term_route = place(P.term_route);
            P.at.out_route = place(P.out_route);
            if (P.n_regs) P.at.next_route = place(P.next_route);
        }
        if (P.n_masks) {
            P.at.pair_node = place(P.pair_node);
            P.at.pair_lane = place(P.pair_lane);
            P.at.off_node = place(P.off_node);
            P.at.off_lane = place(P.off_lane);
        }
        P.at.words = (uint32_t)P.image.size();
    }
};

}  // namespace circuit_detail

// Builds `P` from the circuit `S`, stage by stage.  Returns SGFHE_OK, SGFHE_ERR_INVALID_ARG for a malformed circuit (`P`
// is not touched) or for a masked LUT node that leads a live sibling (known after pruning: `P` is reset),
// SGFHE_ERR_OOM when an allocation fails (`P` is reset).  Nothing throws out of it.
inline int32_t circuit_plan(const CircuitSpec &S, CircuitPlan &P) noexcept {
    if (!circuit_detail::valid(S)) return SGFHE_ERR_INVALID_ARG;
    try {
        P = CircuitPlan();
        circuit_detail::PlanBuild B(S, P);
        B.prune_and_level();
        if (B.masked_family()) {
            P = CircuitPlan();
            return SGFHE_ERR_INVALID_ARG;
        }
        B.order();
        B.slots();
        B.families();
        B.node_table();
        B.outputs_and_jobs();
        B.registers();
        B.mask_pairs();
        B.image();
    } catch (...) {   // std::bad_alloc, std::length_error: nothing else allocates or throws here
        P = CircuitPlan();
        return SGFHE_ERR_OOM;
    }
    return SGFHE_OK;
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
// NULL when the plan has planes and instances > 0).  In a plan with lane masks the three rows of a masked node are 0 on
// the lanes that are off.
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
    // a masked node's three rows are FALSE on its off lanes (it leads no live sibling), instance by instance
    auto mask_rows = [&](size_t k, uint64_t *o) {
        if (!P.masked() || !P.node_mask[k]) return;
        for (size_t t = 0; t < instances; t++)
            if (!P.lane_on(k, (uint32_t)(t % (size_t)G)))
                for (size_t w = 0; w < 3; w++) o[w * wpr + t / 64] &= ~(1ull << (t % 64));
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
            mask_rows(k, o);
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
            mask_rows(k, o);
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
        mask_rows(k, o);
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
    if (P.masked()) {   // the nodes of the first and the last pair
        const uint64_t per = instances / P.group;
        C.ka = C.k0 + P.pair_node[P.pair_start[L] + (size_t)(row0 / per)];
        C.kb = C.k0 + P.pair_node[P.pair_start[L] + (size_t)((row0 + C.rows - 1) / per)];
    } else {
        C.ka = C.k0 + (uint32_t)(row0 / instances);
        C.kb = C.k0 + (uint32_t)((row0 + C.rows - 1) / instances);
    }
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

// ---- the arguments of a run ----------------------------------------------------------------------------------------
// Everything a caller can pass to a run entry (sgfhe_circuit_run*, include/sgfhe_hip.h); an entry leaves what it does
// not take as it is here.  The form bits say which entry it is: `ct` the ciphertext forms, `stepped` the _steps
// entries, `probe` the _probe entries, `device` the _device entries -- and with them which text a refusal carries,
// since every entry of one form speaks under one name.
struct CircuitRequest {
    bool ct = false, stepped = false, probe = false, device = false;
    bool with_data = false;    // the entry takes `data`: the _data, _steps and _device entries
    void *stream = nullptr;    // device form: the caller's hipStream_t, NULL for the ctx's own
    size_t count = 0;          // instances, or -- ct -- blocks of n instances
    size_t steps = 1;          // stepped: the plan is evaluated so often; in, in_a / in_b, data are then per step,
                               // out, out_w / out_v per emitted step
    size_t N = 0;              // ct: words of a ciphertext, n (PackedCiphertext) or m (Ciphertext)
    const uint64_t *in = nullptr;                        // [wire][instances][n + 1]
    const uint64_t *in_a = nullptr, *in_b = nullptr;     // ct: [wire][blocks][N]
    const uint64_t *state_in = nullptr;                  // stepped: [n_regs][instances][n + 1], NULL: every register FALSE
    const uint64_t *state_a = nullptr, *state_b = nullptr;   // stepped ct: [n_regs][blocks][N], both NULL: FALSE
    const uint8_t *data = nullptr;                       // [n_planes][instances] of a plan that has planes
    const uint8_t *emit = nullptr;                       // stepped: [steps] in host memory, NULL: every step's outputs
    uint64_t *out = nullptr;                             // [n_outputs][instances][n + 1]; optional in the ct and stepped forms
    uint64_t *out_w = nullptr, *out_v = nullptr;         // ct: [n_outputs][blocks][m], or both NULL
    uint64_t *state_out = nullptr;                       // stepped: [n_regs][instances][n + 1] after the last step, optional
    uint32_t flags = 0;                                  // ct: SGFHE_CIRCUIT_PACK_DIRECT, SGFHE_CIRCUIT_PACK_LIFT
    const uint64_t *sk = nullptr;                        // probe: n key bits,
    const uint8_t *in_bits = nullptr;                    // the plaintext bit of every input LWE [n_inputs][instances],
    uint64_t *stats = nullptr;                           // the records [n_inputs + 3 n_gates][8], by wire id
    const struct CircuitScript *script = nullptr;        // sgfhe_debug_circuit_script: the run's calls are scripted (below)

    bool packs() const;                                  // ct: the run has a pack stage (out_w, or the script's tail_in)
    bool direct() const { return (flags & SGFHE_CIRCUIT_PACK_DIRECT) != 0; }
    bool lift() const { return (flags & SGFHE_CIRCUIT_PACK_LIFT) != 0; }   // (with direct)
};

// A scripted run (sgfhe_debug_circuit_script): the run of a host-form request with every bootstrap call and the pack
// tail replaced by the caller's arrays.  The scripted calls are those of circuit_script_calls, in that order; each
// block is compact.
struct CircuitScript {
    const uint64_t *results = nullptr;   // per call [rows][3][n + 1] words of Z_r, or -- un-reduced -- [rows][3][n + 1][2]
    uint64_t *staged = nullptr;          // log, per call [rows][2][n + 1]: input 1 then input 2 of every row, a then b
    uint32_t *lut = nullptr;             // log, per call [rows]: the call's LUT descriptor, 0 for a call that carries none
    uint64_t *tail_in = nullptr;         // log [emitted steps][n_ct][n][n + 1][2]: what the tail would read; NULL: no pack stage
};
inline bool CircuitRequest::packs() const { return ct && (out_w || (script && script->tail_in)); }

// The scripted calls of a run: every step's level calls (circuit_level_call, every level from row 0), then -- an emitted
// step of a run that packs -- the refresh call of every pack group that has one (circuit_pack_runs; none with lift).  A
// call is un-reduced (16-byte residues mod Q) where the real run leaves it so: a level call of a direct run that
// produces a direct output, and every refresh call.  `emit` is read ([steps], host memory; NULL: every step).  Returns
// the number of calls; `calls` may be NULL to count only (and is otherwise what may allocate here).
struct CircuitScriptCall {
    uint32_t rows;
    bool raw;   // un-reduced
    bool lut;   // the call carries a LUT descriptor
};
inline size_t circuit_script_calls(const CircuitPlan &P, const CircuitRequest &q, size_t n, uint64_t instances,
                                   std::vector<CircuitScriptCall> *calls) {
    if (calls) calls->clear();
    const bool pack = q.packs(), direct = pack && q.direct(), lift = direct && q.lift();
    const CircuitRunSizes sz = circuit_run_sizes(P, instances, n, q.ct ? q.count : 0, pack, direct, lift);
    size_t count = 0;
    for (size_t s = 0; s < (q.stepped ? q.steps : 1); s++) {
        for (uint32_t L = 1; L <= P.levels; L++)
            for (uint64_t row0 = 0; row0 < P.level_rows(L, instances); row0 += SGFHE_CIRCUIT_CALL_ROWS, count++) {
                const CircuitCall C = circuit_level_call(P, L, row0, instances);
                if (calls) calls->push_back({C.rows, direct && C.j1 > C.j0, C.lut});
            }
        if (q.stepped && q.emit && !q.emit[s]) continue;
        for (size_t q0 = 0; !lift && q0 < sz.n_ct; q0 += sz.cpc) {
            const size_t nb = circuit_pack_runs(P, q.count, q0, std::min(sz.cpc, sz.n_ct - q0), !direct, nullptr) * n;
            if (!nb) continue;
            if (calls) calls->push_back({(uint32_t)nb, true, false});
            count++;
        }
    }
    return count;
}

// What the checks read of a ctx
struct CircuitEnv {
    size_t n = 0, M = 0;
    bool have_key = false;
    bool pack_exact = false;    // the exactness bound of pack_encrypted_bits holds for the ctx's primes
    uint32_t split_tiles = 0;   // workgroups of the split kernel per ciphertext
};

struct CircuitVerdict {
    enum What { REFUSED, EMPTY, RUN } what;   // EMPTY: SGFHE_OK, and the device is not touched
    int32_t code;                             // REFUSED: the error code, with `message`
    std::string message;
    size_t instances;                         // RUN: count, or -- ct -- count * n
};

// The only judge of a run's arguments: one ordered pass for every entry (DESIGN.md section 11 lists it), so which of
// two defects is reported does not depend on the entry.  Reads the plan and the request's own words, never the memory
// behind its pointers; allocates only for the message of a refusal.
inline CircuitVerdict circuit_request_check(const CircuitPlan *P, const CircuitRequest &q, const CircuitEnv &env) {
    const char *form = q.ct ? (q.stepped ? "sgfhe_circuit_run_steps_ct" : "sgfhe_circuit_run_ct")
                            : (q.stepped ? "sgfhe_circuit_run_steps" : "sgfhe_circuit_run");
    const auto refused = [](const char *entry, const std::string &what, int32_t code = SGFHE_ERR_INVALID_ARG) {
        return CircuitVerdict{CircuitVerdict::REFUSED, code, *entry ? std::string(entry) + ": " + what : what, 0};
    };
    const char *hook = "sgfhe_debug_circuit_script";
    if (q.script && (q.probe || q.device)) return refused(hook, "the host forms only: no probe, no device form");
    // (bit 1 without bit 0 was an unknown bit before SGFHE_CIRCUIT_PACK_LIFT existed, and stays refused)
    if (q.ct && ((q.flags & ~(SGFHE_CIRCUIT_PACK_DIRECT | SGFHE_CIRCUIT_PACK_LIFT)) || q.flags == SGFHE_CIRCUIT_PACK_LIFT))
        return refused(q.stepped ? form : "sgfhe_circuit_run_ct_ex", "unknown flag bits (PACK_LIFT goes with PACK_DIRECT)");
    const uint32_t fed = P ? (q.stepped ? P->n_stream() : P->n_inputs) : 0;   // the input wires the caller brings
    const bool no_in = fed && (q.ct ? !q.in_a || !q.in_b : !q.in);
    const bool no_out = !q.ct && !q.out && !q.state_out;                       // (the ct forms: with out_w, below)
    if (!P || no_in || no_out || !q.state_a != !q.state_b)
        return refused(form, q.ct ? (q.stepped ? "NULL circuit or input pointer (state_a and state_b go together)"
                                               : "NULL circuit or input pointer")
                                  : (q.stepped ? "NULL circuit or input pointer, or no output pointer"
                                               : "NULL circuit, input or output pointer"));
    if (q.script && (!q.script->results || !q.script->staged || !q.script->lut))
        return refused(hook, "NULL script: the calls' results, the staged log and the descriptor log are needed");
    if (q.script && P->siblings())   // k_final_lut_multi writes the wires of a sibling inside the call
        return refused(hook, "a plan with a live LUT sibling: its wires are written inside the bootstrap call, from the "
                             "accumulator, which scripted result rows cannot stand in for");
    if (!q.stepped && P->n_regs)
        return refused("sgfhe_circuit_run", "a plan with registers runs through the _steps entries");
    for (uint32_t i = 0; q.stepped && q.ct && i < P->n_regs; i++)   // a split ciphertext is scale 0, and an LWE cannot be halved
        if (P->reg_scale[i]) return refused(form, "a register of scale 1 or 2 has no ciphertext form");
    if (P->n_planes && !q.with_data)
        return refused("sgfhe_circuit_run", "a plan with data planes runs through the _data entries");
    if (P->n_planes && !q.data && q.count && q.steps)
        return refused(q.stepped ? form : "sgfhe_circuit_run_data", "NULL data for a plan with data planes");
    if (q.probe && P->masked())   // (the probe's rows are rank * instances + instance)
        return refused("sgfhe_circuit_run_probe", "a plan with lane masks has no probe", SGFHE_ERR_UNSUPPORTED);
    if (q.probe && (!q.sk || !q.stats || (!q.in_bits && P->n_inputs)))
        return refused("sgfhe_circuit_run_probe", "NULL secret key, input bits or statistics pointer");
    if (q.ct && (!q.out_w != !q.out_v || (!q.packs() && !q.out && !q.state_out)))
        return refused(form, "out_w and out_v go together, and one output form is needed");
    if (q.ct && q.N != env.n && q.N != env.M) return refused(form, "N must be n (PackedCiphertext) or m (Ciphertext)");
    if (!env.have_key && !q.script) return refused("", "no bootstrap key uploaded", SGFHE_ERR_NO_KEY);   // (no call: no key)
    if (q.packs() && !env.pack_exact)
        return refused("pack_encrypted_bits", "exactness bound of the RNS primes", SGFHE_ERR_UNSUPPORTED);
    if (q.count == 0 || q.steps == 0) return {CircuitVerdict::EMPTY, SGFHE_OK, {}, 0};
    // rows of a level, and words of every table, must be addressable by the kernels' indices; in the ct forms the rows
    // of the pack stage (n_outputs * instances) and the workgroups of the split kernel too
    const uint64_t instances = q.ct ? (uint64_t)q.count * env.n : q.count;
    if (q.count >= 0x80000000u || instances >= 0x80000000u || (uint64_t)P->widest * instances > 0xFFFFFFFFull ||
        (q.ct && ((q.packs() && (uint64_t)P->n_outputs * instances > 0xFFFFFFFFull) ||
                  (uint64_t)P->n_inputs * q.count * env.split_tiles > 0x7FFFFFFFull)))
        return refused(form, "too many instances for this circuit");
    if ((q.ct ? env.n : instances) % P->group)   // (ct: a group must not straddle two ciphertexts)
        return refused(form, std::string(q.ct ? "n" : "instances") + " must be a multiple of the circuit's lane group");
    return {CircuitVerdict::RUN, SGFHE_OK, {}, (size_t)instances};
}

}  // namespace sgfhe

// The opaque handle of the C ABI: a plan is host data, independent of any ctx.
struct sgfhe_circuit {
    sgfhe::CircuitPlan plan;
};
