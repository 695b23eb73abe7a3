// What every circuit_*_sanitized.cpp checks of the tables of a CircuitPlan (csrc/circuit.h), whichever entry the
// arrays came through:
//   - check_node_terms: live node k of `order` has the caller's kind and the caller's terms in order -- NOT bits,
//     constants, shifts (zeroed beside a constant), weights -- term_row names the probe row of every term's wire, and
//     gate3_in(k, k) agrees with node_kind[k];
//   - check_plan_tables: the shape of the node table, the pack stage's pseudo-level, the direct-pack job table against
//     the construction a run used to make for itself, and the image: its sections lie inside it, do not overlap and
//     hold what the vectors hold;
//   - same_tables: two plans are equal table by table.
#pragma once

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "circuit.h"

#define TCHECK(cond)                                                                                  \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "check failed at %s line %d: %s\n", __FILE__, __LINE__, #cond);           \
            abort();                                                                                  \
        }                                                                                             \
    } while (0)

// The CircuitSpec an entry of the C ABI fills from its arrays.  spec_gates: sgfhe_circuit_create; spec_arity: the
// [n_gates][arity] arrays of sgfhe_circuit_create_lanes (2) and sgfhe_circuit_create3 (3); spec_csr: the CSR arrays of
// the entry that admits kinds 0 .. max_kind -- 1 sgfhe_circuit_create_w (no node_table), 2 _lut, 3 _lut_multi, 5 _data
// (and its planes).  Registers and routes (_seq, _routed) are set by field: S.regs, S.routes.
inline sgfhe::CircuitSpec spec_arity(int arity, uint32_t n_inputs, const uint32_t *gates, const int32_t *gate_shift,
                                     size_t n_gates, const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs,
                                     uint32_t group) {
    sgfhe::CircuitSpec S;
    S.n_inputs = n_inputs, S.nodes = sgfhe::circuit_nodes_arity(arity, gates, gate_shift), S.n_gates = n_gates;
    S.outputs = outputs, S.out_shift = out_shift, S.n_outputs = n_outputs, S.group = group;
    return S;
}
inline sgfhe::CircuitSpec spec_gates(uint32_t n_inputs, const uint32_t *gates, size_t n_gates, const uint32_t *outputs,
                                     size_t n_outputs) {
    return spec_arity(2, n_inputs, gates, nullptr, n_gates, outputs, nullptr, n_outputs, 1u);
}
inline sgfhe::CircuitSpec spec_csr(uint32_t max_kind, uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind,
                                   const uint32_t *node_start, const uint32_t *term_ref, const int32_t *term_shift,
                                   const int32_t *term_weight, const uint32_t *node_table, size_t n_gates,
                                   const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group) {
    sgfhe::CircuitSpec S = spec_arity(0, n_inputs, nullptr, nullptr, n_gates, outputs, out_shift, n_outputs, group);
    S.nodes = sgfhe::circuit_nodes_csr(max_kind, node_kind, node_start, term_ref, term_shift, term_weight, node_table, n_planes);
    return S;
}

// `count` terms refs[0 ..] / shifts[0 ..] (NULL: all 0) / weights[0 ..] (NULL: all 1) of the caller's node order[k]
inline void check_node_terms(const sgfhe::CircuitPlan &P, size_t k, uint32_t kind, size_t count, const uint32_t *refs,
                             const int32_t *shifts, const int32_t *weights) {
    using namespace sgfhe;
    TCHECK(P.node_kind[k] == kind && P.gate3_in((uint32_t)k, (uint32_t)k) == (kind != 0));
    TCHECK(P.sum_before[k + 1] == P.sum_before[k] + kind);
    TCHECK(P.term_start[k + 1] - P.term_start[k] == count);
    for (size_t j = 0; j < count; j++) {
        const size_t q = P.term_start[k] + j;
        const uint32_t id = refs[j] & ~CIRC_NOT, sid = P.term_ref[q] & ~CIRC_NOT, rid = P.term_row[q] & ~CIRC_NOT;
        TCHECK((P.term_ref[q] & CIRC_NOT) == (refs[j] & CIRC_NOT) && (P.term_row[q] & CIRC_NOT) == (refs[j] & CIRC_NOT));
        TCHECK(P.term_weight[q] == (weights ? weights[j] : 1));
        if (id == CIRC_FALSE) {
            TCHECK(sid == CIRC_FALSE && rid == CIRC_FALSE && P.term_shift[q] == 0);
            continue;
        }
        TCHECK(sid < P.slots && P.term_shift[q] == (shifts ? shifts[j] : 0));
        TCHECK(rid < circuit_probe_rows(P) && circuit_probe_wire(P, rid) == id);
        if (rid >= P.n_inputs) TCHECK((rid - P.n_inputs) / 3 < k);   // an earlier node of `order`
    }
}

inline void check_plan_tables(const sgfhe::CircuitPlan &P) {
    using namespace sgfhe;
    const size_t live = P.live(), nodes = live + P.n_outputs, terms = P.term_row.size();
    // ---- the node table: the live nodes, then the pseudo-level of the pack stage, node live + o = (TRUE, output o)
    TCHECK(P.node_kind.size() == nodes && P.term_start.size() == nodes + 1 && P.term_start[0] == 0);
    TCHECK(P.term_start[live] == terms && P.term_start[nodes] == terms + 2 * (size_t)P.n_outputs);
    TCHECK(P.term_ref.size() == P.term_start[nodes] && P.term_shift.size() == P.term_ref.size() &&
           P.term_weight.size() == P.term_ref.size());
    TCHECK(P.sum_before.size() == live + 1 && P.sum_before[0] == 0 && P.out_slot.size() == 3 * live);
    for (size_t k = 0; k < live; k++) {
        const uint32_t n = P.term_start[k + 1] - P.term_start[k];
        TCHECK(P.node_kind[k] <= 1 && (P.node_kind[k] ? n >= 1 && n <= SGFHE_CIRCUIT_MAX_TERMS : n == 2));
    }
    TCHECK(P.out_ref.size() == P.n_outputs && P.out_shift.size() == P.n_outputs && P.out_node.size() == P.n_outputs &&
           P.out_gate.size() == P.n_outputs && P.input_slot.size() == P.n_inputs);
    for (size_t o = 0; o < P.n_outputs; o++) {
        const size_t q = P.term_start[live + o];
        TCHECK(P.node_kind[live + o] == 0 && P.term_start[live + o + 1] == q + 2);
        TCHECK(P.term_ref[q] == (CIRC_FALSE | CIRC_NOT) && P.term_shift[q] == 0 && P.term_weight[q] == 1);
        TCHECK(P.term_ref[q + 1] == P.out_ref[o] && P.term_shift[q + 1] == P.out_shift[o] && P.term_weight[q + 1] == 1);
    }
    // ---- the job table: the direct outputs by producing node, as a run built them before the planner did
    std::vector<uint32_t> jobs, job_k, byk;
    for (uint32_t o = 0; o < P.n_outputs; o++)
        if (P.out_node[o] != CIRC_NONE) byk.push_back(o);
    std::stable_sort(byk.begin(), byk.end(), [&](uint32_t x, uint32_t y) { return P.out_node[x] < P.out_node[y]; });
    for (uint32_t o : byk) {
        const uint32_t k = P.out_node[o], L = P.level[P.order[k]];
        job_k.push_back(k);
        jobs.insert(jobs.end(), {o, k - P.level_start[L], P.out_gate[o] | (P.out_ref[o] & CIRC_NOT)});
    }
    TCHECK(P.jobs == jobs && P.job_k == job_k);
    // ---- the image: every section inside it, none overlapping another, each holding its vector
    std::vector<std::pair<size_t, size_t>> spans;   // (offset, length)
    auto section = [&](uint32_t at, const auto &tab) {
        TCHECK((size_t)at + tab.size() <= P.image.size());
        for (size_t i = 0; i < tab.size(); i++) TCHECK(P.image[at + i] == (uint32_t)tab[i]);
        spans.push_back({at, tab.size()});
    };
    section(P.at.node_kind, P.node_kind);
    section(P.at.term_start, P.term_start);
    section(P.at.term_ref, P.term_ref);
    section(P.at.term_shift, P.term_shift);
    section(P.at.term_weight, P.term_weight);
    section(P.at.out_slot, P.out_slot);
    section(P.at.out_ref, P.out_ref);
    section(P.at.out_shift, P.out_shift);
    section(P.at.input_slot, P.input_slot);
    section(P.at.jobs, P.jobs);
    TCHECK(P.at.words == P.image.size());
    std::sort(spans.begin(), spans.end());
    size_t covered = 0;
    for (size_t i = 0; i < spans.size(); i++) {
        if (i) TCHECK(spans[i - 1].first + spans[i - 1].second <= spans[i].first);
        covered += spans[i].second;
    }
    TCHECK(covered == P.image.size());
}

// every table of two plans, and what numbers their rows
inline bool same_tables(const sgfhe::CircuitPlan &P, const sgfhe::CircuitPlan &Z) {
    return P.levels == Z.levels && P.widest == Z.widest && P.slots == Z.slots && P.group == Z.group &&
           P.level == Z.level && P.order == Z.order && P.level_start == Z.level_start && P.input_slot == Z.input_slot &&
           P.node_kind == Z.node_kind && P.term_start == Z.term_start && P.term_ref == Z.term_ref &&
           P.term_shift == Z.term_shift && P.term_weight == Z.term_weight && P.term_row == Z.term_row &&
           P.sum_before == Z.sum_before && P.out_slot == Z.out_slot && P.out_ref == Z.out_ref &&
           P.out_shift == Z.out_shift && P.out_node == Z.out_node && P.out_gate == Z.out_gate && P.jobs == Z.jobs &&
           P.job_k == Z.job_k && P.image == Z.image;
}
