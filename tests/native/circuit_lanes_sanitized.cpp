// Lane plans of csrc/circuit.h (sgfhe_circuit_create_lanes) under AddressSanitizer and UndefinedBehaviorSanitizer
// on the CPU (tests/test_circuit_lanes_host.py).  A stand-alone program, no input:
//   - random circuits with random lane shifts and NOTs are planned for (group, instances) = (8, 72), (24, 120),
//     (64, 192) and (1, 5) -- groups that divide a 64-bit word, straddle words and fill one, rows whose last word is
//     ragged -- and circuit_plain_bits is compared, bit by bit, with an evaluation of the ORIGINAL arrays one
//     instance at a time; the plan's node table is compared with the arrays, term by term, and its image checked
//     (tests/native/circuit_tables.h);
//   - the zero-shift lanes plan equals the plan of the old entry;
//   - the inputs the planner must refuse return SGFHE_ERR_INVALID_ARG without a single allocation (the global
//     operator new is counted) and leave the plan they were given untouched.
// Prints "ok <bits compared>".
#include <stdio.h>
#include <stdlib.h>

#include <new>
#include <vector>

static size_t g_allocs = 0;
void *operator new(size_t n) {
    g_allocs++;
    if (void *p = malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void *operator new[](size_t n) { return operator new(n); }
void *operator new(size_t n, const std::nothrow_t &) noexcept {   // (std::stable_sort's buffer)
    g_allocs++;
    return malloc(n ? n : 1);
}
void *operator new[](size_t n, const std::nothrow_t &t) noexcept { return operator new(n, t); }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

#include "circuit.h"
#include "circuit_tables.h"

using namespace sgfhe;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #cond);    \
            abort();                                                              \
        }                                                                         \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % below);
}

struct Arrays {
    uint32_t n_inputs;
    std::vector<uint32_t> gates, outs;
    std::vector<int32_t> gshift, oshift;
};

// shifts from {0, +-1, +-(G - 1), anything inside the group}
static int32_t random_shift(uint32_t G) {
    if (G == 1) return 0;
    switch (rnd(6)) {
    case 0: return 0;
    case 1: return 1;
    case 2: return -1;
    case 3: return (int32_t)(G - 1);
    case 4: return -(int32_t)(G - 1);
    default: return (int32_t)rnd(2 * G - 1) - (int32_t)(G - 1);
    }
}

static Arrays random_circuit(uint32_t n_inputs, uint32_t n_gates, uint32_t n_outputs, uint32_t G) {
    Arrays A;
    A.n_inputs = n_inputs;
    auto ref = [&](uint32_t wires) {
        const uint32_t id = rnd(12) == 0 ? CIRC_FALSE : rnd(wires);
        return id | (rnd(2) ? CIRC_NOT : 0u);
    };
    for (uint32_t g = 0; g < n_gates; g++)
        for (int j = 0; j < 2; j++) {
            A.gates.push_back(ref(n_inputs + 3 * g));
            A.gshift.push_back(random_shift(G));
        }
    for (uint32_t o = 0; o < n_outputs; o++) {
        A.outs.push_back(ref(n_inputs + 3 * n_gates));
        A.oshift.push_back(random_shift(G));
    }
    return A;
}

// the model of include/sgfhe_hip.h, one instance at a time
static int lane_read(const std::vector<uint8_t> &wire, uint32_t ref, int32_t d, size_t t, uint32_t G) {
    int v = 0;
    const int64_t lane = (int64_t)(t % G) + d;
    if ((ref & ~CIRC_NOT) != CIRC_FALSE && lane >= 0 && lane < (int64_t)G) v = wire[(size_t)((int64_t)t + d)];
    return ref & CIRC_NOT ? !v : v;
}

static size_t check_case(uint32_t G, size_t instances, uint32_t n_inputs, uint32_t n_gates, uint32_t n_outputs) {
    const Arrays A = random_circuit(n_inputs, n_gates, n_outputs, G);
    CircuitPlan P;
    CHECK(circuit_plan(spec_arity(2, n_inputs, A.gates.data(), A.gshift.data(), n_gates, A.outs.data(), A.oshift.data(),
                                  n_outputs, G), P) == SGFHE_OK);
    CHECK(P.group == G && P.lanes() == (G > 1));
    check_plan_tables(P);
    for (size_t k = 0; k < P.live(); k++)
        check_node_terms(P, k, 0, 2, &A.gates[2 * (size_t)P.order[k]], &A.gshift[2 * (size_t)P.order[k]], nullptr);
    for (size_t o = 0; o < n_outputs; o++) {
        CHECK(P.out_shift[o] == ((A.outs[o] & ~CIRC_NOT) == CIRC_FALSE ? 0 : A.oshift[o]));
        if (P.out_shift[o]) CHECK(P.out_node[o] == CIRC_NONE);   // a shifted output is refreshed, never direct
    }
    // the same arrays without shifts: levels, order and slots do not depend on the shifts
    CircuitPlan Z;
    CHECK(circuit_plan(spec_gates(n_inputs, A.gates.data(), n_gates, A.outs.data(), n_outputs), Z) == SGFHE_OK);
    CHECK(Z.level == P.level && Z.order == P.order && Z.level_start == P.level_start && Z.slots == P.slots);
    CHECK(Z.node_kind == P.node_kind && Z.term_start == P.term_start && Z.term_ref == P.term_ref && Z.term_row == P.term_row);
    CHECK(Z.term_weight == P.term_weight && Z.out_slot == P.out_slot && Z.out_ref == P.out_ref);
    // and with every shift zero the lanes plan IS the plan of the old entry, table by table
    const std::vector<int32_t> gz(A.gshift.size(), 0), oz(A.oshift.size(), 0);
    CircuitPlan ZL;
    CHECK(circuit_plan(spec_arity(2, n_inputs, A.gates.data(), gz.data(), n_gates, A.outs.data(), oz.data(), n_outputs, G),
                       ZL) == SGFHE_OK);
    ZL.group = Z.group;   // (the group is the one thing the entries give differently)
    CHECK(same_tables(ZL, Z));

    std::vector<uint8_t> bits((size_t)n_inputs * instances);
    for (auto &b : bits) b = (uint8_t)rnd(2);
    std::vector<std::vector<uint8_t>> wire((size_t)n_inputs + 3 * n_gates, std::vector<uint8_t>(instances));
    for (uint32_t i = 0; i < n_inputs; i++)
        for (size_t t = 0; t < instances; t++) wire[i][t] = bits[i * instances + t];
    static const std::vector<uint8_t> none;
    for (uint32_t g = 0; g < n_gates; g++)
        for (size_t t = 0; t < instances; t++) {
            int v[2];
            for (int j = 0; j < 2; j++) {
                const uint32_t ref = A.gates[2 * g + j], id = ref & ~CIRC_NOT;
                v[j] = lane_read(id == CIRC_FALSE ? none : wire[id], ref, A.gshift[2 * g + j], t, G);
            }
            wire[n_inputs + 3 * g][t] = (uint8_t)(v[0] & v[1]);
            wire[n_inputs + 3 * g + 1][t] = (uint8_t)(v[0] | v[1]);
            wire[n_inputs + 3 * g + 2][t] = (uint8_t)(v[0] ^ v[1]);
        }
    std::vector<uint64_t> table;
    CHECK(circuit_plain_bits(P, bits.data(), instances, table) == SGFHE_OK);
    const size_t wpr = circuit_bit_words(instances);
    CHECK(table.size() == circuit_probe_rows(P) * wpr);
    size_t compared = 0;
    for (size_t row = 0; row < circuit_probe_rows(P); row++) {
        const uint32_t w = circuit_probe_wire(P, row);
        for (size_t t = 0; t < instances; t++, compared++)
            CHECK(((table[row * wpr + t / 64] >> (t % 64)) & 1) == wire[w][t]);
    }
    // instances that are no multiple of the group are refused
    if (G > 1) CHECK(circuit_plain_bits(P, bits.data(), instances - 1, table) == SGFHE_ERR_INVALID_ARG);
    return compared;
}

static void check_rejected() {
    const uint32_t gates[4] = {0, 1, 2, 0 | CIRC_NOT}, outs[2] = {2, 5};
    const int32_t zero[4] = {0, 0, 0, 0};
    CircuitPlan P;
    P.n_inputs = 77;   // (stays: a refused call does not touch the plan)
    auto refused = [&](const int32_t *gs, const int32_t *os, uint32_t group) {
        const size_t before = g_allocs;
        const int32_t rc = circuit_plan(spec_arity(2, 2, gates, gs, 2, outs, os, 2, group), P);
        CHECK(rc == SGFHE_ERR_INVALID_ARG && g_allocs == before && P.n_inputs == 77 && P.order.empty());
    };
    refused(nullptr, nullptr, 0);                          // group = 0
    refused(zero, zero, 0);
    for (int32_t d : {8, -8, 9, INT32_MIN, INT32_MAX}) {   // |d| >= G = 8, on a gate input and on an output
        const int32_t gs[4] = {0, 0, d, 0}, os[2] = {0, d};
        refused(gs, nullptr, 8);
        refused(nullptr, os, 8);
    }
    for (int32_t d : {1, -1}) {                            // group = 1 admits no shift but 0
        const int32_t gs[4] = {d, 0, 0, 0}, os[2] = {d, 0};
        refused(gs, nullptr, 1);
        refused(nullptr, os, 1);
    }
    const uint32_t later[4] = {0, 5, 2, 0};                // what sgfhe_circuit_create refuses is refused here too
    {
        const size_t before = g_allocs;
        CHECK(circuit_plan(spec_arity(2, 2, later, zero, 2, outs, zero, 2, 8), P) == SGFHE_ERR_INVALID_ARG && g_allocs == before);
        CHECK(circuit_plan(spec_arity(2, 2, gates, zero, 2, outs, zero, 0, 8), P) == SGFHE_ERR_INVALID_ARG && g_allocs == before);
    }
    // accepted: the largest shifts, NULL arrays, a shift on the constant (dropped)
    const int32_t edge[4] = {7, -7, 0, 0}, oedge[2] = {-7, 7};
    CHECK(circuit_plan(spec_arity(2, 2, gates, edge, 2, outs, oedge, 2, 8), P) == SGFHE_OK && P.group == 8 && P.n_inputs == 2);
    CHECK(P.term_shift[0] == 7 && P.term_shift[1] == -7 && P.out_shift[0] == -7 && P.out_shift[1] == 7);
    CHECK(circuit_plan(spec_arity(2, 2, gates, nullptr, 2, outs, nullptr, 2, 8), P) == SGFHE_OK && P.lanes());
    for (int32_t d : P.term_shift) CHECK(d == 0);
    const uint32_t cgates[2] = {CIRC_FALSE | CIRC_NOT, 0}, couts[1] = {CIRC_FALSE};
    const int32_t cs[2] = {3, 0}, cos_[1] = {-3};
    CHECK(circuit_plan(spec_arity(2, 1, cgates, cs, 1, couts, cos_, 1, 4), P) == SGFHE_OK);
    CHECK(P.out_shift[0] == 0 && P.live() == 0);
}

int main() {
    size_t compared = 0;
    for (int round = 0; round < 6; round++) {
        compared += check_case(8, 72, 3, 12, 5);
        compared += check_case(24, 120, 4, 14, 6);
        compared += check_case(64, 192, 3, 12, 5);
        compared += check_case(1, 5, 3, 10, 4);
    }
    check_rejected();
    printf("ok %zu\n", compared);
    return 0;
}
