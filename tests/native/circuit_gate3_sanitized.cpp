// Three-input nodes of csrc/circuit.h (sgfhe_circuit_create3) under AddressSanitizer and UndefinedBehaviorSanitizer
// on the CPU (tests/test_circuit_gate3_host.py).  A stand-alone program, no input:
//   - random circuits that mix two- and three-input nodes, with NOTs, constants and (for G = 8) lane shifts on all
//     three inputs, are planned for (group, instances) = (1, 5) and (8, 72), and circuit_plain_bits is compared, bit
//     by bit, with an evaluation of the ORIGINAL arrays one instance at a time -- MAJ, ONE_OR_TWO, XOR3 from the count
//     of true inputs; the plan's node table is compared with the arrays, term by term -- a node with a third
//     reference is a sum node of three unit weights -- and its image checked (tests/native/circuit_tables.h);
//   - an output that names an XOR3 wire is never direct, one that names MAJ or ONE_OR_TWO unshifted is;
//   - the plan whose third references are all SGFHE_CIRCUIT_NONE equals the plan of the [n_gates][2] arrays;
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
    std::vector<uint32_t> gates, outs;     // gates [n_gates][3]
    std::vector<int32_t> gshift, oshift;   // gshift [n_gates][3]
};

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

// two nodes in three have a third input; the shift beside SGFHE_CIRCUIT_NONE is out of range on purpose (ignored)
static Arrays random_circuit(uint32_t n_inputs, uint32_t n_gates, uint32_t n_outputs, uint32_t G) {
    Arrays A;
    A.n_inputs = n_inputs;
    auto ref = [&](uint32_t wires) {
        const uint32_t id = rnd(10) == 0 ? CIRC_FALSE : rnd(wires);
        return id | (rnd(2) ? CIRC_NOT : 0u);
    };
    for (uint32_t g = 0; g < n_gates; g++)
        for (int j = 0; j < 3; j++) {
            if (j == 2 && rnd(3) == 0) {
                A.gates.push_back(CIRC_NO_INPUT);
                A.gshift.push_back(INT32_MIN);
                continue;
            }
            A.gates.push_back(ref(n_inputs + 3 * g));
            A.gshift.push_back(random_shift(G));
        }
    for (uint32_t o = 0; o < n_outputs; o++) {
        A.outs.push_back(ref(n_inputs + 3 * n_gates));
        A.oshift.push_back(rnd(2) ? 0 : random_shift(G));
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
    CHECK(circuit_plan(spec_arity(3, n_inputs, A.gates.data(), A.gshift.data(), n_gates, A.outs.data(), A.oshift.data(),
                                  n_outputs, G), P) == SGFHE_OK);
    CHECK(P.group == G);
    check_plan_tables(P);
    uint32_t three = 0;
    for (size_t k = 0; k < P.live(); k++) {   // the caller's kind: a third reference is present
        const size_t g = P.order[k];
        const bool sum = A.gates[3 * g + 2] != CIRC_NO_INPUT;
        three += sum;
        check_node_terms(P, k, sum, sum ? 3 : 2, &A.gates[3 * g], &A.gshift[3 * g], nullptr);
    }
    CHECK(P.sum_before[P.live()] == three);
    for (size_t o = 0; o < n_outputs; o++) {
        const uint32_t id = A.outs[o] & ~CIRC_NOT;
        if (id == CIRC_FALSE || id < n_inputs || P.out_shift[o]) {
            CHECK(P.out_node[o] == CIRC_NONE);
            continue;
        }
        const uint32_t g = (id - n_inputs) / 3, w = (id - n_inputs) % 3;
        const bool xor3 = w == 2 && A.gates[3 * g + 2] != CIRC_NO_INPUT;
        CHECK((P.out_node[o] == CIRC_NONE) == xor3);                 // XOR3 is refreshed, every other gate wire direct
        if (!xor3) CHECK(P.order[P.out_node[o]] == g && P.out_gate[o] == w);
    }

    std::vector<uint8_t> bits((size_t)n_inputs * instances);
    for (auto &b : bits) b = (uint8_t)rnd(2);
    std::vector<std::vector<uint8_t>> wire((size_t)n_inputs + 3 * n_gates, std::vector<uint8_t>(instances));
    for (uint32_t i = 0; i < n_inputs; i++)
        for (size_t t = 0; t < instances; t++) wire[i][t] = bits[i * instances + t];
    static const std::vector<uint8_t> none;
    for (uint32_t g = 0; g < n_gates; g++)
        for (size_t t = 0; t < instances; t++) {
            const int nj = A.gates[3 * g + 2] == CIRC_NO_INPUT ? 2 : 3;
            int s = 0, v[3] = {0, 0, 0};
            for (int j = 0; j < nj; j++) {
                const uint32_t ref = A.gates[3 * g + j], id = ref & ~CIRC_NOT;
                v[j] = lane_read(id == CIRC_FALSE ? none : wire[id], ref, A.gshift[3 * g + j], t, G);
                s += v[j];
            }
            uint8_t *w0 = &wire[n_inputs + 3 * g][t], *w1 = &wire[n_inputs + 3 * g + 1][t], *w2 = &wire[n_inputs + 3 * g + 2][t];
            if (nj == 3) {   // the rows the bootstrap reads at the phase s Dr
                *w0 = (uint8_t)(s >= 2);
                *w1 = (uint8_t)(s == 1 || s == 2);
                *w2 = (uint8_t)(s & 1);
            } else {
                *w0 = (uint8_t)(v[0] & v[1]);
                *w1 = (uint8_t)(v[0] | v[1]);
                *w2 = (uint8_t)(v[0] ^ v[1]);
            }
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
    if (G > 1) CHECK(circuit_plain_bits(P, bits.data(), instances - 1, table) == SGFHE_ERR_INVALID_ARG);
    return compared;
}

// every third reference SGFHE_CIRCUIT_NONE: the plan of the [n_gates][2] arrays, table by table
static void check_all_none(uint32_t G) {
    const uint32_t n_inputs = 3, n_gates = 14, n_outputs = 5;
    Arrays A = random_circuit(n_inputs, n_gates, n_outputs, G);
    std::vector<uint32_t> g2;
    std::vector<int32_t> s2;
    for (uint32_t g = 0; g < n_gates; g++) {
        A.gates[3 * g + 2] = CIRC_NO_INPUT;
        A.gshift[3 * g + 2] = (int32_t)(g % 2 ? 1000 : -1000);   // ignored
        for (int j = 0; j < 2; j++) {
            g2.push_back(A.gates[3 * g + j]);
            s2.push_back(A.gshift[3 * g + j]);
        }
    }
    CircuitPlan P, Z;
    CHECK(circuit_plan(spec_arity(3, n_inputs, A.gates.data(), A.gshift.data(), n_gates, A.outs.data(), A.oshift.data(),
                                  n_outputs, G), P) == SGFHE_OK);
    CHECK(circuit_plan(spec_arity(2, n_inputs, g2.data(), s2.data(), n_gates, A.outs.data(), A.oshift.data(), n_outputs, G),
                       Z) == SGFHE_OK);
    CHECK(P.sum_before[P.live()] == 0 && same_tables(P, Z));
}

static void check_rejected() {
    const uint32_t N = CIRC_NO_INPUT;
    const uint32_t outs[2] = {2, 5};
    CircuitPlan P;
    P.n_inputs = 77;   // (stays: a refused call does not touch the plan)
    auto refused = [&](const uint32_t *gates, const int32_t *gs, const uint32_t *o, uint32_t group) {
        const size_t before = g_allocs;
        const int32_t rc = circuit_plan(spec_arity(3, 2, gates, gs, 2, o, nullptr, 2, group), P);
        CHECK(rc == SGFHE_ERR_INVALID_ARG && g_allocs == before && P.n_inputs == 77 && P.order.empty());
    };
    const uint32_t none_x[6] = {N, 1, 0, 2, 0, N}, none_y[6] = {0, N, 1, 2, 0, N};      // NONE as a first / second input
    const uint32_t none_not[6] = {0, 1, N | CIRC_NOT, 2, 0, N};                         // NONE with NOT
    const uint32_t own[6] = {0, 1, 2, 2, 0, N}, later[6] = {0, 1, 6, 2, 0, N};         // third input: own / later node
    const uint32_t range[6] = {0, 1, 8, 2, 0, N};                                       // third input: no such wire
    const uint32_t good[6] = {0, 1, 0 | CIRC_NOT, 2, 0, 4};
    const uint32_t out_none[2] = {2, N}, out_none_not[2] = {N | CIRC_NOT, 5};
    for (const uint32_t *g : {none_x, none_y, none_not, own, later, range}) refused(g, nullptr, outs, 8);
    refused(good, nullptr, out_none, 8);
    refused(good, nullptr, out_none_not, 8);
    for (int32_t d : {8, -8, INT32_MIN, INT32_MAX}) {   // |d| >= G on the third input
        const int32_t gs[6] = {0, 0, d, 0, 0, 0};
        refused(good, gs, outs, 8);
    }
    const int32_t one[6] = {0, 0, 1, 0, 0, 0};           // group = 1 admits no shift but 0
    refused(good, one, outs, 1);
    refused(good, nullptr, outs, 0);
    // accepted: the largest shifts on a third input, anything beside NONE, a shift on a constant third input (dropped)
    const int32_t edge[6] = {0, 0, -7, 0, 0, 7};
    CHECK(circuit_plan(spec_arity(3, 2, good, edge, 2, outs, nullptr, 2, 8), P) == SGFHE_OK && P.sum_before[2] == 2 &&
          P.n_inputs == 2);
    CHECK(P.term_shift[2] == -7 && P.term_shift[5] == 7 && P.levels == 2);
    const uint32_t mixed[6] = {0, 1, N, 2, 0, CIRC_FALSE | CIRC_NOT};
    const int32_t wild[6] = {0, 0, INT32_MAX, 0, 0, 5};
    CHECK(circuit_plan(spec_arity(3, 2, mixed, wild, 2, outs, nullptr, 2, 8), P) == SGFHE_OK && P.sum_before[2] == 1);
    CHECK(P.node_kind[0] == 0 && P.node_kind[1] == 1 && P.term_start[1] == 2 && P.term_start[2] == 5);
    CHECK(P.term_ref[4] == (CIRC_FALSE | CIRC_NOT) && P.term_shift[4] == 0);
    // a third input alone keeps its node alive and sets the level
    const uint32_t chain[9] = {0, 1, N, 0, 1, N, 0, 0, 5 | CIRC_NOT}, last[1] = {2 + 3 * 2 + 2};
    CHECK(circuit_plan(spec_arity(3, 2, chain, nullptr, 3, last, nullptr, 1, 1), P) == SGFHE_OK);
    CHECK(P.live() == 2 && P.levels == 2 && P.level[0] == 0 && P.level[1] == 1 && P.level[2] == 2);
    CHECK(P.out_node[0] == CIRC_NONE);   // XOR3
}

int main() {
    size_t compared = 0;
    for (int round = 0; round < 16; round++) {
        compared += check_case(1, 5, 3, 12, 6);
        compared += check_case(8, 72, 3, 14, 6);
        compared += check_case(1, 72, 4, 10, 5);
        compared += check_case(8, 8, 2, 9, 4);
    }
    check_all_none(1);
    check_all_none(8);
    check_rejected();
    printf("ok %zu\n", compared);
    return 0;
}
