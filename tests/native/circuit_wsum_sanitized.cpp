// Weighted-sum nodes of csrc/circuit.h (sgfhe_circuit_create_w) under AddressSanitizer and UndefinedBehaviorSanitizer
// on the CPU (tests/test_circuit_wsum_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form that mix classic nodes and sum nodes of fan-in 1, 2, 3, 64 and anything between,
//     weights -2, -1, 1, 2, with NOTs, constants and (for G > 1) lane shifts on every term, are planned for
//     (group, instances) = (1, 5), (8, 72) and (64, 192), and circuit_plain_bits is compared, bit by bit, with an
//     evaluation of the ORIGINAL arrays one instance at a time -- HI, MID, LOW from s = the sum of w x mod 4;
//   - the plan's node table is compared with the arrays, term by term, its kinds with the node kinds, and its image
//     checked (tests/native/circuit_tables.h); a plan whose sum nodes all have two or three unit weights equals the
//     sgfhe_circuit_create3 plan -- whose two-term sum nodes carry one more term, the constant FALSE -- and gives the
//     same circuit_plain_bits word for word;
//   - an output that names a LOW wire is never direct, one that names HI or MID unshifted is;
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

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t below) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % below);
}

struct Arrays {
    uint32_t n_inputs;
    std::vector<uint32_t> kind, start, refs, outs;
    std::vector<int32_t> shift, weight, oshift;
    size_t gates() const { return kind.size(); }
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

// unit_only: every sum node has two or three terms of weight 1 (what sgfhe_circuit_create3 can say)
static Arrays random_circuit(uint32_t n_inputs, uint32_t n_gates, uint32_t n_outputs, uint32_t G, bool unit_only) {
    static const int32_t W[4] = {-2, -1, 1, 2};
    Arrays A;
    A.n_inputs = n_inputs;
    auto ref = [&](uint32_t wires) {
        const uint32_t id = rnd(10) == 0 ? CIRC_FALSE : rnd(wires);
        return id | (rnd(2) ? CIRC_NOT : 0u);
    };
    A.start.push_back(0);
    for (uint32_t g = 0; g < n_gates; g++) {
        const uint32_t pick = rnd(8);
        const bool classic = pick < 2;
        uint32_t fan = 2;
        if (!classic) {
            if (unit_only) fan = 2 + rnd(2);
            else fan = pick == 2 ? 1 : pick == 3 ? 2 : pick == 4 ? 3 : pick == 5 ? SGFHE_CIRCUIT_MAX_TERMS : 1 + rnd(12);
        }
        A.kind.push_back(classic ? 0u : 1u);
        for (uint32_t j = 0; j < fan; j++) {
            A.refs.push_back(ref(n_inputs + 3 * g));
            A.shift.push_back(random_shift(G));
            A.weight.push_back(classic || unit_only || (fan <= 3 && rnd(3) == 0) ? 1 : W[rnd(4)]);
        }
        A.start.push_back((uint32_t)A.refs.size());
    }
    for (uint32_t o = 0; o < n_outputs; o++) {
        A.outs.push_back(ref(n_inputs + 3 * n_gates));
        A.oshift.push_back(rnd(2) ? 0 : random_shift(G));
    }
    return A;
}

static int32_t plan_w(const Arrays &A, uint32_t G, CircuitPlan &P) {
    return circuit_plan(spec_csr(1, A.n_inputs, 0, A.kind.data(), A.start.data(), A.refs.data(), A.shift.data(),
                                 A.weight.data(), nullptr, A.gates(), A.outs.data(), A.oshift.data(), A.outs.size(), G), P);
}

// the model of include/sgfhe_hip.h, one instance at a time
static int lane_read(const std::vector<uint8_t> &wire, uint32_t ref, int32_t d, size_t t, uint32_t G) {
    int v = 0;
    const int64_t lane = (int64_t)(t % G) + d;
    if ((ref & ~CIRC_NOT) != CIRC_FALSE && lane >= 0 && lane < (int64_t)G) v = wire[(size_t)((int64_t)t + d)];
    return ref & CIRC_NOT ? !v : v;
}

static size_t check_case(uint32_t G, size_t instances, uint32_t n_inputs, uint32_t n_gates, uint32_t n_outputs) {
    const Arrays A = random_circuit(n_inputs, n_gates, n_outputs, G, false);
    CircuitPlan P;
    CHECK(plan_w(A, G, P) == SGFHE_OK);
    CHECK(P.group == G);
    check_plan_tables(P);
    uint32_t sums = 0;
    for (size_t k = 0; k < P.live(); k++) {   // every live node's terms in order
        const size_t g = P.order[k], i = A.start[g];
        sums += A.kind[g];
        check_node_terms(P, k, A.kind[g], A.start[g + 1] - i, &A.refs[i], &A.shift[i], &A.weight[i]);
    }
    CHECK(P.sum_before[P.live()] == sums);
    for (size_t o = 0; o < n_outputs; o++) {
        const uint32_t id = A.outs[o] & ~CIRC_NOT;
        if (id == CIRC_FALSE || id < n_inputs || P.out_shift[o]) {
            CHECK(P.out_node[o] == CIRC_NONE);
            continue;
        }
        const uint32_t g = (id - n_inputs) / 3, w = (id - n_inputs) % 3;
        const bool low = w == 2 && A.kind[g] != 0;
        CHECK((P.out_node[o] == CIRC_NONE) == low);                  // LOW is refreshed, every other gate wire direct
        if (!low) CHECK(P.order[P.out_node[o]] == g && P.out_gate[o] == w);
    }

    std::vector<uint8_t> bits((size_t)n_inputs * instances);
    for (auto &b : bits) b = (uint8_t)rnd(2);
    std::vector<std::vector<uint8_t>> wire((size_t)n_inputs + 3 * n_gates, std::vector<uint8_t>(instances));
    for (uint32_t i = 0; i < n_inputs; i++)
        for (size_t t = 0; t < instances; t++) wire[i][t] = bits[i * instances + t];
    static const std::vector<uint8_t> none;
    for (uint32_t g = 0; g < n_gates; g++)
        for (size_t t = 0; t < instances; t++) {
            int s = 0, v[2] = {0, 0};
            for (uint32_t i = A.start[g]; i < A.start[g + 1]; i++) {
                const uint32_t ref = A.refs[i], id = ref & ~CIRC_NOT;
                const int x = lane_read(id == CIRC_FALSE ? none : wire[id], ref, A.shift[i], t, G);
                if (i - A.start[g] < 2) v[i - A.start[g]] = x;
                s += A.weight[i] * x;
            }
            s = ((s % 4) + 4) % 4;
            uint8_t *w0 = &wire[n_inputs + 3 * g][t], *w1 = &wire[n_inputs + 3 * g + 1][t], *w2 = &wire[n_inputs + 3 * g + 2][t];
            if (A.kind[g]) {   // the rows the bootstrap reads at the phase s Dr
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

// sum nodes of two or three unit weights only: the plan of the [n_gates][3] arrays, table by table -- but for the third
// term (FALSE, shift 0, weight 1) those arrays give a sum node of two terms -- and the same plaintext bits
static void check_unit_is_create3(uint32_t G) {
    const uint32_t n_inputs = 3, n_gates = 14, n_outputs = 5;
    const Arrays A = random_circuit(n_inputs, n_gates, n_outputs, G, true);
    std::vector<uint32_t> g3;
    std::vector<int32_t> s3;
    for (uint32_t g = 0; g < n_gates; g++)
        for (uint32_t j = 0; j < 3; j++) {
            const bool have = j < A.start[g + 1] - A.start[g];
            g3.push_back(have ? A.refs[A.start[g] + j] : A.kind[g] ? CIRC_FALSE : CIRC_NO_INPUT);
            s3.push_back(have ? A.shift[A.start[g] + j] : 0);
        }
    CircuitPlan P, Z;
    CHECK(plan_w(A, G, P) == SGFHE_OK);
    CHECK(circuit_plan(spec_arity(3, n_inputs, g3.data(), s3.data(), n_gates, A.outs.data(), A.oshift.data(), n_outputs, G),
                       Z) == SGFHE_OK);
    check_plan_tables(P);
    check_plan_tables(Z);
    CHECK(P.levels == Z.levels && P.widest == Z.widest && P.slots == Z.slots && P.group == Z.group);
    CHECK(P.level == Z.level && P.order == Z.order && P.level_start == Z.level_start && P.input_slot == Z.input_slot);
    CHECK(P.node_kind == Z.node_kind && P.sum_before == Z.sum_before && P.out_slot == Z.out_slot && P.out_ref == Z.out_ref);
    CHECK(P.out_shift == Z.out_shift && P.out_node == Z.out_node && P.out_gate == Z.out_gate);
    CHECK(P.jobs == Z.jobs && P.job_k == Z.job_k);
    size_t padded = 0;
    for (size_t k = 0; k < P.node_kind.size(); k++) {   // (the pseudo-level's nodes included)
        const uint32_t p0 = P.term_start[k], np = P.term_start[k + 1] - p0, z0 = Z.term_start[k], nz = Z.term_start[k + 1] - z0;
        CHECK(nz == np || (nz == np + 1 && np == 2 && P.node_kind[k] == 1));
        for (uint32_t j = 0; j < np; j++) {
            CHECK(P.term_ref[p0 + j] == Z.term_ref[z0 + j] && P.term_shift[p0 + j] == Z.term_shift[z0 + j]);
            CHECK(P.term_weight[p0 + j] == Z.term_weight[z0 + j]);
            if (k < P.live()) CHECK(P.term_row[p0 + j] == Z.term_row[z0 + j]);
        }
        if (nz == np) continue;
        padded++;
        CHECK(Z.term_ref[z0 + 2] == CIRC_FALSE && Z.term_shift[z0 + 2] == 0 && Z.term_weight[z0 + 2] == 1);
        CHECK(Z.term_row[z0 + 2] == CIRC_FALSE);
    }
    CHECK(Z.term_ref.size() == P.term_ref.size() + padded);
    const size_t instances = 3 * (size_t)(G > 1 ? G * 9 : 70);   // (ragged last word)
    std::vector<uint8_t> bits((size_t)n_inputs * instances);
    for (auto &b : bits) b = (uint8_t)rnd(2);
    std::vector<uint64_t> tp, tz;
    CHECK(circuit_plain_bits(P, bits.data(), instances, tp) == SGFHE_OK);
    CHECK(circuit_plain_bits(Z, bits.data(), instances, tz) == SGFHE_OK && tp == tz && !tp.empty());
}

static void check_rejected() {
    // 2 inputs; node 0 classic (0, 1), node 1 a sum node 2 * AND(0) + 1 * in0 - 1 * ~XOR(0): wires 2..4 and 5..7
    const uint32_t kind[2] = {0, 1}, start[3] = {0, 2, 5}, refs[5] = {0, 1, 2, 0, 4 | CIRC_NOT}, outs[2] = {5, 7};
    const int32_t weight[5] = {1, 1, 2, 1, -1};
    CircuitPlan P;
    P.n_inputs = 77;   // (stays: a refused call does not touch the plan)
    auto refused = [&](const uint32_t *k, const uint32_t *s, const uint32_t *r, const int32_t *sh, const int32_t *w,
                       const uint32_t *o, uint32_t group) {
        const size_t before = g_allocs;
        const int32_t rc = circuit_plan(spec_csr(1, 2, 0, k, s, r, sh, w, nullptr, 2, o, nullptr, 2, group), P);
        CHECK(rc == SGFHE_ERR_INVALID_ARG && g_allocs == before && P.n_inputs == 77 && P.order.empty());
    };
    for (int32_t bad : {0, 3, -3, INT32_MIN, INT32_MAX}) {   // weights
        int32_t w[5] = {1, 1, 2, 1, -1};
        w[3] = bad;
        refused(kind, start, refs, nullptr, w, outs, 8);
    }
    const int32_t w_classic2[5] = {1, 2, 2, 1, -1}, w_classic_neg[5] = {-1, 1, 2, 1, -1};
    refused(kind, start, refs, nullptr, w_classic2, outs, 8);       // a classic node with a weight of 2 / -1
    refused(kind, start, refs, nullptr, w_classic_neg, outs, 8);
    const uint32_t s_first[3] = {1, 2, 5}, s_down[3] = {0, 5, 2}, s_empty[3] = {0, 2, 2}, s_classic3[3] = {0, 3, 5};
    refused(kind, s_first, refs, nullptr, weight, outs, 8);         // node_start[0] != 0
    refused(kind, s_down, refs, nullptr, weight, outs, 8);          // decreasing
    refused(kind, s_empty, refs, nullptr, weight, outs, 8);         // a sum node without a term
    refused(kind, s_classic3, refs, nullptr, weight, outs, 8);      // a classic node with three terms
    const uint32_t k_bad[2] = {0, 2};
    refused(k_bad, start, refs, nullptr, weight, outs, 8);          // node_kind above 1
    const uint32_t none[5] = {0, 1, 2, CIRC_NO_INPUT, 4}, none_not[5] = {0, 1, 2, CIRC_NO_INPUT | CIRC_NOT, 4};
    const uint32_t own[5] = {0, 1, 2, 0, 5}, later[5] = {0, 6, 2, 0, 4}, range[5] = {0, 1, 2, 0, 8};
    for (const uint32_t *r : {none, none_not, own, later, range}) refused(kind, start, r, nullptr, weight, outs, 8);
    const uint32_t out_none[2] = {5, CIRC_NO_INPUT};
    refused(kind, start, refs, nullptr, weight, out_none, 8);
    for (int32_t d : {8, -8, INT32_MIN, INT32_MAX}) {               // |d| >= G on a term
        const int32_t sh[5] = {0, 0, 0, 0, d};
        refused(kind, start, refs, sh, weight, outs, 8);
    }
    const int32_t one[5] = {0, 0, 1, 0, 0};                          // group = 1 admits no shift but 0
    refused(kind, start, refs, one, weight, outs, 1);
    refused(kind, start, refs, nullptr, weight, outs, 0);
    refused(nullptr, start, refs, nullptr, weight, outs, 8);
    refused(kind, nullptr, refs, nullptr, weight, outs, 8);
    refused(kind, start, nullptr, nullptr, weight, outs, 8);
    refused(kind, start, refs, nullptr, nullptr, outs, 8);
    {   // 65 terms
        std::vector<uint32_t> r65(2 + 65, 0u);
        std::vector<int32_t> w65(2 + 65, 1);
        r65[1] = 1;
        const uint32_t s65[3] = {0, 2, 67};
        refused(kind, s65, r65.data(), nullptr, w65.data(), outs, 8);
        // accepted: 64 terms, the largest shifts, a shift on a constant term (dropped)
        const uint32_t s64[3] = {0, 2, 66};
        std::vector<int32_t> sh64(66, 0);
        sh64[2] = 7, sh64[3] = -7;
        r65[4] = CIRC_FALSE | CIRC_NOT, sh64[4] = 5;
        for (size_t i = 2; i < 66; i++) w65[i] = (i & 1) ? -2 : 2;
        CHECK(circuit_plan(spec_csr(1, 2, 0, kind, s64, r65.data(), sh64.data(), w65.data(), nullptr, 2, outs, nullptr, 2, 8),
                           P) == SGFHE_OK);
        CHECK(P.node_kind[0] == 1 && P.n_inputs == 2 && P.live() == 1 && P.term_row.size() == 64);   // (node 0 is pruned)
        CHECK(P.term_shift[0] == 7 && P.term_shift[1] == -7 && P.term_shift[2] == 0 && P.out_node[0] == 0 && P.out_node[1] == CIRC_NONE);
        for (size_t i = 0; i < 64; i++) CHECK(P.term_weight[i] == w65[2 + i]);
        check_plan_tables(P);
    }
    CHECK(circuit_plan(spec_csr(1, 2, 0, kind, start, refs, nullptr, weight, nullptr, 2, outs, nullptr, 2, 1), P) == SGFHE_OK);
    CHECK(P.sum_before[2] == 1 && P.levels == 2 && P.live() == 2 && P.term_start[2] == 5 && P.term_row.size() == 5);
}

int main() {
    size_t compared = 0;
    for (int round = 0; round < 12; round++) {
        compared += check_case(1, 5, 3, 12, 6);
        compared += check_case(8, 72, 3, 14, 6);
        compared += check_case(64, 192, 4, 10, 5);
    }
    check_unit_is_create3(1);
    check_unit_is_create3(8);
    check_rejected();
    printf("ok %zu\n", compared);
    return 0;
}
