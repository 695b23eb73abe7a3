// LUT nodes of csrc/circuit.h (sgfhe_circuit_create_lut) under AddressSanitizer and UndefinedBehaviorSanitizer on the
// CPU (tests/test_circuit_lut_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form that mix classic nodes, sum nodes and LUT nodes and obey the scale rule (position
//     i of a LUT node reads the constant or a wire of scale 2 - i, everything else scale 0), with NOTs, constants and
//     (for G > 1) lane shifts, are planned for (group, instances) = (1, 5), (4, 24) and (8, 72), and circuit_plain_bits
//     is compared, bit by bit, with an evaluation of the ORIGINAL arrays one instance at a time -- a LUT node's three
//     wires are bit x0 + 2 x1 + 4 x2 of its table;
//   - the plan's kind words carry kind and table, lut_before counts the LUT nodes, circuit_level_call flags the calls
//     that hold one, and an output naming wire +0 of a LUT node is never direct;
//   - a plan without LUT nodes equals the sgfhe_circuit_create_w plan of the same arrays, table by table and image word
//     by word;
//   - the inputs the planner must refuse -- every violation of the scale rule, a table of 256, a LUT node without
//     exactly three unit-weight terms, kind 3, a NULL node_table, kind 2 through sgfhe_circuit_create_w -- return
//     SGFHE_ERR_INVALID_ARG without a single allocation (the global operator new is counted) and leave the plan they
//     were given untouched.
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
void *operator new(size_t n, const std::nothrow_t &) noexcept {
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

static uint64_t g_state = 0x13198A2E03707344ull;
static uint32_t rnd(uint32_t below) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % below);
}

struct Arrays {
    uint32_t n_inputs = 0, group = 1;
    std::vector<uint32_t> kind, start, ref, table, outputs;
    std::vector<int32_t> shift, weight, out_shift;
    size_t n_gates() const { return kind.size(); }
    // through the entry that admits kinds 0 .. max_kind (1: sgfhe_circuit_create_w, which takes no node_table)
    int32_t plan_kinds(uint32_t max_kind, CircuitPlan &P) const {
        return circuit_plan(spec_csr(max_kind, n_inputs, 0, kind.data(), start.data(), ref.data(), shift.data(), weight.data(),
                                     max_kind >= 2 ? table.data() : nullptr, n_gates(), outputs.data(), out_shift.data(),
                                     outputs.size(), group), P);
    }
    int32_t plan(CircuitPlan &P) const { return plan_kinds(2, P); }
    int32_t plan_w(CircuitPlan &P) const { return plan_kinds(1, P); }
};

static int32_t a_shift(uint32_t group) { return group > 1 ? (int32_t)rnd(2 * group - 1) - (int32_t)(group - 1) : 0; }

// A random circuit that obeys the scale rule; `luts`: whether LUT nodes appear at all.
static Arrays random_circuit(uint32_t n_inputs, size_t n_gates, uint32_t group, bool luts) {
    Arrays A;
    A.n_inputs = n_inputs;
    A.group = group;
    std::vector<uint32_t> by_scale[3];
    for (uint32_t i = 0; i < n_inputs; i++) by_scale[0].push_back(i);
    auto pick = [&](uint32_t scale) -> uint32_t {
        uint32_t r = by_scale[scale].empty() || rnd(8) == 0 ? CIRC_FALSE : by_scale[scale][rnd((uint32_t)by_scale[scale].size())];
        return rnd(3) == 0 ? r | CIRC_NOT : r;
    };
    auto term = [&](uint32_t r, int32_t w) {
        A.ref.push_back(r);
        A.shift.push_back(a_shift(group));
        A.weight.push_back(w);
    };
    A.start.push_back(0);
    for (size_t g = 0; g < n_gates; g++) {
        const uint32_t k = luts ? rnd(3) : rnd(2);
        A.kind.push_back(k);
        A.table.push_back(k == 2 ? rnd(256) : 0x12345u);   // (read for LUT nodes only)
        if (k == 0) {
            term(pick(0), 1);
            term(pick(0), 1);
        } else if (k == 1) {
            static const int32_t ws[4] = {-2, -1, 1, 2};
            for (uint32_t j = 0, nj = 1 + rnd(5); j < nj; j++) term(pick(0), ws[rnd(4)]);
        } else {
            for (uint32_t p = 0; p < 3; p++) term(pick(2 - p), 1);
        }
        A.start.push_back((uint32_t)A.ref.size());
        const uint32_t base = n_inputs + 3 * (uint32_t)g;
        for (uint32_t w = 0; w < 3; w++) by_scale[k == 2 ? w : 0].push_back(base + w);
    }
    for (uint32_t o = 0, no = 1 + rnd(6); o < no; o++) {
        A.outputs.push_back(pick(0));
        A.out_shift.push_back(a_shift(group));
    }
    // the last node is always live: its wire +0 has scale 0 whatever its kind
    A.outputs.push_back(n_inputs + 3 * (uint32_t)(n_gates - 1));
    A.out_shift.push_back(0);
    return A;
}

// the ORIGINAL arrays, one instance at a time: every wire of every node, [wire][instance]
static std::vector<std::vector<uint8_t>> evaluate(const Arrays &A, const std::vector<uint8_t> &in_bits, size_t inst) {
    std::vector<std::vector<uint8_t>> val(A.n_inputs + 3 * A.n_gates(), std::vector<uint8_t>(inst, 0));
    for (uint32_t i = 0; i < A.n_inputs; i++)
        for (size_t t = 0; t < inst; t++) val[i][t] = in_bits[i * inst + t] & 1;
    auto read = [&](size_t i, size_t t) -> uint32_t {
        const uint32_t id = A.ref[i] & ~CIRC_NOT;
        uint32_t v = 0;
        if (id != CIRC_FALSE) {
            const int64_t lane = (int64_t)(t % A.group) + A.shift[i];
            if (lane >= 0 && lane < (int64_t)A.group) v = val[id][(size_t)((int64_t)t + A.shift[i])];
        }
        return A.ref[i] & CIRC_NOT ? v ^ 1u : v;
    };
    for (size_t g = 0; g < A.n_gates(); g++) {
        const size_t base = A.n_inputs + 3 * g, t0 = A.start[g], t1 = A.start[g + 1];
        for (size_t t = 0; t < inst; t++) {
            if (A.kind[g] == 0) {
                const uint32_t x = read(t0, t), y = read(t0 + 1, t);
                val[base][t] = x & y, val[base + 1][t] = x | y, val[base + 2][t] = x ^ y;
            } else if (A.kind[g] == 1) {
                int32_t s = 0;
                for (size_t i = t0; i < t1; i++) s += A.weight[i] * (int32_t)read(i, t);
                s = ((s % 4) + 4) % 4;
                val[base][t] = s >= 2, val[base + 1][t] = s == 1 || s == 2, val[base + 2][t] = s & 1;
            } else {
                const uint32_t s = read(t0, t) + 2 * read(t0 + 1, t) + 4 * read(t0 + 2, t);
                val[base][t] = val[base + 1][t] = val[base + 2][t] = (A.table[g] >> s) & 1;
            }
        }
    }
    return val;
}

static size_t compare_bits(const Arrays &A, const CircuitPlan &P, size_t inst) {
    std::vector<uint8_t> in_bits(A.n_inputs * inst);
    for (auto &b : in_bits) b = (uint8_t)(rnd(2) | (rnd(2) << 1));   // (only bit 0 counts)
    std::vector<uint64_t> table;
    CHECK(circuit_plain_bits(P, in_bits.data(), inst, table) == SGFHE_OK);
    const auto val = evaluate(A, in_bits, inst);
    const size_t wpr = circuit_bit_words(inst);
    size_t compared = 0;
    for (size_t row = 0; row < circuit_probe_rows(P); row++) {
        const uint32_t wire = circuit_probe_wire(P, row);
        for (size_t t = 0; t < inst; t++, compared++)
            CHECK(((table[row * wpr + t / 64] >> (t % 64)) & 1) == val[wire][t]);
    }
    return compared;
}

static void check_kinds(const Arrays &A, const CircuitPlan &P, size_t inst) {
    uint32_t luts = 0;
    for (size_t k = 0; k < P.live(); k++) {
        const size_t g = P.order[k];
        CHECK(P.kind(k) == A.kind[g]);
        CHECK(P.node_kind[k] == (A.kind[g] == 2 ? 2u | (A.table[g] << 8) : A.kind[g]));
        if (A.kind[g] == 2) CHECK(P.table(k) == A.table[g] && P.term_start[k + 1] - P.term_start[k] == 3);
        CHECK(P.lut_before[k] == luts);
        luts += A.kind[g] == 2;
        CHECK(P.lut_in((uint32_t)k, (uint32_t)k) == (A.kind[g] == 2) && P.gate3_in((uint32_t)k, (uint32_t)k) == (A.kind[g] == 1));
    }
    CHECK(P.lut_before[P.live()] == luts && P.lut_before.size() == P.live() + 1);
    for (size_t k = P.live(); k < P.node_kind.size(); k++) CHECK(P.node_kind[k] == 0);
    for (size_t o = 0; o < P.n_outputs; o++) {   // wire +0 of a LUT node is refreshed or lifted, never direct
        const uint32_t id = A.outputs[o] & ~CIRC_NOT;
        if (id != CIRC_FALSE && id >= A.n_inputs && A.kind[(id - A.n_inputs) / 3] == 2) CHECK(P.out_node[o] == CIRC_NONE);
    }
    for (uint32_t L = 1; L <= P.levels; L++)
        for (uint64_t row0 = 0; row0 < P.level_rows(L, inst); row0 += SGFHE_CIRCUIT_CALL_ROWS) {
            const CircuitCall C = circuit_level_call(P, L, row0, inst);
            bool lut = false, sum = false;
            for (uint32_t k = C.ka; k <= C.kb; k++) lut |= P.kind(k) == 2, sum |= P.kind(k) == 1;
            CHECK(C.lut == lut && C.sum == sum);
        }
}

static void refused(const Arrays &A, bool through_w = false) {
    CircuitPlan P;
    P.n_inputs = 77;   // (must survive)
    const size_t before = g_allocs;
    const int32_t rc = through_w ? A.plan_w(P) : A.plan(P);
    CHECK(rc == SGFHE_ERR_INVALID_ARG && g_allocs == before && P.n_inputs == 77 && P.order.empty());
}

int main() {
    size_t compared = 0;
    const uint32_t cfg[3][2] = {{1, 5}, {4, 24}, {8, 72}};
    for (const auto &gc : cfg)
        for (int rep = 0; rep < 40; rep++) {
            const Arrays A = random_circuit(1 + rnd(4), 1 + rnd(24), gc[0], true);
            CircuitPlan P;
            CHECK(A.plan(P) == SGFHE_OK);
            check_kinds(A, P, gc[1]);
            compared += compare_bits(A, P, gc[1]);
        }
    // without LUT nodes: the plan of sgfhe_circuit_create_w
    for (int rep = 0; rep < 20; rep++) {
        const Arrays A = random_circuit(1 + rnd(4), 1 + rnd(24), rep % 2 ? 4 : 1, false);
        CircuitPlan P, W;
        CHECK(A.plan(P) == SGFHE_OK && A.plan_w(W) == SGFHE_OK);
        CHECK(same_tables(P, W) && P.image == W.image && P.lut_before == W.lut_before && P.lut_before[P.live()] == 0);
        CHECK(P.levels == W.levels && P.slots == W.slots && P.widest == W.widest && P.order == W.order);
        check_plan_tables(P);
        compared += compare_bits(A, P, rep % 2 ? 24 : 5);
    }
    // ---- refused.  3 inputs; node 0 = fan(in 0): wires 3, 4, 5 at scales 0, 1, 2; node 1 = lut(5, 4, 3): wires 6, 7, 8
    Arrays G;
    G.n_inputs = 3;
    G.kind = {2, 2};
    G.start = {0, 3, 6};
    G.ref = {CIRC_FALSE, CIRC_FALSE, 0, 5, 4 | CIRC_NOT, 3};
    G.shift = {0, 0, 0, 0, 0, 0};
    G.weight = {1, 1, 1, 1, 1, 1};
    G.table = {0xF0, 0xCA};
    G.outputs = {6, 3 | CIRC_NOT};
    G.out_shift = {0, 0};
    {
        CircuitPlan P;
        CHECK(G.plan(P) == SGFHE_OK && P.levels == 2 && P.live() == 2 && P.lut_before[2] == 2);
        CHECK(P.out_node[0] == CIRC_NONE && P.out_node[1] == CIRC_NONE);
    }
    auto with = [&](auto &&edit) {
        Arrays B = G;
        edit(B);
        return B;
    };
    refused(with([](Arrays &B) { B.ref[3] = 4; }));               // position 0 reads scale 1
    refused(with([](Arrays &B) { B.ref[3] = 3; }));               // ... scale 0
    refused(with([](Arrays &B) { B.ref[3] = 1; }));               // ... an input
    refused(with([](Arrays &B) { B.ref[4] = 5; }));               // position 1 reads scale 2
    refused(with([](Arrays &B) { B.ref[4] = 3 | CIRC_NOT; }));    // ... scale 0
    refused(with([](Arrays &B) { B.ref[5] = 4; }));               // position 2 reads scale 1
    refused(with([](Arrays &B) { B.ref[5] = 5 | CIRC_NOT; }));    // ... scale 2
    refused(with([](Arrays &B) { B.ref[2] = 0; B.ref[0] = 1; })); // a fan reading an input at position 0
    refused(with([](Arrays &B) { B.outputs[0] = 7; }));           // an output of scale 1
    refused(with([](Arrays &B) { B.outputs[1] = 8 | CIRC_NOT; }));// ... of scale 2
    refused(with([](Arrays &B) { B.table[1] = 256; }));
    refused(with([](Arrays &B) { B.table[0] = 0xFFFFFFFFu; }));
    refused(with([](Arrays &B) { B.weight[4] = 2; }));
    refused(with([](Arrays &B) { B.weight[0] = -1; }));
    refused(with([](Arrays &B) { B.kind[1] = 3; }));
    refused(with([](Arrays &B) { B.start = {0, 2, 6}; }));        // LUT nodes of two and four terms
    refused(with([](Arrays &B) { B.start = {0, 3, 5}; B.ref.pop_back(); B.shift.pop_back(); B.weight.pop_back(); }));
    refused(G, true);                                             // kind 2 through sgfhe_circuit_create_w
    {   // a classic and a sum node reading scaled wires; NULL node_table
        Arrays B = G;
        B.kind.push_back(0);
        B.ref.push_back(6), B.ref.push_back(7);
        B.shift.push_back(0), B.shift.push_back(0);
        B.weight.push_back(1), B.weight.push_back(1);
        B.table.push_back(0);
        B.start.push_back(8);
        refused(B);
        B.ref[7] = 3;
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK);
        B.kind[2] = 1;
        B.ref[6] = 8;
        refused(B);
        CircuitPlan Q;
        Q.n_inputs = 77;
        const size_t before = g_allocs;
        CHECK(circuit_plan(spec_csr(2, G.n_inputs, 0, G.kind.data(), G.start.data(), G.ref.data(), G.shift.data(),
                                    G.weight.data(), nullptr, G.n_gates(), G.outputs.data(), G.out_shift.data(),
                                    G.outputs.size(), 1), Q) == SGFHE_ERR_INVALID_ARG && g_allocs == before && Q.n_inputs == 77);
    }
    printf("ok %zu\n", compared);
    return 0;
}
