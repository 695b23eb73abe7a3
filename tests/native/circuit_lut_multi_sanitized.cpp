// LUT families of csrc/circuit.h (sgfhe_circuit_create_lut_multi) under AddressSanitizer and UndefinedBehaviorSanitizer
// on the CPU (tests/test_circuit_lut_multi_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form that mix classic nodes, sum nodes, LUT nodes and their siblings (kind 3: no terms,
//     a table, behind a LUT node or a sibling) and obey the scale rule, with NOTs, constants and (for G > 1) lane
//     shifts, are planned for (group, instances) = (1, 5), (4, 24) and (8, 72), and circuit_plain_bits is compared, bit
//     by bit, with an evaluation of the ORIGINAL arrays one instance at a time -- a sibling's three wires are bit
//     x0 + 2 x1 + 4 x2 of ITS table at its LEADER's inputs; the probe rows of the live siblings follow those of the
//     nodes that take rows;
//   - the plan against a restatement of the model: which nodes are live (a leader through a live sibling too), that a
//     sibling has its leader's level and is in no level's ranks, the family CSR (the live siblings of every live node in
//     ascending index, their tables, a slot exactly for the wires something reads), the image sections, and the plan
//     against the one of the arrays with every sibling turned into a LUT node of its own (the same level of every
//     node that is live in both);
//   - the call arithmetic: the calls of every level cover its rows once, rows = ranks x instances with no rank for a
//     sibling, and circuit_level_call flags exactly the calls whose nodes lead a live sibling -- over 8192 rows too, with
//     the boundary inside a leader's rows;
//   - arrays without kind 3 give the plan of sgfhe_circuit_create_lut, table by table and image word by word;
//   - the inputs the planner must refuse -- terms on a sibling, a sibling first or behind a classic or a sum node, a
//     table of 256, a family of 257, a scale violation through a sibling's wire, kind 3 through
//     sgfhe_circuit_create_lut and sgfhe_circuit_create_w -- return SGFHE_ERR_INVALID_ARG without a single allocation
//     (the global operator new is counted) and leave the plan they were given untouched; a family of 256 is accepted.
// Prints "ok <bits compared>".
#include <stdio.h>
#include <stdlib.h>

#include <new>
#include <set>
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

static uint64_t g_state = 0x243F6A8885A308D3ull;
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
    int32_t plan(CircuitPlan &P) const { return plan_kinds(3, P); }
    int32_t plan_lut(CircuitPlan &P) const { return plan_kinds(2, P); }
    int32_t plan_w(CircuitPlan &P) const { return plan_kinds(1, P); }
    size_t leader(size_t g) const {
        while (kind[g] == 3) g--;
        return g;
    }
};

static int32_t a_shift(uint32_t group) { return group > 1 ? (int32_t)rnd(2 * group - 1) - (int32_t)(group - 1) : 0; }

// A random circuit that obeys the scale rule; `siblings`: whether kind 3 appears at all.
static Arrays random_circuit(uint32_t n_inputs, size_t n_nodes, uint32_t group, bool siblings) {
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
    auto node = [&](uint32_t k, uint32_t tb) {
        A.kind.push_back(k);
        A.table.push_back(tb);
    };
    auto close = [&](bool lut) {
        A.start.push_back((uint32_t)A.ref.size());
        const uint32_t base = n_inputs + 3 * (uint32_t)(A.n_gates() - 1);
        for (uint32_t w = 0; w < 3; w++) by_scale[lut ? w : 0].push_back(base + w);
    };
    A.start.push_back(0);
    for (size_t g = 0; g < n_nodes; g++) {
        const uint32_t k = rnd(3);
        node(k, k == 2 ? rnd(256) : 0x12345u);   // (read for LUT nodes and siblings only)
        if (k == 0) {
            term(pick(0), 1);
            term(pick(0), 1);
        } else if (k == 1) {
            static const int32_t ws[4] = {-2, -1, 1, 2};
            for (uint32_t j = 0, nj = 1 + rnd(5); j < nj; j++) term(pick(0), ws[rnd(4)]);
        } else {
            for (uint32_t p = 0; p < 3; p++) term(pick(2 - p), 1);
        }
        close(k == 2);
        for (uint32_t s = 0, ns = k == 2 && siblings ? rnd(5) : 0; s < ns; s++) {
            node(3, rnd(256));
            close(true);
        }
    }
    for (uint32_t o = 0, no = 1 + rnd(6); o < no; o++) {
        A.outputs.push_back(pick(0));
        A.out_shift.push_back(a_shift(group));
    }
    A.outputs.push_back(n_inputs + 3 * (uint32_t)(A.n_gates() - 1));   // the last node is always live
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
        const size_t base = A.n_inputs + 3 * g, l = A.leader(g), t0 = A.start[l], t1 = A.start[l + 1];
        for (size_t t = 0; t < inst; t++) {
            if (A.kind[g] == 0) {
                const uint32_t x = read(t0, t), y = read(t0 + 1, t);
                val[base][t] = x & y, val[base + 1][t] = x | y, val[base + 2][t] = x ^ y;
            } else if (A.kind[g] == 1) {
                int32_t s = 0;
                for (size_t i = t0; i < t1; i++) s += A.weight[i] * (int32_t)read(i, t);
                s = ((s % 4) + 4) % 4;
                val[base][t] = s >= 2, val[base + 1][t] = s == 1 || s == 2, val[base + 2][t] = s & 1;
            } else {   // a LUT node, or a sibling at its leader's terms
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
    CHECK(circuit_probe_rows(P) == A.n_inputs + 3 * (P.live() + P.siblings()) && table.size() == circuit_probe_rows(P) * wpr);
    size_t compared = 0;
    std::set<uint32_t> seen;
    for (size_t row = 0; row < circuit_probe_rows(P); row++) {
        const uint32_t wire = circuit_probe_wire(P, row);
        CHECK(seen.insert(wire).second);
        for (size_t t = 0; t < inst; t++, compared++)
            CHECK(((table[row * wpr + t / 64] >> (t % 64)) & 1) == val[wire][t]);
    }
    return compared;
}

// the model of include/sgfhe_hip.h, restated from the arrays
static void check_model(const Arrays &A, const CircuitPlan &P, size_t inst) {
    const size_t NG = A.n_gates();
    auto node_of = [&](uint32_t ref) -> int64_t {
        const uint32_t id = ref & ~CIRC_NOT;
        return id == CIRC_FALSE || id < A.n_inputs ? -1 : (int64_t)((id - A.n_inputs) / 3);
    };
    std::vector<uint8_t> live(NG, 0);
    for (uint32_t o : A.outputs)
        if (node_of(o) >= 0) live[node_of(o)] = 1;
    for (size_t g = NG; g-- > 0;) {
        if (!live[g]) continue;
        live[A.leader(g)] = 1;
        for (size_t i = A.start[g]; i < A.start[g + 1]; i++)
            if (node_of(A.ref[i]) >= 0) live[node_of(A.ref[i])] = 1;
    }
    // what reads a wire: the terms of live nodes, the outputs
    std::set<uint32_t> read;
    for (size_t g = 0; g < NG; g++)
        for (size_t i = A.start[g]; live[g] && i < A.start[g + 1]; i++) read.insert(A.ref[i] & ~CIRC_NOT);
    for (uint32_t o : A.outputs) read.insert(o & ~CIRC_NOT);
    size_t rows_taken = 0, sibs = 0;
    for (size_t g = 0; g < NG; g++) {
        CHECK((P.level[g] != 0) == (live[g] != 0));
        if (A.kind[g] == 3) CHECK(P.level[g] == (live[g] ? P.level[A.leader(g)] : 0u));
        rows_taken += live[g] && A.kind[g] != 3;
        sibs += live[g] && A.kind[g] == 3;
    }
    CHECK(P.live() == rows_taken && P.siblings() == sibs && P.fam_start.size() == P.live() + 1 && P.fam_start[0] == 0);
    CHECK(P.fam_entry.size() == 4 * sibs && P.fam_start[P.live()] == sibs);
    uint32_t widest = 0;
    for (uint32_t L = 1; L <= P.levels; L++) widest = std::max(widest, P.level_start[L + 1] - P.level_start[L]);
    CHECK(widest == P.widest);
    for (size_t k = 0; k < P.live(); k++) {
        const size_t g = P.order[k];
        CHECK(A.kind[g] != 3 && live[g]);
        CHECK(P.kind(k) == A.kind[g] && (A.kind[g] != 2 || P.table(k) == A.table[g]));
        if (k) CHECK(P.level[P.order[k - 1]] < P.level[g] || (P.level[P.order[k - 1]] == P.level[g] && P.order[k - 1] < g));
        size_t i = P.fam_start[k];
        for (size_t h = g + 1; h < NG && A.kind[h] == 3; h++) {
            if (!live[h]) continue;
            CHECK(i < P.fam_start[k + 1] && P.fam_node[i] == h && P.fam_entry[4 * i] == A.table[h]);
            bool any = false;
            for (uint32_t w = 0; w < 3; w++) {
                const uint32_t slot = P.fam_entry[4 * i + 1 + w];
                const bool is_read = read.count(A.n_inputs + 3 * (uint32_t)h + w) != 0;
                CHECK((slot != CIRC_NONE) == is_read && (slot == CIRC_NONE || slot < P.slots));
                any |= is_read;
                for (uint32_t w2 = 0; w2 < 3; w2++)   // no slot of the level shared with the leader's wires
                    CHECK(slot == CIRC_NONE || slot != P.out_slot[3 * k + w2]);
            }
            CHECK(any);
            i++;
        }
        CHECK(i == P.fam_start[k + 1]);
        CHECK(P.fam_in((uint32_t)k, (uint32_t)k) == (P.fam_start[k + 1] != P.fam_start[k]));
    }
    // an output naming a LUT or sibling wire is never direct
    for (size_t o = 0; o < P.n_outputs; o++)
        if (node_of(A.outputs[o]) >= 0 && A.kind[node_of(A.outputs[o])] >= 2) CHECK(P.out_node[o] == CIRC_NONE);
    // the image: the family sections behind the others, only with live siblings
    if (sibs) {
        CHECK(P.at.fam_start >= P.at.jobs + P.jobs.size() && P.at.fam_entry == P.at.fam_start + P.fam_start.size());
        CHECK(P.at.words == P.at.fam_entry + P.fam_entry.size() && P.image.size() == P.at.words);
        for (size_t i = 0; i < P.fam_start.size(); i++) CHECK(P.image[P.at.fam_start + i] == P.fam_start[i]);
        for (size_t i = 0; i < P.fam_entry.size(); i++) CHECK(P.image[P.at.fam_entry + i] == P.fam_entry[i]);
    } else {
        CHECK(P.at.fam_start == 0 && P.at.fam_entry == 0 && P.at.words == P.at.jobs + P.jobs.size());
    }
    // the calls: every level's rows once, ranks x instances, the family flag
    for (uint32_t L = 1; L <= P.levels; L++) {
        const uint64_t rows = P.level_rows(L, inst);
        CHECK(rows == (uint64_t)(P.level_start[L + 1] - P.level_start[L]) * inst);
        uint64_t covered = 0;
        for (uint64_t row0 = 0; row0 < rows; row0 += SGFHE_CIRCUIT_CALL_ROWS) {
            const CircuitCall C = circuit_level_call(P, L, row0, inst);
            CHECK(C.rows && C.rows <= SGFHE_CIRCUIT_CALL_ROWS && C.ka == P.level_start[L] + row0 / inst);
            CHECK(C.kb == P.level_start[L] + (row0 + C.rows - 1) / inst && C.kb < P.level_start[L + 1]);
            bool fam = false;
            for (uint32_t k = C.ka; k <= C.kb; k++) fam |= P.fam_start[k + 1] != P.fam_start[k];
            CHECK(C.fam == fam && (!fam || C.lut));
            covered += C.rows;
        }
        CHECK(covered == rows);
    }
    // every sibling as a LUT node of its own, at its leader's terms: the same level for every node live in both plans
    Arrays Z;
    Z.n_inputs = A.n_inputs, Z.group = A.group, Z.outputs = A.outputs, Z.out_shift = A.out_shift, Z.table = A.table;
    Z.start.push_back(0);
    for (size_t g = 0; g < NG; g++) {
        const size_t l = A.leader(g);
        Z.kind.push_back(A.kind[g] == 3 ? 2u : A.kind[g]);
        for (size_t i = A.start[l]; i < A.start[l + 1]; i++)
            Z.ref.push_back(A.ref[i]), Z.shift.push_back(A.shift[i]), Z.weight.push_back(A.weight[i]);
        Z.start.push_back((uint32_t)Z.ref.size());
    }
    CircuitPlan Q;
    CHECK(Z.plan_lut(Q) == SGFHE_OK && Q.levels == P.levels && Q.siblings() == 0);
    for (size_t g = 0; g < NG; g++) {
        if (Q.level[g]) CHECK(P.level[g] == Q.level[g]);
        else CHECK(!P.level[g] || (A.kind[g] == 2 && P.fam_in(0, (uint32_t)P.live() - 1)));   // a leader live through a sibling
    }
    CHECK(Q.live() == P.live() + P.siblings() - [&] {
        size_t extra = 0;
        for (size_t g = 0; g < NG; g++) extra += P.level[g] && !Q.level[g];
        return extra;
    }());
}

static void refused(const Arrays &A, int through = 0) {
    CircuitPlan P;
    P.n_inputs = 77;   // (must survive)
    const size_t before = g_allocs;
    const int32_t rc = through == 2 ? A.plan_w(P) : (through == 1 ? A.plan_lut(P) : A.plan(P));
    CHECK(rc == SGFHE_ERR_INVALID_ARG && g_allocs == before && P.n_inputs == 77 && P.order.empty());
}

int main() {
    size_t compared = 0;
    const uint32_t cfg[3][2] = {{1, 5}, {4, 24}, {8, 72}};
    size_t with_siblings = 0;
    for (const auto &gc : cfg)
        for (int rep = 0; rep < 40; rep++) {
            const Arrays A = random_circuit(1 + rnd(4), 1 + rnd(16), gc[0], true);
            CircuitPlan P;
            CHECK(A.plan(P) == SGFHE_OK);
            check_model(A, P, gc[1]);
            compared += compare_bits(A, P, gc[1]);
            with_siblings += P.siblings() != 0;
        }
    CHECK(with_siblings > 40);
    // without kind 3: the plan of sgfhe_circuit_create_lut
    for (int rep = 0; rep < 20; rep++) {
        const Arrays A = random_circuit(1 + rnd(4), 1 + rnd(24), rep % 2 ? 4 : 1, false);
        CircuitPlan P, W;
        CHECK(A.plan(P) == SGFHE_OK && A.plan_lut(W) == SGFHE_OK);
        CHECK(same_tables(P, W) && P.image == W.image && P.lut_before == W.lut_before && P.siblings() == 0);
        compared += compare_bits(A, P, rep % 2 ? 24 : 5);
    }
    // ---- 3 inputs; node 0 = fan(in 0): wires 3, 4, 5; node 1 = lut(5, 4, 3): wires 6, 7, 8; node 2 = its sibling: wires
    // 9, 10, 11; node 3 = lut(11, 10, 9) reads the sibling at every scale: wires 12, 13, 14
    Arrays G;
    G.n_inputs = 3;
    G.kind = {2, 2, 3, 2};
    G.start = {0, 3, 6, 6, 9};
    G.ref = {CIRC_FALSE, CIRC_FALSE, 0, 5, 4 | CIRC_NOT, 3, 11, 10 | CIRC_NOT, 9};
    G.shift = std::vector<int32_t>(9, 0);
    G.weight = std::vector<int32_t>(9, 1);
    G.table = {0xF0, 0xCA, 0x96, 0xE8};
    G.outputs = {12, 9 | CIRC_NOT};
    G.out_shift = {0, 0};
    {
        CircuitPlan P;
        CHECK(G.plan(P) == SGFHE_OK && P.levels == 3 && P.live() == 3 && P.siblings() == 1 && P.widest == 1);
        CHECK(P.level[1] == 2 && P.level[2] == 2 && P.level[3] == 3 && P.fam_node[0] == 2 && P.fam_entry[0] == 0x96);
        CHECK(P.out_node[0] == CIRC_NONE && P.out_node[1] == CIRC_NONE);
        // the leader is live through its sibling alone, and none of its own wires has a slot
        CHECK(P.out_slot[3] == CIRC_NONE && P.out_slot[4] == CIRC_NONE && P.out_slot[5] == CIRC_NONE);
        CHECK(P.fam_entry[1] != CIRC_NONE && P.fam_entry[2] != CIRC_NONE && P.fam_entry[3] != CIRC_NONE);
        compared += compare_bits(G, P, 7);
    }
    {   // a level of more than 8192 rows, the boundary inside a leader's rows: 3 leaders x 3000 instances
        Arrays B;
        B.n_inputs = 1;
        B.start.push_back(0);
        for (int f = 0; f < 3; f++)
            for (int m = 0; m < 3; m++) {
                B.kind.push_back(m ? 3u : 2u);
                B.table.push_back(0x10u * f + m);
                if (!m) {
                    B.ref.insert(B.ref.end(), {CIRC_FALSE, CIRC_FALSE, 0u});
                    B.shift.insert(B.shift.end(), {0, 0, 0});
                    B.weight.insert(B.weight.end(), {1, 1, 1});
                }
                B.start.push_back((uint32_t)B.ref.size());
                B.outputs.push_back(1 + 3 * (uint32_t)(B.kind.size() - 1));
                B.out_shift.push_back(0);
            }
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK && P.levels == 1 && P.live() == 3 && P.siblings() == 6 && P.level_rows(1, 3000) == 9000);
        check_model(B, P, 3000);
        const CircuitCall C0 = circuit_level_call(P, 1, 0, 3000), C1 = circuit_level_call(P, 1, SGFHE_CIRCUIT_CALL_ROWS, 3000);
        CHECK(C0.rows == 8192 && C0.ka == 0 && C0.kb == 2 && C1.rows == 808 && C1.ka == 2 && C1.kb == 2 && C0.fam && C1.fam);
    }
    auto with = [&](auto &&edit) {
        Arrays B = G;
        edit(B);
        return B;
    };
    refused(with([](Arrays &B) {   // terms on a sibling
        B.start = {0, 3, 6, 7, 10};
        B.ref.insert(B.ref.begin() + 6, CIRC_FALSE), B.shift.push_back(0), B.weight.push_back(1);
    }));
    refused(with([](Arrays &B) { B.kind = {3, 2, 3, 2}; B.start = {0, 0, 3, 3, 6}; B.ref.resize(6); B.outputs = {6, 6}; }));   // first
    refused(with([](Arrays &B) { B.kind[1] = 0; B.start = {0, 3, 5, 5, 8}; B.ref = {CIRC_FALSE, CIRC_FALSE, 0, 3, 3, 11, 10, 9}; }));   // after kind 0
    refused(with([](Arrays &B) { B.kind[1] = 1; B.ref[3] = 3; B.ref[4] = 3; }));   // after kind 1
    refused(with([](Arrays &B) { B.table[2] = 256; }));
    refused(with([](Arrays &B) { B.ref[6] = 10; }));                 // position 0 reads the sibling's scale-1 wire
    refused(with([](Arrays &B) { B.ref[8] = 11; }));                 // position 2 reads its scale-2 wire
    refused(with([](Arrays &B) { B.outputs[1] = 10; }));             // an output of scale 1
    refused(with([](Arrays &B) { B.outputs[1] = 11 | CIRC_NOT; }));  // ... of scale 2
    refused(G, 1);                                                   // kind 3 through sgfhe_circuit_create_lut
    refused(G, 2);                                                   // ... through sgfhe_circuit_create_w
    {   // a classic node reading a sibling's scaled wire; its wire +0 is fine
        Arrays B = G;
        B.kind.push_back(0);
        B.ref.push_back(9), B.ref.push_back(10);
        B.shift.push_back(0), B.shift.push_back(0);
        B.weight.push_back(1), B.weight.push_back(1);
        B.table.push_back(0);
        B.start.push_back(11);
        refused(B);
        B.ref[10] = 12;
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK);
    }
    for (uint32_t members : {256u, 257u}) {   // a leader and 255 siblings is the largest family
        Arrays B;
        B.n_inputs = 1;
        B.kind.assign(members, 3);
        B.kind[0] = 2;
        B.start.assign(members + 1, 3);
        B.start[0] = 0;
        B.ref = {CIRC_FALSE, CIRC_FALSE, 0};
        B.shift = {0, 0, 0};
        B.weight = {1, 1, 1};
        B.table.assign(members, 0x96);
        B.outputs = {1 + 3 * (members - 1)};
        B.out_shift = {0};
        if (members == 257) {
            refused(B);
            continue;
        }
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK && P.live() == 1 && P.siblings() == 1 && P.fam_node[0] == 255 && P.slots == 2);
        check_model(B, P, 5);
    }
    printf("ok %zu\n", compared);
    return 0;
}
