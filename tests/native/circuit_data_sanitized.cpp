// Data planes of csrc/circuit.h (sgfhe_circuit_create_data) under AddressSanitizer and UndefinedBehaviorSanitizer on the
// CPU (tests/test_circuit_data_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form that mix classic nodes, sum nodes, LUT nodes, data LUT nodes (kind 4) and families
//     of constant (kind 3) and data (kind 5) siblings and obey the scale rule, with NOTs, constants and (for G > 1) lane
//     shifts, are planned for (group, instances) = (1, 5), (4, 24) and (8, 72) and (1, 130), and circuit_plain_bits with
//     random planes is compared, bit by bit, with an evaluation of the ORIGINAL arrays one instance at a time: a data
//     node's or data sibling's table at instance t is data[plane][t], at its OWN instance whatever its terms' shifts;
//   - the plan against the plan of the same arrays with kind 4 read as 2 and kind 5 read as 3 (the plane's low byte as
//     the table): every table but the table bits of node_kind and fam_entry[4 i] is equal, those name the planes behind
//     CIRC_DATA, and the low byte of a data node's kind word is 2; the call arithmetic is the twin's, call by call;
//   - arrays without kinds 4 and 5 and n_planes = 0 give the plan of sgfhe_circuit_create_lut_multi, word by word;
//   - the inputs the planner must refuse -- a plane that is not below n_planes, n_planes above the cap, kind 6, a kind-5
//     node first or behind a classic or a sum node, terms on a kind-5 node, a family of 257 with mixed members, the scale
//     violations through data wires, kinds 4 and 5 through sgfhe_circuit_create_lut_multi and sgfhe_circuit_create_lut,
//     missing planes in circuit_plain_bits -- return SGFHE_ERR_INVALID_ARG without a single allocation (the global
//     operator new is counted) and leave the plan they were given untouched; a mixed family of 256 is accepted.
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

static uint64_t g_state = 0x13198A2E03707344ull;
static uint32_t rnd(uint32_t below) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % below);
}

struct Arrays {
    uint32_t n_inputs = 0, group = 1, n_planes = 0;
    std::vector<uint32_t> kind, start, ref, table, outputs;
    std::vector<int32_t> shift, weight, out_shift;
    size_t n_gates() const { return kind.size(); }
    // through the entry that admits kinds 0 .. max_kind; only sgfhe_circuit_create_data (5) takes the planes
    int32_t plan_kinds(uint32_t max_kind, CircuitPlan &P) const {
        return circuit_plan(spec_csr(max_kind, n_inputs, max_kind == 5 ? n_planes : 0, kind.data(), start.data(), ref.data(),
                                     shift.data(), weight.data(), table.data(), n_gates(), outputs.data(), out_shift.data(),
                                     outputs.size(), group), P);
    }
    int32_t plan(CircuitPlan &P) const { return plan_kinds(5, P); }
    int32_t plan_multi(CircuitPlan &P) const { return plan_kinds(3, P); }
    int32_t plan_lut(CircuitPlan &P) const { return plan_kinds(2, P); }
    bool sibling(size_t g) const { return kind[g] == 3 || kind[g] == 5; }
    bool data(size_t g) const { return kind[g] == 4 || kind[g] == 5; }
    size_t leader(size_t g) const {
        while (sibling(g)) g--;
        return g;
    }
    // kind 4 read as 2, kind 5 read as 3, the plane's low byte as the table
    Arrays twin() const {
        Arrays Z = *this;
        Z.n_planes = 0;
        for (size_t g = 0; g < n_gates(); g++)
            if (data(g)) Z.kind[g] -= 2, Z.table[g] &= 0xFFu;
        return Z;
    }
};

static int32_t a_shift(uint32_t group) { return group > 1 ? (int32_t)rnd(2 * group - 1) - (int32_t)(group - 1) : 0; }

// A random circuit that obeys the scale rule; `planes`: how many planes it may name (0: no kind 4 or 5 at all).
static Arrays random_circuit(uint32_t n_inputs, size_t n_nodes, uint32_t group, uint32_t planes) {
    Arrays A;
    A.n_inputs = n_inputs;
    A.group = group;
    A.n_planes = planes;
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
    auto close = [&](bool lut) {
        A.start.push_back((uint32_t)A.ref.size());
        const uint32_t base = n_inputs + 3 * (uint32_t)(A.n_gates() - 1);
        for (uint32_t w = 0; w < 3; w++) by_scale[lut ? w : 0].push_back(base + w);
    };
    auto lut_node = [&](bool sib) {   // constant or data, at random
        const bool d = planes && rnd(2);
        A.kind.push_back((sib ? 3u : 2u) + (d ? 2u : 0u));
        A.table.push_back(d ? rnd(planes) : rnd(256));
    };
    A.start.push_back(0);
    for (size_t g = 0; g < n_nodes; g++) {
        const uint32_t k = rnd(3);
        if (k == 0) {
            A.kind.push_back(0), A.table.push_back(0x12345u);   // (read for LUT nodes and siblings only)
            term(pick(0), 1);
            term(pick(0), 1);
        } else if (k == 1) {
            A.kind.push_back(1), A.table.push_back(0x12345u);
            static const int32_t ws[4] = {-2, -1, 1, 2};
            for (uint32_t j = 0, nj = 1 + rnd(5); j < nj; j++) term(pick(0), ws[rnd(4)]);
        } else {
            lut_node(false);
            for (uint32_t p = 0; p < 3; p++) term(pick(2 - p), 1);
        }
        close(k == 2);
        for (uint32_t s = 0, ns = k == 2 ? rnd(5) : 0; s < ns; s++) {
            lut_node(true);
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
static std::vector<std::vector<uint8_t>> evaluate(const Arrays &A, const std::vector<uint8_t> &in_bits,
                                                  const std::vector<uint8_t> &data, size_t inst) {
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
            } else {   // a LUT node, or a sibling at its leader's terms; a data table at the node's own instance
                const uint32_t s = read(t0, t) + 2 * read(t0 + 1, t) + 4 * read(t0 + 2, t);
                const uint32_t tb = A.data(g) ? data[(size_t)A.table[g] * inst + t] : A.table[g];
                val[base][t] = val[base + 1][t] = val[base + 2][t] = (tb >> s) & 1;
            }
        }
    }
    return val;
}

static size_t compare_bits(const Arrays &A, const CircuitPlan &P, size_t inst) {
    std::vector<uint8_t> in_bits(A.n_inputs * inst), data((size_t)A.n_planes * inst);
    for (auto &b : in_bits) b = (uint8_t)(rnd(2) | (rnd(2) << 1));   // (only bit 0 counts)
    for (auto &b : data) b = (uint8_t)rnd(256);
    std::vector<uint64_t> table;
    CHECK(circuit_plain_bits(P, in_bits.data(), inst, table, A.n_planes ? data.data() : nullptr) == SGFHE_OK);
    const auto val = evaluate(A, in_bits, data, inst);
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

// the plan of the data arrays against the plan of their constant twin: equal but for the table bits
static void check_twin(const Arrays &A, const CircuitPlan &P, size_t inst) {
    CircuitPlan Z;
    CHECK(A.twin().plan_multi(Z) == SGFHE_OK);
    CHECK(P.n_planes == A.n_planes && Z.n_planes == 0);
    CHECK(P.levels == Z.levels && P.widest == Z.widest && P.slots == Z.slots && P.group == Z.group && P.level == Z.level &&
          P.order == Z.order && P.level_start == Z.level_start && P.input_slot == Z.input_slot &&
          P.term_start == Z.term_start && P.term_ref == Z.term_ref && P.term_shift == Z.term_shift &&
          P.term_weight == Z.term_weight && P.term_row == Z.term_row && P.sum_before == Z.sum_before &&
          P.lut_before == Z.lut_before && P.out_slot == Z.out_slot && P.out_ref == Z.out_ref && P.out_shift == Z.out_shift &&
          P.out_node == Z.out_node && P.out_gate == Z.out_gate && P.jobs == Z.jobs && P.job_k == Z.job_k &&
          P.fam_start == Z.fam_start && P.fam_node == Z.fam_node);
    CHECK(P.at.words == Z.at.words && P.at.node_kind == Z.at.node_kind && P.at.fam_entry == Z.at.fam_entry &&
          P.at.fam_start == Z.at.fam_start && P.image.size() == Z.image.size());
    CHECK(P.node_kind.size() == Z.node_kind.size() && P.fam_entry.size() == Z.fam_entry.size());
    size_t differ = 0;
    for (size_t k = 0; k < P.node_kind.size(); k++) {
        const size_t g = k < P.live() ? P.order[k] : 0;
        CHECK(P.kind(k) == Z.kind(k));
        if (k < P.live() && A.data(g)) {
            CHECK(P.kind(k) == 2 && (P.node_kind[k] & CIRC_DATA) && ((P.node_kind[k] >> 8) & 0xFFFFu) == A.table[g]);
            CHECK((P.node_kind[k] & ~(CIRC_DATA | 0xFFFFFFu)) == 0);
            differ += P.node_kind[k] != Z.node_kind[k];
        } else {
            CHECK(P.node_kind[k] == Z.node_kind[k] && !(P.node_kind[k] & CIRC_DATA));
        }
    }
    for (size_t i = 0; i < P.siblings(); i++) {
        const size_t h = P.fam_node[i];
        for (uint32_t w = 1; w < 4; w++) CHECK(P.fam_entry[4 * i + w] == Z.fam_entry[4 * i + w]);
        if (A.data(h)) {
            CHECK(P.fam_entry[4 * i] == (CIRC_DATA | A.table[h]));
            differ += P.fam_entry[4 * i] != Z.fam_entry[4 * i];
        } else {
            CHECK(P.fam_entry[4 * i] == A.table[h] && Z.fam_entry[4 * i] == A.table[h]);
        }
    }
    size_t image_differ = 0;
    for (size_t i = 0; i < P.image.size(); i++) image_differ += P.image[i] != Z.image[i];
    CHECK(image_differ == differ);
    for (size_t i = 0; i < P.node_kind.size(); i++) CHECK(P.image[P.at.node_kind + i] == P.node_kind[i]);
    for (size_t i = 0; i < P.fam_entry.size() && P.siblings(); i++) CHECK(P.image[P.at.fam_entry + i] == P.fam_entry[i]);
    // the calls of a run: the twin's
    CHECK(circuit_probe_rows(P) == circuit_probe_rows(Z));
    for (uint32_t L = 1; L <= P.levels; L++)
        for (uint64_t row0 = 0; row0 < P.level_rows(L, inst); row0 += SGFHE_CIRCUIT_CALL_ROWS) {
            const CircuitCall C = circuit_level_call(P, L, row0, inst), D = circuit_level_call(Z, L, row0, inst);
            CHECK(C.k0 == D.k0 && C.rows == D.rows && C.ka == D.ka && C.kb == D.kb && C.j0 == D.j0 && C.j1 == D.j1 &&
                  C.sum == D.sum && C.lut == D.lut && C.fam == D.fam);
        }
    const CircuitRunSizes S = circuit_run_sizes(P, inst, 8, 1, false, false, false), T = circuit_run_sizes(Z, inst, 8, 1, false, false, false);
    CHECK(S.max_rows == T.max_rows && S.work_rows == T.work_rows);
}

static void refused(const Arrays &A, int through = 0) {
    CircuitPlan P;
    P.n_inputs = 77;   // (must survive)
    const size_t before = g_allocs;
    const int32_t rc = through == 2 ? A.plan_lut(P) : (through == 1 ? A.plan_multi(P) : A.plan(P));
    CHECK(rc == SGFHE_ERR_INVALID_ARG && g_allocs == before && P.n_inputs == 77 && P.order.empty());
}

int main() {
    size_t compared = 0;
    const uint32_t cfg[4][2] = {{1, 5}, {4, 24}, {8, 72}, {1, 130}};
    size_t with_data_siblings = 0, with_data_nodes = 0;
    for (const auto &gc : cfg)
        for (int rep = 0; rep < 40; rep++) {
            const Arrays A = random_circuit(1 + rnd(4), 1 + rnd(16), gc[0], 1 + rnd(rep % 2 ? 3 : 300));
            CircuitPlan P;
            CHECK(A.plan(P) == SGFHE_OK);
            check_twin(A, P, gc[1]);
            compared += compare_bits(A, P, gc[1]);
            bool ds = false, dn = false;
            for (size_t i = 0; i < P.siblings(); i++) ds |= (P.fam_entry[4 * i] & CIRC_DATA) != 0;
            for (size_t k = 0; k < P.live(); k++) dn |= (P.node_kind[k] & CIRC_DATA) != 0;
            with_data_siblings += ds, with_data_nodes += dn;
        }
    CHECK(with_data_siblings > 40 && with_data_nodes > 60);
    // without kinds 4 and 5, n_planes = 0: the plan of sgfhe_circuit_create_lut_multi
    for (int rep = 0; rep < 20; rep++) {
        const Arrays A = random_circuit(1 + rnd(4), 1 + rnd(24), rep % 2 ? 4 : 1, 0);
        CircuitPlan P, W;
        CHECK(A.plan(P) == SGFHE_OK && A.plan_multi(W) == SGFHE_OK);
        CHECK(same_tables(P, W) && P.image == W.image && P.lut_before == W.lut_before && P.fam_start == W.fam_start &&
              P.fam_entry == W.fam_entry && P.fam_node == W.fam_node && P.n_planes == 0);
        compared += compare_bits(A, P, rep % 2 ? 24 : 5);
    }
    // ---- 3 inputs, 2 planes; node 0 = fan(in 0): wires 3, 4, 5; node 1 = data lut(5, ~4, 3) of plane 1: wires 6, 7, 8;
    // node 2 = its data sibling of plane 0: wires 9, 10, 11; node 3 = its constant sibling: wires 12, 13, 14; node 4 =
    // lut(11, ~10, 12) reads the siblings: wires 15, 16, 17
    Arrays G;
    G.n_inputs = 3, G.n_planes = 2;
    G.kind = {2, 4, 5, 3, 2};
    G.start = {0, 3, 6, 6, 6, 9};
    G.ref = {CIRC_FALSE, CIRC_FALSE, 0, 5, 4 | CIRC_NOT, 3, 11, 10 | CIRC_NOT, 12};
    G.shift = std::vector<int32_t>(9, 0);
    G.weight = std::vector<int32_t>(9, 1);
    G.table = {0xF0, 1, 0, 0x96, 0xE8};
    G.outputs = {15, 9 | CIRC_NOT, 6};
    G.out_shift = {0, 0, 0};
    {
        CircuitPlan P;
        CHECK(G.plan(P) == SGFHE_OK && P.levels == 3 && P.live() == 3 && P.siblings() == 2 && P.widest == 1 && P.n_planes == 2);
        CHECK(P.node_kind[1] == (2u | CIRC_DATA | 1u << 8) && P.fam_entry[0] == (CIRC_DATA | 0u) && P.fam_entry[4] == 0x96);
        CHECK(P.out_node[0] == CIRC_NONE && P.out_node[1] == CIRC_NONE && P.out_node[2] == CIRC_NONE);   // refreshed or lifted
        check_twin(G, P, 7);
        compared += compare_bits(G, P, 7);
        // planes are needed where the plan has any and there is an instance
        std::vector<uint8_t> in_bits(3 * 7, 1);
        std::vector<uint64_t> table;
        CHECK(circuit_plain_bits(P, in_bits.data(), 7, table, nullptr) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plain_bits(P, in_bits.data(), 0, table, nullptr) == SGFHE_OK);
    }
    {   // a level of more than 8192 rows, the boundary inside a data leader with two data siblings
        Arrays B;
        B.n_inputs = 1, B.n_planes = 9;
        B.start.push_back(0);
        for (int f = 0; f < 3; f++)
            for (int m = 0; m < 3; m++) {
                B.kind.push_back(m ? 5u : 4u);
                B.table.push_back(3u * f + m);
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
        check_twin(B, P, 3000);
        const CircuitCall C0 = circuit_level_call(P, 1, 0, 3000), C1 = circuit_level_call(P, 1, SGFHE_CIRCUIT_CALL_ROWS, 3000);
        CHECK(C0.rows == 8192 && C0.ka == 0 && C0.kb == 2 && C1.rows == 808 && C1.ka == 2 && C1.kb == 2 && C0.fam && C1.fam);
        compared += compare_bits(B, P, 3000);
    }
    auto with = [&](auto &&edit) {
        Arrays B = G;
        edit(B);
        return B;
    };
    refused(with([](Arrays &B) { B.table[1] = 2; }));                   // a plane that is not below n_planes, on a node
    refused(with([](Arrays &B) { B.table[2] = 2; }));                   // ... on a sibling
    refused(with([](Arrays &B) { B.table[2] = 0xFFFFFFFFu; }));
    refused(with([](Arrays &B) { B.n_planes = SGFHE_CIRCUIT_MAX_PLANES + 1; }));
    refused(with([](Arrays &B) { B.n_planes = 0; }));                   // no plane at all
    refused(with([](Arrays &B) { B.kind[2] = 6; }));
    refused(with([](Arrays &B) {   // terms on a data sibling
        B.start = {0, 3, 6, 7, 7, 10};
        B.ref.insert(B.ref.begin() + 6, CIRC_FALSE), B.shift.push_back(0), B.weight.push_back(1);
    }));
    refused(with([](Arrays &B) {   // a data sibling first
        B.kind = {5, 2};
        B.start = {0, 0, 3};
        B.table = {0, 0xF0};
        B.ref.resize(3), B.shift.resize(3), B.weight.resize(3);
        B.outputs = {6, 6, 6};
    }));
    refused(with([](Arrays &B) {   // ... behind a classic node
        B.kind = {2, 0, 5};
        B.start = {0, 3, 5, 5};
        B.table = {0xF0, 0, 0};
        B.ref = {CIRC_FALSE, CIRC_FALSE, 0, 3, 3};
        B.outputs = {6, 6, 6};
    }));
    refused(with([](Arrays &B) {   // ... behind a sum node
        B.kind = {2, 1, 5};
        B.start = {0, 3, 6, 6};
        B.table = {0xF0, 0, 0};
        B.ref = {CIRC_FALSE, CIRC_FALSE, 0, 3, 3, 3};
        B.outputs = {6, 6, 6};
    }));
    refused(with([](Arrays &B) { B.ref[6] = 10; }));                    // position 0 reads the data sibling's scale-1 wire
    refused(with([](Arrays &B) { B.ref[8] = 8; }));                     // position 2 reads the data node's scale-2 wire
    refused(with([](Arrays &B) { B.outputs[1] = 10; }));                // an output of scale 1
    refused(with([](Arrays &B) { B.outputs[2] = 8 | CIRC_NOT; }));      // ... of scale 2
    refused(G, 1);                                                      // kinds 4 and 5 through sgfhe_circuit_create_lut_multi
    refused(G, 2);                                                      // ... through sgfhe_circuit_create_lut
    refused(with([](Arrays &B) { B.kind[2] = 3; B.table[2] = 0x17; }), 1);   // kind 4 alone through ..._lut_multi
    for (uint32_t members : {256u, 257u}) {   // a leader and 255 siblings, constant and data ones, is the largest family
        Arrays B;
        B.n_inputs = 1, B.n_planes = 3;
        B.kind.resize(members);
        B.table.resize(members);
        for (uint32_t i = 0; i < members; i++) B.kind[i] = (i ? 3u : 2u) + (i % 2 ? 2u : 0u), B.table[i] = i % 2 ? i % 3 : i & 0xFFu;
        B.start.assign(members + 1, 3);
        B.start[0] = 0;
        B.ref = {CIRC_FALSE, CIRC_FALSE, 0};
        B.shift = {0, 0, 0};
        B.weight = {1, 1, 1};
        B.outputs = {1 + 3 * (members - 1)};
        B.out_shift = {0};
        if (members == 257) {
            refused(B);
            continue;
        }
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK && P.live() == 1 && P.siblings() == 1 && P.fam_node[0] == 255 && P.slots == 2);
        CHECK(P.fam_entry[0] == (CIRC_DATA | 255u % 3));
        check_twin(B, P, 5);
        compared += compare_bits(B, P, 5);
    }
    {   // n_planes at the cap, the last plane named
        Arrays B = G;
        B.n_planes = SGFHE_CIRCUIT_MAX_PLANES;
        B.table[1] = SGFHE_CIRCUIT_MAX_PLANES - 1;
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK && ((P.node_kind[1] >> 8) & 0xFFFFu) == 0xFFFFu && P.kind(1) == 2 &&
              (P.node_kind[1] & CIRC_DATA));
    }
    printf("ok %zu\n", compared);
    return 0;
}
