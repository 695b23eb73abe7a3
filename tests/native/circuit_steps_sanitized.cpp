// Registers of csrc/circuit.h (sgfhe_circuit_create_seq) under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU
// (tests/test_circuit_steps_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form (classic nodes, sum nodes, LUT nodes behind a fan; NOTs, constants and, for G > 1,
//     lane shifts) with random registers and next-state references are planned, and the plan is compared with the STEP
//     PLAN -- the sgfhe_circuit_create_data plan of the same nodes with outputs = outputs ++ next_ref: level, order,
//     level_start, slots, input_slot, out_slot, the live nodes' part of the node table, the call arithmetic, and
//     next_ref / next_shift against the step plan's last out_ref / out_shift entries; the image's register tables;
//   - with n_regs = 0 the plan is the sgfhe_circuit_create_data plan field for field and its image byte for byte;
//   - a node reached only through next_ref is live, and a register only next_ref reads has a slot;
//   - scaled registers: a LUT node reads registers of scales 2, 1, 0 at positions 0, 1, 2 and feeds them back; a constant
//     is accepted at any scale;
//   - the inputs the planner must refuse -- n_regs above n_inputs, a next-state reference out of range or carrying
//     SGFHE_CIRCUIT_NONE, a shift outside the group, reg_scale 3, a scale mismatch between a register and its next
//     reference, a scaled register read by a classic node, NULL next_ref -- return SGFHE_ERR_INVALID_ARG without a
//     single allocation (the global operator new is counted, in the build without sanitizers) and leave the plan they
//     were given untouched.
// Prints "ok <words compared>".
#include <stdio.h>
#include <stdlib.h>

#include <new>
#include <vector>

// (the sanitized build links the sanitizer's runtime statically, which defines the global operator new itself: the
// allocations are counted in the plain build, -DCOUNT_ALLOCATIONS, which runs the same checks)
static size_t g_allocs = 0;
#ifdef COUNT_ALLOCATIONS
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
#endif

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

static size_t g_compared = 0;
template <class T>
static void same(const std::vector<T> &a, const std::vector<T> &b) {
    CHECK(a == b);
    g_compared += a.size();
}

struct Arrays {
    uint32_t n_inputs = 0, group = 1, n_planes = 0, n_regs = 0;
    std::vector<uint32_t> kind, start, ref, table, outputs, next_ref, reg_scale;
    std::vector<int32_t> shift, weight, out_shift, next_shift;
    size_t n_gates() const { return kind.size(); }
    // what sgfhe_circuit_create_data fills, then (spec) the registers of sgfhe_circuit_create_seq
    CircuitSpec spec_data() const {
        return spec_csr(5, n_inputs, n_planes, kind.data(), start.data(), ref.data(), shift.data(), weight.data(), table.data(),
                        n_gates(), outputs.data(), out_shift.data(), outputs.size(), group);
    }
    CircuitSpec spec() const {
        CircuitSpec S = spec_data();
        S.regs.n_regs = n_regs, S.regs.next_ref = next_ref.data();
        S.regs.next_shift = next_shift.data(), S.regs.reg_scale = reg_scale.data();
        return S;
    }
    int32_t plan(CircuitPlan &P) const { return circuit_plan(spec(), P); }
    // the same with next_shift and reg_scale NULL
    int32_t plan_null(CircuitPlan &P) const {
        CircuitSpec S = spec();
        S.regs.next_shift = nullptr, S.regs.reg_scale = nullptr;
        return circuit_plan(S, P);
    }
    int32_t plan_data(CircuitPlan &P) const { return circuit_plan(spec_data(), P); }
    // no registers, outputs = outputs ++ next_ref
    Arrays step() const {
        Arrays Z = *this;
        Z.n_regs = 0;
        Z.outputs.insert(Z.outputs.end(), next_ref.begin(), next_ref.end());
        Z.out_shift.insert(Z.out_shift.end(), next_shift.begin(), next_shift.end());
        Z.next_ref.clear(), Z.next_shift.clear(), Z.reg_scale.clear();
        return Z;
    }
};

static int32_t a_shift(uint32_t group) { return group > 1 ? (int32_t)rnd(2 * group - 1) - (int32_t)(group - 1) : 0; }

// A random circuit that obeys the scale rule, every register of scale 0
static Arrays random_circuit(uint32_t n_inputs, uint32_t n_regs, size_t n_nodes, uint32_t group) {
    Arrays A;
    A.n_inputs = n_inputs;
    A.n_regs = n_regs;
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
    for (size_t g = 0; g < n_nodes; g++) {
        const uint32_t what = rnd(4);
        bool lut = false;
        if (what == 0) {
            A.kind.push_back(0), A.table.push_back(0);
            term(pick(0), 1), term(pick(0), 1);
        } else if (what == 1) {
            A.kind.push_back(1), A.table.push_back(0);
            static const int32_t W[4] = {-2, -1, 1, 2};
            for (uint32_t i = 0, cnt = 1 + rnd(5); i < cnt; i++) term(pick(0), W[rnd(4)]);
        } else {
            lut = true;
            A.kind.push_back(2), A.table.push_back(rnd(256));
            term(pick(2), 1), term(pick(1), 1), term(pick(0), 1);
        }
        A.start.push_back((uint32_t)A.ref.size());
        const uint32_t base = n_inputs + 3 * (uint32_t)g;
        for (uint32_t w = 0; w < 3; w++) by_scale[lut ? w : 0].push_back(base + w);
    }
    for (uint32_t o = 0, cnt = 1 + rnd(3); o < cnt; o++) A.outputs.push_back(pick(0)), A.out_shift.push_back(a_shift(group));
    for (uint32_t i = 0; i < n_regs; i++) {
        A.next_ref.push_back(pick(0)), A.next_shift.push_back(a_shift(group)), A.reg_scale.push_back(0);
    }
    return A;
}

static void compare_with_step_plan(const Arrays &A, uint64_t instances) {
    CircuitPlan P, Z;
    CHECK(A.plan(P) == SGFHE_OK);
    CHECK(A.step().plan_data(Z) == SGFHE_OK);
    CHECK(P.n_regs == A.n_regs && Z.n_regs == 0 && P.n_stream() == A.n_inputs - A.n_regs);
    CHECK(P.levels == Z.levels && P.widest == Z.widest && P.slots == Z.slots && P.n_outputs + P.n_regs == Z.n_outputs);
    same(P.level, Z.level);
    same(P.order, Z.order);
    same(P.level_start, Z.level_start);
    same(P.input_slot, Z.input_slot);
    same(P.out_slot, Z.out_slot);
    same(P.fam_start, Z.fam_start);
    same(P.fam_entry, Z.fam_entry);
    same(P.sum_before, Z.sum_before);
    same(P.lut_before, Z.lut_before);
    // the live nodes' part of the node table (the pack stage's pseudo-level differs: it has one node per output)
    const size_t live = P.live(), terms = P.term_start[live];
    CHECK(terms == Z.term_start[live]);
    for (size_t k = 0; k <= live; k++) CHECK(P.term_start[k] == Z.term_start[k]);
    for (size_t k = 0; k < live; k++) CHECK(P.node_kind[k] == Z.node_kind[k]);
    for (size_t i = 0; i < terms; i++)
        CHECK(P.term_ref[i] == Z.term_ref[i] && P.term_shift[i] == Z.term_shift[i] && P.term_weight[i] == Z.term_weight[i]);
    g_compared += 3 * terms + 2 * live;
    // outputs, then the next states, are the step plan's outputs
    for (size_t o = 0; o < P.n_outputs; o++) CHECK(P.out_ref[o] == Z.out_ref[o] && P.out_shift[o] == Z.out_shift[o]);
    for (size_t i = 0; i < P.n_regs; i++) {
        CHECK(P.next_ref[i] == Z.out_ref[P.n_outputs + i] && P.next_shift[i] == Z.out_shift[P.n_outputs + i]);
        CHECK(P.reg_scale[i] == 0 && P.reg_index[i] == i);
        const uint32_t slot = P.next_ref[i] & ~CIRC_NOT;
        CHECK(slot == CIRC_FALSE || slot < P.slots);
    }
    g_compared += 2 * (size_t)Z.n_outputs;
    // the register tables of the image, behind everything else; the image in front of them is that of the tables
    if (P.n_regs) {
        CHECK(P.at.words == P.image.size() && P.at.reg_index + P.n_regs == P.at.words);
        CHECK(P.at.next_ref < P.at.next_shift && P.at.next_shift < P.at.next_scale && P.at.next_scale < P.at.reg_index);
        CHECK(P.at.next_ref >= P.at.jobs + P.jobs.size());
        for (uint32_t i = 0; i < P.n_regs; i++) {
            CHECK(P.image[P.at.next_ref + i] == P.next_ref[i] && P.image[P.at.next_shift + i] == (uint32_t)P.next_shift[i]);
            CHECK(P.image[P.at.next_scale + i] == P.reg_scale[i] && P.image[P.at.reg_index + i] == i);
            CHECK(P.image[P.at.input_slot + i] == P.input_slot[i]);
        }
        g_compared += 5 * (size_t)P.n_regs;
    } else {
        CHECK(P.at.next_ref == 0 && P.at.next_shift == 0 && P.at.next_scale == 0 && P.at.reg_index == 0);
    }
    // the call arithmetic of a step is the step plan's, call by call
    if (instances % A.group == 0) {
        for (uint32_t L = 1; L <= P.levels; L++)
            for (uint64_t row0 = 0; row0 < P.level_rows(L, instances); row0 += SGFHE_CIRCUIT_CALL_ROWS) {
                const CircuitCall a = circuit_level_call(P, L, row0, instances), b = circuit_level_call(Z, L, row0, instances);
                CHECK(a.k0 == b.k0 && a.rows == b.rows && a.ka == b.ka && a.kb == b.kb && a.sum == b.sum && a.lut == b.lut &&
                      a.fam == b.fam);
                g_compared += 7;
            }
        const CircuitRunSizes sa = circuit_run_sizes(P, instances, 64, 0, false, false, false);
        const CircuitRunSizes sb = circuit_run_sizes(Z, instances, 64, 0, false, false, false);
        CHECK(sa.max_rows == sb.max_rows && sa.work_rows == sb.work_rows);
    }
}

static void no_registers_is_the_data_plan(const Arrays &A0) {
    Arrays A = A0;
    A.n_regs = 0;
    A.next_ref.clear(), A.next_shift.clear(), A.reg_scale.clear();
    CircuitPlan P, Z, N;
    CHECK(A.plan(P) == SGFHE_OK && A.plan_null(N) == SGFHE_OK && A.plan_data(Z) == SGFHE_OK);
    for (const CircuitPlan *Q : {&P, &N}) {
        CHECK(Q->n_inputs == Z.n_inputs && Q->n_gates == Z.n_gates && Q->n_outputs == Z.n_outputs && Q->levels == Z.levels &&
              Q->widest == Z.widest && Q->slots == Z.slots && Q->group == Z.group && Q->n_planes == Z.n_planes && Q->n_regs == 0);
        same(Q->level, Z.level), same(Q->order, Z.order), same(Q->level_start, Z.level_start), same(Q->input_slot, Z.input_slot);
        same(Q->node_kind, Z.node_kind), same(Q->term_start, Z.term_start), same(Q->term_ref, Z.term_ref);
        same(Q->term_shift, Z.term_shift), same(Q->term_weight, Z.term_weight), same(Q->out_slot, Z.out_slot);
        same(Q->out_ref, Z.out_ref), same(Q->out_shift, Z.out_shift), same(Q->out_node, Z.out_node), same(Q->out_gate, Z.out_gate);
        same(Q->jobs, Z.jobs), same(Q->job_k, Z.job_k), same(Q->term_row, Z.term_row), same(Q->sum_before, Z.sum_before);
        same(Q->lut_before, Z.lut_before), same(Q->fam_start, Z.fam_start), same(Q->fam_entry, Z.fam_entry);
        same(Q->fam_node, Z.fam_node), same(Q->image, Z.image);
        CHECK(Q->next_ref.empty() && Q->next_shift.empty() && Q->reg_scale.empty() && Q->reg_index.empty());
        CHECK(Q->at.words == Z.at.words && Q->at.jobs == Z.at.jobs && Q->at.fam_start == Z.at.fam_start &&
              Q->at.fam_entry == Z.at.fam_entry && Q->at.next_ref == 0 && Q->at.reg_index == 0);
    }
}

// 3 inputs, 2 registers; node 0 = (input 2, register 0): wires 3, 4, 5; node 1 = (3, register 1): wires 6, 7, 8
static Arrays small() {
    Arrays A;
    A.n_inputs = 3, A.n_regs = 2, A.group = 4;
    A.kind = {0, 0}, A.table = {0, 0}, A.start = {0, 2, 4};
    A.ref = {2, 0, 3, 1}, A.shift = {0, 0, 0, 0}, A.weight = {1, 1, 1, 1};
    A.outputs = {3}, A.out_shift = {0};
    A.next_ref = {6 | CIRC_NOT, 0}, A.next_shift = {1, -3}, A.reg_scale = {0, 0};
    return A;
}

// 4 inputs: registers 0, 1, 2 of scales 2, 1, 0 and a stream input; node 0 = lut(0x96; reg 0, reg 1, reg 2): wires 4, 5, 6
// at scales 0, 1, 2, fed back to registers 2, 1, 0 (one negated); node 1 = classic (stream input, wire 4): wires 7, 8, 9
static Arrays scaled() {
    Arrays A;
    A.n_inputs = 4, A.n_regs = 3, A.group = 1;
    A.kind = {2, 0}, A.table = {0x96, 0}, A.start = {0, 3, 5};
    A.ref = {0, 1, 2, 3, 4}, A.shift = {0, 0, 0, 0, 0}, A.weight = {1, 1, 1, 1, 1};
    A.outputs = {7}, A.out_shift = {0};
    A.next_ref = {6, 5 | CIRC_NOT, 4}, A.next_shift = {0, 0, 0}, A.reg_scale = {2, 1, 0};
    return A;
}

static void refused(const Arrays &A, int line) {
    CircuitPlan P;
    P.slots = 77, P.n_regs = 5;   // (a plan the refusal must leave as it is)
    const size_t before = g_allocs;
    const int32_t rc = A.plan(P);
    if (rc != SGFHE_ERR_INVALID_ARG || g_allocs != before || P.slots != 77 || P.n_regs != 5) {
        fprintf(stderr, "case at line %d: rc %d, %zu allocations\n", line, rc, g_allocs - before);
        abort();
    }
    g_compared++;
}
#define REFUSED(A) refused(A, __LINE__)

int main() {
    // ---- random circuits against their step plans
    static const uint32_t shapes[][2] = {{1, 5}, {4, 24}, {8, 72}, {1, 130}, {2, 8200}};
    for (const auto &sh : shapes)
        for (int rep = 0; rep < 40; rep++) {
            const uint32_t n_inputs = 1 + rnd(6), n_regs = rnd(n_inputs + 1);
            const Arrays A = random_circuit(n_inputs, n_regs, 1 + rnd(14), sh[0]);
            compare_with_step_plan(A, sh[1]);
            no_registers_is_the_data_plan(A);
        }
    // ---- the small plan: node 1 is reached only through next_ref and is live; register 0 is read by node 0 and by its
    // own ... register 1's next state, so both have slots; next_shift NULL reads as 0
    {
        const Arrays A = small();
        CircuitPlan P;
        CHECK(A.plan(P) == SGFHE_OK);
        CHECK(P.live() == 2 && P.level[1] == 2 && P.levels == 2 && P.n_regs == 2 && P.n_stream() == 1);
        CHECK(P.input_slot[0] != CIRC_NONE && P.input_slot[1] != CIRC_NONE);
        CHECK(P.next_ref[0] == (P.out_slot[3 * 1 + 0] | CIRC_NOT) && P.next_ref[1] == P.input_slot[0]);
        CHECK(P.next_shift[0] == 1 && P.next_shift[1] == -3);
        compare_with_step_plan(A, 8);
        CircuitPlan N;
        CHECK(A.plan_null(N) == SGFHE_OK && N.next_shift[0] == 0 && N.next_shift[1] == 0 && N.reg_scale[0] == 0);
        // a register that only its own next state reads still gets a slot; one that nothing reads gets none
        Arrays B = small();
        B.ref[3] = CIRC_FALSE;                     // node 1 no longer reads register 1
        B.next_ref = {6, 1}, B.next_shift = {0, 0};
        CHECK(B.plan(P) == SGFHE_OK && P.input_slot[1] != CIRC_NONE && P.next_ref[1] == P.input_slot[1]);
        B.next_ref = {6, CIRC_FALSE | CIRC_NOT};
        CHECK(B.plan(P) == SGFHE_OK && P.input_slot[1] == CIRC_NONE && P.next_ref[1] == (CIRC_FALSE | CIRC_NOT));
        // the shift beside a constant is dropped, as for outputs
        B.next_shift = {0, 3};
        CHECK(B.plan(P) == SGFHE_OK && P.next_shift[1] == 0);
        // without the next state, node 1 is pruned
        B.next_ref = {3, CIRC_FALSE};
        CHECK(B.plan(P) == SGFHE_OK && P.live() == 1 && P.level[1] == 0);
    }
    // ---- scaled registers
    {
        const Arrays A = scaled();
        CircuitPlan P;
        CHECK(A.plan(P) == SGFHE_OK);
        CHECK(P.reg_scale[0] == 2 && P.reg_scale[1] == 1 && P.reg_scale[2] == 0 && P.live() == 2);
        CHECK(P.image[P.at.next_scale] == 2 && P.image[P.at.next_scale + 1] == 1 && P.image[P.at.next_scale + 2] == 0);
        CHECK(P.next_ref[1] == (P.out_slot[1] | CIRC_NOT));
        Arrays B = A;   // a constant at any scale
        B.next_ref = {CIRC_FALSE, CIRC_FALSE | CIRC_NOT, CIRC_FALSE};
        CHECK(B.plan(P) == SGFHE_OK);
        B = A;          // a register may hold itself at its own scale
        B.next_ref = {0, 1 | CIRC_NOT, 2};
        CHECK(B.plan(P) == SGFHE_OK);
        // mismatches
        B = A, B.next_ref = {5, 5, 4};
        REFUSED(B);     // register 0 (scale 2) fed a scale-1 wire
        B = A, B.next_ref = {6, 5, 6};
        REFUSED(B);     // register 2 (scale 0) fed a scale-2 wire
        B = A, B.next_ref = {6, 5, 1};
        REFUSED(B);     // register 2 (scale 0) fed register 1 (scale 1)
        B = A, B.next_ref = {6, 3, 4};
        REFUSED(B);     // register 1 (scale 1) fed the stream input (scale 0)
        B = A, B.ref[3] = 1;
        REFUSED(B);     // a classic node reads the scale-1 register
        B = A, B.ref[0] = 2;
        REFUSED(B);     // position 0 of the LUT node reads the scale-0 register
        B = A, B.outputs[0] = 0;
        REFUSED(B);     // an output names the scale-2 register
        B = A, B.reg_scale[2] = 3;
        REFUSED(B);
        // no LUT node at all, and a classic node that reads a scale-1 register: the scale rule still applies
        B = small(), B.reg_scale = {1, 0}, B.next_ref = {CIRC_FALSE, 0 };
        REFUSED(B);
    }
    // ---- refused
    {
        Arrays B = small();
        B.n_regs = 4, B.next_ref = {6, 0, 0, 0}, B.next_shift = {0, 0, 0, 0}, B.reg_scale = {0, 0, 0, 0};
        REFUSED(B);     // n_regs above n_inputs
        B = small(), B.next_ref[0] = 9;
        REFUSED(B);     // out of range: the wires are 0 .. 8
        B = small(), B.next_ref[1] = 9 | CIRC_NOT;
        REFUSED(B);
        B = small(), B.next_ref[0] = CIRC_NO_INPUT;
        REFUSED(B);
        B = small(), B.next_ref[0] = CIRC_NO_INPUT | CIRC_NOT;
        REFUSED(B);
        B = small(), B.next_shift[0] = 4;
        REFUSED(B);     // the group is 4
        B = small(), B.next_shift[1] = -4;
        REFUSED(B);
        B = small(), B.next_shift[1] = INT32_MIN;
        REFUSED(B);
        B = small(), B.reg_scale[1] = 3;
        REFUSED(B);
        B = small(), B.reg_scale[0] = 0xFFFFFFFFu;
        REFUSED(B);
        B = small(), B.outputs.clear(), B.out_shift.clear();
        REFUSED(B);     // n_outputs >= 1 stays
        {
            const Arrays A = small();
            CircuitPlan P;
            P.slots = 77;
            CircuitSpec S = A.spec();
            S.nodes.n_planes = 0, S.regs.next_ref = nullptr, S.regs.next_shift = nullptr, S.regs.reg_scale = nullptr;
            const size_t before = g_allocs;
            CHECK(circuit_plan(S, P) == SGFHE_ERR_INVALID_ARG);   // NULL next_ref
            CHECK(g_allocs == before && P.slots == 77);
        }
        B = small(), B.next_shift = {3, -3};
        CircuitPlan P;
        CHECK(B.plan(P) == SGFHE_OK);   // the largest shifts of the group
    }
#ifdef COUNT_ALLOCATIONS
    {   // the counter counts: an accepted plan allocates
        const size_t before = g_allocs;
        CircuitPlan P;
        CHECK(small().plan(P) == SGFHE_OK && g_allocs > before);
    }
#endif
    printf("ok %zu\n", g_compared);
    return 0;
}
