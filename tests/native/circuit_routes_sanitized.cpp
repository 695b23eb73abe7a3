// Lane routes of csrc/circuit.h (sgfhe_circuit_create_routed) under AddressSanitizer and UndefinedBehaviorSanitizer on the
// CPU (tests/test_circuit_routes_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form with every node kind (classic, sum, LUT, sibling, data LUT, data sibling; NOTs,
//     constants, registers), whose references carry a lane shift, a random route table (fills included) or neither,
//     are planned at (G, instances) = (8, 72), (24, 120), (1, 5): everything that must not see routes -- levels, order,
//     slots, the node table, the registers' tables, the call arithmetic -- is that of the plan of the same arrays
//     without routes; the route tables and indices are the caller's, dropped on the constant; a routed output has no
//     out_node; the image carries the four route tables behind every other table;
//   - circuit_plain_bits of the routed plan against a scalar evaluation of the caller's arrays, wire by wire and
//     instance by instance;
//   - with n_routes = 0 (NULL or all-zero index arrays, unused tables aside) the plan is the sgfhe_circuit_create_seq
//     plan field for field and its image word for word;
//   - tables that spell lane shifts give the bits of the shifted plan;
//   - the inputs the planner must refuse -- an entry outside [-1, G), a route index above n_routes, a route beside a
//     non-zero shift, n_routes > 0 with NULL routes, n_routes above SGFHE_CIRCUIT_MAX_ROUTES -- return
//     SGFHE_ERR_INVALID_ARG without a single allocation (the global operator new is counted, in the build without
//     sanitizers) and leave the plan they were given untouched.
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

static uint64_t g_state = 0x13198A2E03707344ull;
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
    uint32_t n_inputs = 0, group = 1, n_planes = 0, n_regs = 0, n_routes = 0;
    std::vector<uint32_t> kind, start, ref, table, outputs, next_ref, reg_scale, term_route, out_route, next_route;
    std::vector<int32_t> shift, weight, out_shift, next_shift, routes;
    size_t n_gates() const { return kind.size(); }
    // what sgfhe_circuit_create_seq fills, then (spec) the routes of sgfhe_circuit_create_routed
    CircuitSpec spec_seq() const {
        CircuitSpec S = spec_csr(5, n_inputs, n_planes, kind.data(), start.data(), ref.data(), shift.data(), weight.data(),
                                 table.data(), n_gates(), outputs.data(), out_shift.data(), outputs.size(), group);
        S.regs.n_regs = n_regs, S.regs.next_ref = next_ref.data();
        S.regs.next_shift = next_shift.data(), S.regs.reg_scale = reg_scale.data();
        return S;
    }
    CircuitSpec spec() const {
        CircuitSpec S = spec_seq();
        S.routes.n_routes = n_routes, S.routes.routes = routes.data(), S.routes.term_route = term_route.data();
        S.routes.out_route = out_route.data(), S.routes.next_route = next_route.data();
        return S;
    }
    int32_t plan(CircuitPlan &P) const { return circuit_plan(spec(), P); }
    // the same arrays without routes: every route index 0
    int32_t plan_seq(CircuitPlan &P) const { return circuit_plan(spec_seq(), P); }
    bool lut(size_t g) const { return kind[g] >= 2; }
    bool sibling(size_t g) const { return kind[g] == 3 || kind[g] == 5; }
    bool data(size_t g) const { return kind[g] >= 4; }
};

// how a reference reads its group: nothing, a shift, or a route (index into the tables made so far; a new table now
// and then, with fills)
struct Lanes {
    int32_t shift;
    uint32_t route;
};
static Lanes a_lanes(Arrays &A) {
    const uint32_t G = A.group, what = rnd(3);
    if (what == 0) return {0, 0};
    if (what == 1) return {G > 1 ? (int32_t)rnd(2 * G - 1) - (int32_t)(G - 1) : 0, 0};
    if (A.n_routes == 0 || rnd(3) == 0) {
        const uint32_t form = rnd(4);   // random with fills, a permutation-like rotation, a broadcast, all fill
        const uint32_t d = rnd(G), lane = rnd(G);
        for (uint32_t t = 0; t < G; t++)
            A.routes.push_back(form == 0 ? (int32_t)rnd(G + 1) - 1 : form == 1 ? (int32_t)((t + d) % G) : form == 2 ? (int32_t)lane : -1);
        A.n_routes++;
    }
    return {0, 1 + rnd(A.n_routes)};
}

// A random circuit that obeys the scale rule, every register of scale 0
static Arrays random_circuit(uint32_t n_inputs, uint32_t n_regs, size_t n_nodes, uint32_t group, uint32_t n_planes) {
    Arrays A;
    A.n_inputs = n_inputs, A.n_regs = n_regs, A.group = group, A.n_planes = n_planes;
    std::vector<uint32_t> by_scale[3];
    for (uint32_t i = 0; i < n_inputs; i++) by_scale[0].push_back(i);
    auto pick = [&](uint32_t scale) -> uint32_t {
        uint32_t r = by_scale[scale].empty() || rnd(8) == 0 ? CIRC_FALSE : by_scale[scale][rnd((uint32_t)by_scale[scale].size())];
        return rnd(3) == 0 ? r | CIRC_NOT : r;
    };
    auto term = [&](uint32_t r, int32_t w) {
        const Lanes l = a_lanes(A);
        A.ref.push_back(r), A.shift.push_back(l.shift), A.term_route.push_back(l.route), A.weight.push_back(w);
    };
    A.start.push_back(0);
    for (size_t g = 0; g < n_nodes; g++) {
        const uint32_t what = rnd(5);
        const bool prev_lut = g > 0 && A.lut(g - 1);
        if (what == 0) {
            A.kind.push_back(0), A.table.push_back(0);
            term(pick(0), 1), term(pick(0), 1);
        } else if (what == 1) {
            A.kind.push_back(1), A.table.push_back(0);
            static const int32_t W[4] = {-2, -1, 1, 2};
            for (uint32_t i = 0, cnt = 1 + rnd(5); i < cnt; i++) term(pick(0), W[rnd(4)]);
        } else if (what == 2 && prev_lut) {   // a sibling of the family in front of it, constant or data
            const bool dat = n_planes && rnd(2);
            A.kind.push_back(dat ? 5 : 3), A.table.push_back(dat ? rnd(n_planes) : rnd(256));
        } else {
            const bool dat = n_planes && rnd(2);
            A.kind.push_back(dat ? 4 : 2), A.table.push_back(dat ? rnd(n_planes) : rnd(256));
            term(pick(2), 1), term(pick(1), 1), term(pick(0), 1);
        }
        A.start.push_back((uint32_t)A.ref.size());
        const uint32_t base = n_inputs + 3 * (uint32_t)g;
        for (uint32_t w = 0; w < 3; w++) by_scale[A.lut(g) ? w : 0].push_back(base + w);
    }
    for (uint32_t o = 0, cnt = 1 + rnd(4); o < cnt; o++) {
        const Lanes l = a_lanes(A);
        A.outputs.push_back(pick(0)), A.out_shift.push_back(l.shift), A.out_route.push_back(l.route);
    }
    for (uint32_t i = 0; i < n_regs; i++) {
        const Lanes l = a_lanes(A);
        A.next_ref.push_back(pick(0)), A.next_shift.push_back(l.shift), A.next_route.push_back(l.route), A.reg_scale.push_back(0);
    }
    A.ref.push_back(0), A.shift.push_back(0), A.term_route.push_back(0), A.weight.push_back(1);   // (never an empty array)
    A.next_ref.push_back(0), A.next_shift.push_back(0), A.next_route.push_back(0), A.reg_scale.push_back(0);
    A.routes.push_back(0);
    return A;
}

// the caller's arrays in clear, one wire and one instance at a time: val [wire][instance]
static std::vector<uint8_t> scalar_bits(const Arrays &A, const std::vector<uint8_t> &in_bits, const std::vector<uint8_t> &data,
                                        size_t instances) {
    const size_t n_wires = A.n_inputs + 3 * A.n_gates();
    const uint32_t G = A.group;
    std::vector<uint8_t> val(n_wires * instances, 0);
    for (size_t i = 0; i < (size_t)A.n_inputs * instances; i++) val[i] = in_bits[i] & 1u;
    auto read = [&](size_t i, size_t t) -> uint32_t {
        const uint32_t id = A.ref[i] & ~CIRC_NOT;
        uint32_t v = 0;
        if (id != CIRC_FALSE) {
            const int64_t own = (int64_t)(t % G);
            const int64_t lane = A.term_route[i] ? A.routes[(size_t)(A.term_route[i] - 1) * G + (size_t)own] : own + A.shift[i];
            if (lane >= 0 && lane < (int64_t)G) v = val[(size_t)id * instances + (size_t)((int64_t)t - own + lane)];
        }
        return A.ref[i] & CIRC_NOT ? v ^ 1u : v;
    };
    size_t leader = 0;
    for (size_t g = 0; g < A.n_gates(); g++) {
        uint8_t *o = val.data() + ((size_t)A.n_inputs + 3 * g) * instances;
        if (!A.sibling(g)) leader = g;
        const size_t t0 = A.start[leader], cnt = A.start[leader + 1] - t0;
        for (size_t t = 0; t < instances; t++) {
            uint32_t w[3];
            if (A.lut(g)) {
                const uint32_t idx = read(t0, t) + 2 * read(t0 + 1, t) + 4 * read(t0 + 2, t);
                const uint32_t tab = A.data(g) ? data[(size_t)A.table[g] * instances + t] : A.table[g];
                w[0] = w[1] = w[2] = (tab >> idx) & 1u;
            } else if (A.kind[g] == 1) {
                int32_t s = 0;
                for (size_t i = 0; i < cnt; i++) s += A.weight[t0 + i] * (int32_t)read(t0 + i, t);
                const uint32_t m = (uint32_t)(s & 3);
                w[0] = m >= 2, w[1] = m == 1 || m == 2, w[2] = m & 1u;
            } else {
                const uint32_t x = read(t0, t), y = read(t0 + 1, t);
                w[0] = x & y, w[1] = x | y, w[2] = x ^ y;
            }
            for (uint32_t k = 0; k < 3; k++) o[k * instances + t] = (uint8_t)w[k];
        }
    }
    return val;
}

static void check_bits(const Arrays &A, const CircuitPlan &P, size_t instances) {
    std::vector<uint8_t> in_bits((size_t)A.n_inputs * instances + 1), data((size_t)A.n_planes * instances + 1);
    for (auto &b : in_bits) b = (uint8_t)rnd(256);   // (only bit 0 counts)
    for (auto &b : data) b = (uint8_t)rnd(256);
    std::vector<uint64_t> table;
    CHECK(circuit_plain_bits(P, in_bits.data(), instances, table, data.data()) == SGFHE_OK);
    const std::vector<uint8_t> val = scalar_bits(A, in_bits, data, instances);
    const size_t wpr = circuit_bit_words(instances);
    CHECK(table.size() == circuit_probe_rows(P) * wpr);
    for (size_t row = 0; row < circuit_probe_rows(P); row++) {
        const size_t wire = circuit_probe_wire(P, row);
        for (size_t t = 0; t < instances; t++)
            CHECK(((table[row * wpr + t / 64] >> (t % 64)) & 1ull) == val[wire * instances + t]);
        g_compared += instances;
    }
}

static void routes_are_seen_by_nothing_else(const Arrays &A, uint64_t instances) {
    CircuitPlan P, Z;
    CHECK(A.plan(P) == SGFHE_OK && A.plan_seq(Z) == SGFHE_OK);
    CHECK(P.n_routes == A.n_routes && Z.n_routes == 0 && P.levels == Z.levels && P.widest == Z.widest && P.slots == Z.slots);
    same(P.level, Z.level), same(P.order, Z.order), same(P.level_start, Z.level_start), same(P.input_slot, Z.input_slot);
    same(P.node_kind, Z.node_kind), same(P.term_start, Z.term_start), same(P.term_ref, Z.term_ref);
    same(P.term_shift, Z.term_shift), same(P.term_weight, Z.term_weight), same(P.out_slot, Z.out_slot);
    same(P.out_ref, Z.out_ref), same(P.out_shift, Z.out_shift), same(P.term_row, Z.term_row);
    same(P.sum_before, Z.sum_before), same(P.lut_before, Z.lut_before), same(P.fam_start, Z.fam_start);
    same(P.fam_entry, Z.fam_entry), same(P.fam_node, Z.fam_node), same(P.next_ref, Z.next_ref);
    same(P.next_shift, Z.next_shift), same(P.reg_scale, Z.reg_scale), same(P.reg_index, Z.reg_index);
    CHECK(Z.routes.empty() && Z.term_route.empty() && Z.out_route.empty() && Z.next_route.empty());
    CHECK(Z.at.routes == 0 && Z.at.term_route == 0 && Z.at.out_route == 0 && Z.at.next_route == 0);
    check_bits(A, P, (size_t)instances);
    if (!A.n_routes) {
        same(P.image, Z.image), same(P.out_node, Z.out_node), same(P.jobs, Z.jobs);
        return;
    }
    // the tables and the indices are the caller's; a route on the constant is dropped; a routed reference has shift 0
    const uint32_t G = A.group;
    CHECK(P.routes.size() == (size_t)A.n_routes * G);
    for (size_t i = 0; i < P.routes.size(); i++) CHECK(P.routes[i] == A.routes[i]);
    auto kept = [&](uint32_t ref, uint32_t route) { return (ref & ~CIRC_NOT) == CIRC_FALSE ? 0u : route; };
    size_t at = 0;
    for (size_t k = 0; k < P.live(); k++) {
        const size_t g = P.order[k];
        for (size_t i = A.start[g]; i < A.start[g + 1]; i++, at++) {
            CHECK(P.term_route[at] == kept(A.ref[i], A.term_route[i]));
            CHECK(!P.term_route[at] || P.term_shift[at] == 0);
        }
    }
    CHECK(P.term_route.size() == P.term_ref.size() && at + 2 * (size_t)P.n_outputs == P.term_route.size());
    for (size_t o = 0; o < P.n_outputs; o++) {
        const uint32_t want = kept(A.outputs[o], A.out_route[o]);
        CHECK(P.out_route[o] == want && P.term_route[at + 2 * o] == 0 && P.term_route[at + 2 * o + 1] == want);
        if (want) CHECK(P.out_node[o] == CIRC_NONE);           // refreshed or lifted, never direct
        else CHECK(P.out_node[o] == Z.out_node[o]);
    }
    for (size_t i = 0; i < P.n_regs; i++) CHECK(P.next_route[i] == kept(A.next_ref[i], A.next_route[i]));
    g_compared += P.term_route.size() + P.n_outputs + P.n_regs;
    // the image: the route-free plan's tables word for word up to the jobs (a routed output drops a job), the four route
    // tables behind everything
    CHECK(P.at.jobs == Z.at.jobs);
    for (uint32_t i = 0; i < P.at.jobs; i++) CHECK(P.image[i] == Z.image[i]);
    CHECK(P.at.words == P.image.size());
    const uint32_t tail = P.n_regs ? P.at.next_route + P.n_regs : P.at.out_route + P.n_outputs;
    CHECK(tail == P.at.words && P.at.routes < P.at.term_route && P.at.term_route < P.at.out_route);
    CHECK(P.at.routes >= (P.n_regs ? P.at.reg_index + P.n_regs : P.at.jobs + (uint32_t)P.jobs.size()));
    CHECK(P.at.term_route == P.at.routes + P.routes.size() && P.at.out_route == P.at.term_route + P.term_route.size());
    for (size_t i = 0; i < P.routes.size(); i++) CHECK(P.image[P.at.routes + i] == (uint32_t)P.routes[i]);
    for (size_t i = 0; i < P.term_route.size(); i++) CHECK(P.image[P.at.term_route + i] == P.term_route[i]);
    for (size_t o = 0; o < P.n_outputs; o++) CHECK(P.image[P.at.out_route + o] == P.out_route[o]);
    for (size_t i = 0; i < P.n_regs; i++) CHECK(P.image[P.at.next_route + i] == P.next_route[i]);
    g_compared += P.at.words;
    // the call arithmetic but for the jobs
    for (uint32_t L = 1; L <= P.levels; L++)
        for (uint64_t row0 = 0; row0 < P.level_rows(L, instances); row0 += SGFHE_CIRCUIT_CALL_ROWS) {
            const CircuitCall a = circuit_level_call(P, L, row0, instances), b = circuit_level_call(Z, L, row0, instances);
            CHECK(a.k0 == b.k0 && a.rows == b.rows && a.ka == b.ka && a.kb == b.kb && a.sum == b.sum && a.lut == b.lut &&
                  a.fam == b.fam);
            g_compared += 7;
        }
}

// every index array NULL or zero, tables unused: the sgfhe_circuit_create_seq plan
static void no_routes_is_the_seq_plan(const Arrays &A0) {
    Arrays A = A0;
    A.n_routes = 0;
    for (auto *v : {&A.term_route, &A.out_route, &A.next_route}) std::fill(v->begin(), v->end(), 0u);
    CircuitPlan P, N, Z;
    CHECK(A.plan(P) == SGFHE_OK && A.plan_seq(Z) == SGFHE_OK);
    CircuitSpec S = A.spec();
    S.routes = CircuitRoutes();   // n_routes 0 and every array NULL
    CHECK(circuit_plan(S, N) == SGFHE_OK);
    for (const CircuitPlan *Q : {&P, &N}) {
        CHECK(Q->n_routes == 0 && Q->levels == Z.levels && Q->slots == Z.slots && Q->n_regs == Z.n_regs);
        same(Q->image, Z.image), same(Q->order, Z.order), same(Q->out_node, Z.out_node), same(Q->jobs, Z.jobs);
        same(Q->term_shift, Z.term_shift), same(Q->next_shift, Z.next_shift), same(Q->out_shift, Z.out_shift);
        CHECK(Q->routes.empty() && Q->term_route.empty() && Q->out_route.empty() && Q->next_route.empty());
        CHECK(Q->at.words == Z.at.words && Q->at.routes == 0 && Q->at.term_route == 0 && Q->at.out_route == 0 &&
              Q->at.next_route == 0);
    }
}

// 2 inputs, group 4; node 0 = classic (input 0, input 1): wires 2, 3, 4; node 1 = classic (wire 2, input 0): wires 5, 6, 7;
// one register would be input 0
static Arrays small() {
    Arrays A;
    A.n_inputs = 2, A.group = 4;
    A.kind = {0, 0}, A.table = {0, 0}, A.start = {0, 2, 4};
    A.ref = {0, 1, 2, 0}, A.shift = {0, 0, 0, 0}, A.weight = {1, 1, 1, 1}, A.term_route = {1, 0, 2, 0};
    A.outputs = {5, 4}, A.out_shift = {0, 0}, A.out_route = {0, 1};
    A.next_ref = {0}, A.next_shift = {0}, A.next_route = {0}, A.reg_scale = {0};
    A.n_routes = 2, A.routes = {3, 2, 1, 0, -1, 0, 0, 2};
    return A;
}

static void shifts_spelled_as_routes() {
    // every reference of small() shifted by d, against the same circuit with the table of that shift
    for (int32_t d = -3; d <= 3; d++) {
        Arrays S = small(), R = small();
        S.n_routes = 0, S.routes = {0}, S.term_route = {0, 0, 0, 0}, S.out_route = {0, 0};
        S.shift = {d, 0, d, -d}, S.out_shift = {d, 0};
        R.n_routes = 2, R.routes.clear();
        for (int32_t s : {d, -d})
            for (int32_t t = 0; t < 4; t++) R.routes.push_back(t + s >= 0 && t + s < 4 ? t + s : -1);
        R.term_route = {1, 0, 1, 2}, R.out_route = {1, 0};
        CircuitPlan PS, PR;
        CHECK(S.plan(PS) == SGFHE_OK && R.plan(PR) == SGFHE_OK);
        std::vector<uint8_t> bits(2 * 24);
        for (auto &b : bits) b = (uint8_t)rnd(2);
        std::vector<uint64_t> ts, tr;
        CHECK(circuit_plain_bits(PS, bits.data(), 24, ts) == SGFHE_OK && circuit_plain_bits(PR, bits.data(), 24, tr) == SGFHE_OK);
        same(ts, tr);
    }
}

static void refused(const Arrays &A, int line) {
    CircuitPlan P;
    P.slots = 77, P.n_routes = 5;   // (a plan the refusal must leave as it is)
    const size_t before = g_allocs;
    const int32_t rc = A.plan(P);
    if (rc != SGFHE_ERR_INVALID_ARG || g_allocs != before || P.slots != 77 || P.n_routes != 5) {
        fprintf(stderr, "case at line %d: rc %d, %zu allocations\n", line, rc, g_allocs - before);
        abort();
    }
    g_compared++;
}
#define REFUSED(A) refused(A, __LINE__)

int main() {
    static const uint32_t shapes[][2] = {{8, 72}, {24, 120}, {1, 5}};
    for (const auto &sh : shapes)
        for (int rep = 0; rep < 60; rep++) {
            const uint32_t n_inputs = 1 + rnd(6), n_regs = rnd(2) ? rnd(n_inputs + 1) : 0;
            const Arrays A = random_circuit(n_inputs, n_regs, 1 + rnd(16), sh[0], rnd(2) ? 1 + rnd(3) : 0);
            routes_are_seen_by_nothing_else(A, sh[1]);
            no_routes_is_the_seq_plan(A);
        }
    shifts_spelled_as_routes();
    {   // the small plan: accepted, its routed output refreshed, an unused table allowed, the largest entries
        Arrays A = small();
        CircuitPlan P;
        CHECK(A.plan(P) == SGFHE_OK && P.n_routes == 2 && P.out_node[0] != CIRC_NONE && P.out_node[1] == CIRC_NONE);
        A.term_route = {0, 0, 0, 0}, A.out_route = {0, 0};
        CHECK(A.plan(P) == SGFHE_OK && P.n_routes == 2 && P.out_node[1] != CIRC_NONE);   // tables nothing uses
        A = small(), A.out_route = {0, 1}, A.routes = {0, 1, 2, 3, 0, 1, 2, 3};
        CHECK(A.plan(P) == SGFHE_OK && P.out_node[1] == CIRC_NONE);   // the identity table is still a route
        A = small(), A.outputs[1] = CIRC_FALSE | CIRC_NOT, A.out_shift[1] = 0;
        CHECK(A.plan(P) == SGFHE_OK && P.out_route[1] == 0);   // dropped on the constant
        A = small(), A.n_regs = 1, A.next_ref = {5}, A.next_route = {2};
        CHECK(A.plan(P) == SGFHE_OK && P.next_route[0] == 2 && P.image[P.at.next_route] == 2);
    }
    {   // ---- refused
        Arrays B = small();
        B.routes[2] = 4;
        REFUSED(B);     // an entry at G
        B = small(), B.routes[5] = -2;
        REFUSED(B);     // an entry below the fill
        B = small(), B.routes[0] = INT32_MIN;
        REFUSED(B);
        B = small(), B.routes[7] = INT32_MAX;
        REFUSED(B);
        B = small(), B.term_route[1] = 3;
        REFUSED(B);     // an index above n_routes
        B = small(), B.out_route[0] = 3;
        REFUSED(B);
        B = small(), B.out_route[0] = 0xFFFFFFFFu;
        REFUSED(B);
        B = small(), B.n_regs = 1, B.next_route = {3};
        REFUSED(B);
        B = small(), B.shift[0] = 1;
        REFUSED(B);     // a route beside a shift
        B = small(), B.out_shift[1] = -1;
        REFUSED(B);
        B = small(), B.n_regs = 1, B.next_route = {1}, B.next_shift = {2};
        REFUSED(B);
        B = small(), B.n_routes = 0;
        REFUSED(B);     // indices 1 and 2 with no table at all
        B = small(), B.n_routes = SGFHE_CIRCUIT_MAX_ROUTES + 1;
        REFUSED(B);     // (refused before a table is read)
        B = small(), B.shift[1] = 4;
        REFUSED(B);     // what sgfhe_circuit_create_seq refuses stays refused
        {
            const Arrays A = small();
            CircuitPlan P;
            P.slots = 77;
            CircuitSpec S = A.spec();
            S.nodes.n_planes = 0, S.regs = CircuitRegs();
            S.routes.n_routes = 2, S.routes.routes = nullptr, S.routes.next_route = nullptr;
            const size_t before = g_allocs;
            CHECK(circuit_plan(S, P) == SGFHE_ERR_INVALID_ARG);   // NULL routes
            CHECK(g_allocs == before && P.slots == 77);
        }
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
