// Lane masks of csrc/circuit.h (sgfhe_circuit_create_masked) under AddressSanitizer and UndefinedBehaviorSanitizer on the
// CPU (tests/test_circuit_masks_host.py).  A stand-alone program, no input:
//   - random circuits in the CSR form with every node kind (classic, sum, LUT, sibling, data LUT, data sibling; NOTs,
//     constants, registers, lane shifts and routes on references) whose nodes carry a random lane mask or none are
//     planned at (G, instances) = (8, 72), (24, 120), (2, 6): everything that must not see masks -- levels, order,
//     slots, the node table, the routes' and registers' tables -- is that of the plan of the same arrays without
//     masks; an output naming a masked node's wire has no out_node, every other output the out_node it had; the pair
//     tables and the off pairs are restated from the caller's masks, the image carries the four tables behind every
//     other table, and rows_per_group is the sum of the lanes set;
//   - the call arithmetic restated row by row: level_rows, and k0 / rows / ka / kb / sum / lut / fam / jobs of every call
//     of every level from a row-by-row list of (node, instance); on the random plans, and on one level of five nodes with
//     8, 3, 5, 8, 1 lanes set over 3200 instances (row 8192 inside the fourth node's pairs) and one whose boundary
//     falls between two nodes (8, 8 lanes over 8192 instances);
//   - circuit_plain_bits of the masked plan against a scalar evaluation of the caller's arrays, wire by wire and
//     instance by instance;
//   - with n_masks = 0 (NULL or all-zero node_mask, unused tables aside) the plan is the sgfhe_circuit_create_routed
//     plan field for field and its image word for word;
//   - the inputs the planner must refuse -- an entry other than 0 or 1, a table with no lane set, an index above
//     n_masks, n_masks > 0 with NULL masks, n_masks above SGFHE_CIRCUIT_MAX_MASKS, a mask on a sibling, what the routed
//     creator refuses -- return SGFHE_ERR_INVALID_ARG without a single allocation (the global operator new is counted, in
//     the build without sanitizers) and leave the plan they were given untouched; a masked LUT node that leads a live
//     sibling is refused after pruning (the plan is reset), and accepted where the sibling is dead.
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
    uint32_t n_inputs = 0, group = 1, n_planes = 0, n_regs = 0, n_routes = 0, n_masks = 0;
    std::vector<uint32_t> kind, start, ref, table, outputs, next_ref, reg_scale, term_route, out_route, next_route, node_mask;
    std::vector<int32_t> shift, weight, out_shift, next_shift, routes;
    std::vector<uint8_t> masks;
    size_t n_gates() const { return kind.size(); }
    // what sgfhe_circuit_create_routed fills, then (spec) the masks of sgfhe_circuit_create_masked
    CircuitSpec spec_routed() const {
        CircuitSpec S = spec_csr(5, n_inputs, n_planes, kind.data(), start.data(), ref.data(), shift.data(), weight.data(),
                                 table.data(), n_gates(), outputs.data(), out_shift.data(), outputs.size(), group);
        S.regs.n_regs = n_regs, S.regs.next_ref = next_ref.data();
        S.regs.next_shift = next_shift.data(), S.regs.reg_scale = reg_scale.data();
        S.routes.n_routes = n_routes, S.routes.routes = routes.data(), S.routes.term_route = term_route.data();
        S.routes.out_route = out_route.data(), S.routes.next_route = next_route.data();
        return S;
    }
    CircuitSpec spec() const {
        CircuitSpec S = spec_routed();
        S.masks.n_masks = n_masks, S.masks.masks = masks.data(), S.masks.node_mask = node_mask.data();
        return S;
    }
    int32_t plan(CircuitPlan &P) const { return circuit_plan(spec(), P); }
    int32_t plan_routed(CircuitPlan &P) const { return circuit_plan(spec_routed(), P); }
    bool lut(size_t g) const { return kind[g] >= 2; }
    bool sibling(size_t g) const { return kind[g] == 3 || kind[g] == 5; }
    bool data(size_t g) const { return kind[g] >= 4; }
    // node g takes a row at lane l
    bool on(size_t g, uint32_t l) const { return !node_mask[g] || masks[(size_t)(node_mask[g] - 1) * group + l] != 0; }
};

struct Lanes {
    int32_t shift;
    uint32_t route;
};
static Lanes a_lanes(Arrays &A) {
    const uint32_t G = A.group, what = rnd(3);
    if (what == 0) return {0, 0};
    if (what == 1) return {G > 1 ? (int32_t)rnd(2 * G - 1) - (int32_t)(G - 1) : 0, 0};
    if (A.n_routes == 0 || rnd(3) == 0) {
        const uint32_t form = rnd(3), d = rnd(G), lane = rnd(G);
        for (uint32_t t = 0; t < G; t++)
            A.routes.push_back(form == 0 ? (int32_t)rnd(G + 1) - 1 : form == 1 ? (int32_t)((t + d) % G) : (int32_t)lane);
        A.n_routes++;
    }
    return {0, 1 + rnd(A.n_routes)};
}
// a mask index for the node being made: none, a table made so far, or a new one (one lane, all but one, alternating,
// random with a lane forced on)
static uint32_t a_mask(Arrays &A) {
    const uint32_t G = A.group;
    if (rnd(3) == 0) return 0;
    if (A.n_masks == 0 || rnd(3) == 0) {
        const uint32_t form = rnd(4), lane = rnd(G);
        for (uint32_t t = 0; t < G; t++)
            A.masks.push_back(form == 0 ? t == lane : form == 1 ? t != lane || G == 1 : form == 2 ? (t & 1u) == (lane & 1u)
                                                                                                  : (t == lane || rnd(2)));
        A.n_masks++;
    }
    return 1 + rnd(A.n_masks);
}

// A random circuit that obeys the scale rule, every register of scale 0; no masked LUT node is given a sibling
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
    size_t leader = 0;
    for (size_t g = 0; g < n_nodes; g++) {
        const uint32_t what = rnd(5);
        const bool prev_lut = g > 0 && A.lut(g - 1);
        if (what == 0) {
            A.kind.push_back(0), A.table.push_back(0), A.node_mask.push_back(a_mask(A));
            term(pick(0), 1), term(pick(0), 1);
        } else if (what == 1) {
            A.kind.push_back(1), A.table.push_back(0), A.node_mask.push_back(a_mask(A));
            static const int32_t W[4] = {-2, -1, 1, 2};
            for (uint32_t i = 0, cnt = 1 + rnd(5); i < cnt; i++) term(pick(0), W[rnd(4)]);
        } else if (what == 2 && prev_lut && !A.node_mask[leader]) {   // a sibling of the (unmasked) family in front of it
            const bool dat = n_planes && rnd(2);
            A.kind.push_back(dat ? 5 : 3), A.table.push_back(dat ? rnd(n_planes) : rnd(256)), A.node_mask.push_back(0);
        } else {
            const bool dat = n_planes && rnd(2);
            A.kind.push_back(dat ? 4 : 2), A.table.push_back(dat ? rnd(n_planes) : rnd(256)), A.node_mask.push_back(a_mask(A));
            term(pick(2), 1), term(pick(1), 1), term(pick(0), 1);
        }
        if (!A.sibling(g)) leader = g;
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
    A.routes.push_back(0), A.masks.push_back(1), A.node_mask.push_back(0);
    return A;
}

// the caller's arrays in clear, one wire and one instance at a time: val [wire][instance]; a masked node's wires are 0
// on its off lanes
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
            if (!A.on(g, (uint32_t)(t % G))) {
                w[0] = w[1] = w[2] = 0;
            } else if (A.lut(g)) {
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

// The rows of every level of a masked plan, one by one, from the caller's masks: row R of level L is (node k of `order`,
// instance t).  Then every call of the level against that list.
struct Row {
    uint32_t k, t;
};
static std::vector<Row> level_rows_restated(const Arrays &A, const CircuitPlan &P, uint32_t L, uint64_t instances) {
    const uint32_t G = A.group;
    const uint64_t per = instances / G;
    std::vector<Row> rows;
    for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++)
        for (uint32_t l = 0; l < G; l++) {
            if (!A.on(P.order[k], l)) continue;
            for (uint64_t grp = 0; grp < per; grp++) rows.push_back({k, (uint32_t)(grp * G + l)});
        }
    return rows;
}
static void check_calls(const Arrays &A, const CircuitPlan &P, uint64_t instances) {
    CHECK(P.masked());
    const uint64_t per = instances / A.group;
    uint64_t rows_per_group = 0;
    for (uint32_t L = 1; L <= P.levels; L++) {
        const std::vector<Row> rows = level_rows_restated(A, P, L, instances);
        CHECK(P.level_rows(L, instances) == rows.size());
        rows_per_group += rows.size() / per;
        // the pair tables say the same, pair by pair; the off pairs are the rest of the masked nodes' lanes
        const uint32_t p0 = P.pair_start[L];
        CHECK(rows.size() == (uint64_t)(P.pair_start[L + 1] - p0) * per);
        for (size_t R = 0; R < rows.size(); R++) {
            const uint32_t p = p0 + (uint32_t)(R / per);
            CHECK(P.level_start[L] + P.pair_node[p] == rows[R].k);
            CHECK((R % per) * A.group + P.pair_lane[p] == rows[R].t);
        }
        uint32_t off = P.off_start[L];
        for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++)
            for (uint32_t l = 0; l < A.group; l++) {
                if (A.on(P.order[k], l)) continue;
                CHECK(off < P.off_start[L + 1] && P.off_node[off] == k - P.level_start[L] && P.off_lane[off] == l);
                off++;
            }
        CHECK(off == P.off_start[L + 1]);
        g_compared += rows.size();
        for (uint64_t row0 = 0; row0 < rows.size(); row0 += SGFHE_CIRCUIT_CALL_ROWS) {
            const CircuitCall C = circuit_level_call(P, L, row0, instances);
            const uint64_t end = std::min<uint64_t>(rows.size(), row0 + SGFHE_CIRCUIT_CALL_ROWS);
            CHECK(C.k0 == P.level_start[L] && C.rows == end - row0 && C.ka == rows[row0].k && C.kb == rows[end - 1].k);
            bool sum = false, lut = false, fam = false;
            size_t jobs = 0;
            for (uint32_t k = C.ka; k <= C.kb; k++) {
                sum = sum || P.kind(k) == 1, lut = lut || P.kind(k) == 2;
                fam = fam || (P.siblings() && P.fam_start[k + 1] != P.fam_start[k]);
                for (uint32_t jk : P.job_k) jobs += jk == k;
            }
            CHECK(C.sum == sum && C.lut == lut && C.fam == fam && C.j1 - C.j0 == jobs);
            for (size_t j = C.j0; j < C.j1; j++) CHECK(P.job_k[j] >= C.ka && P.job_k[j] <= C.kb);
            g_compared += 8;
        }
    }
    CHECK(P.rows_per_group == rows_per_group);
    const CircuitRunSizes sz = circuit_run_sizes(P, instances, 16, 0, false, false, false);
    uint64_t max_rows = 0;
    for (uint32_t L = 1; L <= P.levels; L++)
        max_rows = std::max(max_rows, std::min<uint64_t>(P.level_rows(L, instances), SGFHE_CIRCUIT_CALL_ROWS));
    CHECK(sz.max_rows == max_rows && sz.work_rows == max_rows);
}

static void masks_are_seen_by_nothing_else(const Arrays &A, uint64_t instances) {
    CircuitPlan P, Z;
    CHECK(A.plan(P) == SGFHE_OK && A.plan_routed(Z) == SGFHE_OK);
    CHECK(P.n_masks == A.n_masks && Z.n_masks == 0 && !Z.masked() && P.levels == Z.levels && P.widest == Z.widest &&
          P.slots == Z.slots && P.n_routes == Z.n_routes);
    same(P.level, Z.level), same(P.order, Z.order), same(P.level_start, Z.level_start), same(P.input_slot, Z.input_slot);
    same(P.node_kind, Z.node_kind), same(P.term_start, Z.term_start), same(P.term_ref, Z.term_ref);
    same(P.term_shift, Z.term_shift), same(P.term_weight, Z.term_weight), same(P.out_slot, Z.out_slot);
    same(P.out_ref, Z.out_ref), same(P.out_shift, Z.out_shift), same(P.term_row, Z.term_row);
    same(P.sum_before, Z.sum_before), same(P.lut_before, Z.lut_before), same(P.fam_start, Z.fam_start);
    same(P.fam_entry, Z.fam_entry), same(P.fam_node, Z.fam_node), same(P.next_ref, Z.next_ref);
    same(P.next_shift, Z.next_shift), same(P.reg_scale, Z.reg_scale), same(P.reg_index, Z.reg_index);
    same(P.routes, Z.routes), same(P.term_route, Z.term_route), same(P.out_route, Z.out_route), same(P.next_route, Z.next_route);
    CHECK(Z.masks.empty() && Z.node_mask.empty() && Z.pair_start.empty() && Z.pair_node.empty() && Z.pair_lane.empty() &&
          Z.off_start.empty() && Z.off_node.empty() && Z.off_lane.empty());
    CHECK(Z.at.pair_node == 0 && Z.at.pair_lane == 0 && Z.at.off_node == 0 && Z.at.off_lane == 0);
    CHECK(Z.rows_per_group == (uint64_t)Z.live() * Z.group);
    check_bits(A, P, (size_t)instances);
    if (!A.n_masks) {
        same(P.image, Z.image), same(P.out_node, Z.out_node), same(P.jobs, Z.jobs);
        CHECK(P.rows_per_group == Z.rows_per_group);
        return;
    }
    // the tables and the indices are the caller's
    CHECK(P.masks.size() == (size_t)A.n_masks * A.group && P.node_mask.size() == P.live());
    for (size_t i = 0; i < P.masks.size(); i++) CHECK(P.masks[i] == A.masks[i]);
    for (size_t k = 0; k < P.live(); k++) CHECK(P.node_mask[k] == A.node_mask[P.order[k]]);
    // an output naming a masked node's wire is no gate row; every other output is what it was
    for (size_t o = 0; o < P.n_outputs; o++) {
        const uint32_t id = A.outputs[o] & ~CIRC_NOT;
        const bool masked = id != CIRC_FALSE && id >= A.n_inputs && A.node_mask[(id - A.n_inputs) / 3];
        if (masked) CHECK(P.out_node[o] == CIRC_NONE);
        else CHECK(P.out_node[o] == Z.out_node[o] && P.out_gate[o] == Z.out_gate[o]);
    }
    g_compared += P.masks.size() + P.live() + P.n_outputs;
    // the image: the mask-free plan's tables word for word up to the jobs (a masked output drops a job), the four pair
    // tables behind everything
    CHECK(P.at.jobs == Z.at.jobs);
    for (uint32_t i = 0; i < P.at.jobs; i++) CHECK(P.image[i] == Z.image[i]);
    CHECK(P.at.words == P.image.size() && P.at.off_lane + P.off_lane.size() == P.at.words);
    CHECK(P.at.pair_lane == P.at.pair_node + P.pair_node.size() && P.at.off_node == P.at.pair_lane + P.pair_lane.size() &&
          P.at.off_lane == P.at.off_node + P.off_node.size());
    const uint32_t before = P.n_routes ? (P.n_regs ? P.at.next_route + P.n_regs : P.at.out_route + P.n_outputs)
                                       : (P.n_regs ? P.at.reg_index + P.n_regs
                                                   : P.siblings() ? P.at.fam_entry + (uint32_t)P.fam_entry.size()
                                                                  : P.at.jobs + (uint32_t)P.jobs.size());
    CHECK(P.at.pair_node == before);
    for (size_t i = 0; i < P.pair_node.size(); i++)
        CHECK(P.image[P.at.pair_node + i] == P.pair_node[i] && P.image[P.at.pair_lane + i] == P.pair_lane[i]);
    for (size_t i = 0; i < P.off_node.size(); i++)
        CHECK(P.image[P.at.off_node + i] == P.off_node[i] && P.image[P.at.off_lane + i] == P.off_lane[i]);
    CHECK(P.pair_node.size() + P.off_node.size() == P.live() * (size_t)A.group);
    g_compared += P.at.words;
    check_calls(A, P, instances);
}

// node_mask NULL or zero, tables unused: the sgfhe_circuit_create_routed plan
static void no_masks_is_the_routed_plan(const Arrays &A0) {
    Arrays A = A0;
    std::fill(A.node_mask.begin(), A.node_mask.end(), 0u);
    CircuitPlan U, P, N, Z;
    CHECK(A.plan(U) == SGFHE_OK && A.plan_routed(Z) == SGFHE_OK);   // tables nothing uses: a masked plan all the same
    CHECK(U.n_masks == A0.n_masks && U.rows_per_group == Z.rows_per_group && same_tables(U, Z) == (!A0.n_masks || !U.live()));
    A.n_masks = 0;
    CHECK(A.plan(P) == SGFHE_OK);
    CircuitSpec S = A.spec();
    S.masks = CircuitMasks();   // n_masks 0 and every array NULL
    CHECK(circuit_plan(S, N) == SGFHE_OK);
    for (const CircuitPlan *Q : {&P, &N}) {
        CHECK(same_tables(*Q, Z) && Q->n_masks == 0 && Q->n_regs == Z.n_regs && Q->n_routes == Z.n_routes);
        same(Q->image, Z.image), same(Q->routes, Z.routes), same(Q->term_route, Z.term_route), same(Q->next_ref, Z.next_ref);
        same(Q->fam_start, Z.fam_start), same(Q->fam_entry, Z.fam_entry), same(Q->lut_before, Z.lut_before);
        CHECK(Q->masks.empty() && Q->node_mask.empty() && Q->pair_start.empty() && Q->pair_node.empty() && Q->off_node.empty());
        CHECK(Q->at.words == Z.at.words && Q->at.pair_node == 0 && Q->at.pair_lane == 0 && Q->at.off_node == 0 &&
              Q->at.off_lane == 0 && Q->rows_per_group == Z.rows_per_group);
        for (uint32_t L = 1; L <= Z.levels; L++) {
            CHECK(Q->level_rows(L, 48) == Z.level_rows(L, 48));
            const CircuitCall a = circuit_level_call(*Q, L, 0, 48), b = circuit_level_call(Z, L, 0, 48);
            CHECK(a.k0 == b.k0 && a.rows == b.rows && a.ka == b.ka && a.kb == b.kb && a.j0 == b.j0 && a.j1 == b.j1);
        }
    }
}

// `lanes` [nodes]: one level of classic nodes on two inputs, group 8, node i with its first lanes[i] lanes set
static Arrays one_level(const std::vector<uint32_t> &lanes) {
    Arrays A;
    A.n_inputs = 2, A.group = 8;
    A.start.push_back(0);
    for (size_t g = 0; g < lanes.size(); g++) {
        A.kind.push_back(0), A.table.push_back(0);
        A.ref.push_back(0), A.ref.push_back(1 | (g & 1 ? CIRC_NOT : 0u));
        A.start.push_back((uint32_t)A.ref.size());
        A.outputs.push_back(2 + 3 * (uint32_t)g + (uint32_t)(g % 3));
        if (lanes[g] == 8) {
            A.node_mask.push_back(0);
            continue;
        }
        for (uint32_t t = 0; t < 8; t++) A.masks.push_back(t < lanes[g]);
        A.node_mask.push_back(++A.n_masks);
    }
    A.shift.assign(A.ref.size(), 0), A.weight.assign(A.ref.size(), 1), A.term_route.assign(A.ref.size(), 0);
    A.out_shift.assign(A.outputs.size(), 0), A.out_route.assign(A.outputs.size(), 0);
    A.next_ref = {0}, A.next_shift = {0}, A.next_route = {0}, A.reg_scale = {0}, A.routes = {0};
    A.masks.push_back(1), A.node_mask.push_back(0);
    return A;
}

// 2 inputs, group 4; node 0 = classic (input 0, input 1), lanes 0 and 2; node 1 = classic (wire 2, input 0), every lane
static Arrays small() {
    Arrays A;
    A.n_inputs = 2, A.group = 4;
    A.kind = {0, 0}, A.table = {0, 0}, A.start = {0, 2, 4};
    A.ref = {0, 1, 2, 0}, A.shift = {0, 0, 1, 0}, A.weight = {1, 1, 1, 1}, A.term_route = {0, 0, 0, 0};
    A.outputs = {5, 4}, A.out_shift = {0, 0}, A.out_route = {0, 0};
    A.next_ref = {0}, A.next_shift = {0}, A.next_route = {0}, A.reg_scale = {0}, A.routes = {0};
    A.n_masks = 2, A.masks = {1, 0, 1, 0, 0, 0, 0, 1}, A.node_mask = {1, 0};
    return A;
}

// a LUT family: inputs 0 .. 2 fanned (nodes 0, 1, 2), node 3 the leader on them, node 4 its sibling, group 4
static Arrays family(uint32_t leader_mask, bool sibling_live) {
    Arrays A;
    A.n_inputs = 3, A.group = 4;
    A.kind = {2, 2, 2, 2, 3}, A.table = {0xF0, 0xF0, 0xF0, 0x96, 0xE8}, A.start = {0, 3, 6, 9, 12, 12};
    A.ref = {CIRC_FALSE, CIRC_FALSE, 0, CIRC_FALSE, CIRC_FALSE, 1, CIRC_FALSE, CIRC_FALSE, 2, 3 + 2, 6 + 1, 9 + 0};
    A.shift.assign(12, 0), A.weight.assign(12, 1), A.term_route.assign(12, 0);
    A.outputs = {12};
    if (sibling_live) A.outputs.push_back(15);
    A.out_shift.assign(A.outputs.size(), 0), A.out_route.assign(A.outputs.size(), 0);
    A.next_ref = {0}, A.next_shift = {0}, A.next_route = {0}, A.reg_scale = {0}, A.routes = {0};
    A.n_masks = 1, A.masks = {0, 1, 1, 0}, A.node_mask = {0, 0, 1, leader_mask, 0};
    return A;
}

static void refused(const Arrays &A, int line) {
    CircuitPlan P;
    P.slots = 77, P.n_masks = 5;   // (a plan the refusal must leave as it is)
    const size_t before = g_allocs;
    const int32_t rc = A.plan(P);
    if (rc != SGFHE_ERR_INVALID_ARG || g_allocs != before || P.slots != 77 || P.n_masks != 5) {
        fprintf(stderr, "case at line %d: rc %d, %zu allocations\n", line, rc, g_allocs - before);
        abort();
    }
    g_compared++;
}
#define REFUSED(A) refused(A, __LINE__)

int main() {
    static const uint32_t shapes[][2] = {{8, 72}, {24, 120}, {2, 6}};
    for (const auto &sh : shapes)
        for (int rep = 0; rep < 60; rep++) {
            const uint32_t n_inputs = 1 + rnd(6), n_regs = rnd(2) ? rnd(n_inputs + 1) : 0;
            const Arrays A = random_circuit(n_inputs, n_regs, 1 + rnd(16), sh[0], rnd(2) ? 1 + rnd(3) : 0);
            masks_are_seen_by_nothing_else(A, sh[1]);
            no_masks_is_the_routed_plan(A);
        }
    {   // 8 + 3 + 5 + 8 + 1 = 25 pairs of 400 groups: 10000 rows, row 8192 = pair 20 = the fourth node at lane 4
        const Arrays A = one_level({8, 3, 5, 8, 1});
        CircuitPlan P;
        CHECK(A.plan(P) == SGFHE_OK && P.levels == 1 && P.rows_per_group == 25 && P.level_rows(1, 3200) == 10000);
        const CircuitCall C0 = circuit_level_call(P, 1, 0, 3200), C1 = circuit_level_call(P, 1, 8192, 3200);
        CHECK(C0.rows == 8192 && C0.ka == 0 && C0.kb == 3 && C1.rows == 1808 && C1.ka == 3 && C1.kb == 4);
        CHECK(P.pair_node[20] == 3 && P.pair_lane[20] == 4 && 20 * 400 < 8192 && 8192 < 21 * 400);
        // the outputs of the unmasked nodes 0 and 3 stay direct, the others are not
        CHECK(P.out_node[0] == 0 && P.out_node[3] == 3 && P.out_node[1] == CIRC_NONE && P.out_node[2] == CIRC_NONE &&
              P.out_node[4] == CIRC_NONE);
        CHECK(C0.j1 - C0.j0 == 2 && C1.j1 - C1.j0 == 1);   // (node 3's job belongs to both calls)
        check_calls(A, P, 3200);
        check_bits(A, P, 64);
    }
    {   // 8 + 8 pairs of 1024 groups: the boundary at row 8192 falls between the two nodes
        Arrays A = one_level({8, 8, 2});
        CircuitPlan P;
        CHECK(A.plan(P) == SGFHE_OK && P.level_rows(1, 8192) == 18 * 1024);
        const CircuitCall C0 = circuit_level_call(P, 1, 0, 8192), C1 = circuit_level_call(P, 1, 8192, 8192),
                          C2 = circuit_level_call(P, 1, 16384, 8192);
        CHECK(C0.rows == 8192 && C0.ka == 0 && C0.kb == 0 && C1.rows == 8192 && C1.ka == 1 && C1.kb == 1);
        CHECK(C2.rows == 2048 && C2.ka == 2 && C2.kb == 2);
        check_calls(A, P, 8192);
    }
    {   // the small plan, and what a mask does to its outputs
        Arrays A = small();
        CircuitPlan P;
        CHECK(A.plan(P) == SGFHE_OK && P.n_masks == 2 && P.rows_per_group == 6);
        CHECK(P.out_node[0] == 1 && P.out_node[1] == CIRC_NONE);   // node 1 unmasked: direct; node 0 masked: not
        A.node_mask = {0, 2};
        CHECK(A.plan(P) == SGFHE_OK && P.rows_per_group == 5 && P.out_node[0] == CIRC_NONE && P.out_node[1] == 0);
        A.masks = {1, 1, 1, 1, 1, 1, 1, 1};   // all lanes is still a mask to the planner (Python normalises it away)
        CHECK(A.plan(P) == SGFHE_OK && P.masked() && P.rows_per_group == 8 && P.out_node[0] == CIRC_NONE);
        // a masked LUT node: alone, and leading a sibling nothing reads
        CHECK(family(1, false).plan(P) == SGFHE_OK && P.rows_per_group == 4 + 4 + 2 + 2 && P.siblings() == 0);
        CHECK(family(0, true).plan(P) == SGFHE_OK && P.siblings() == 1 && P.masked());   // an unmasked leader may
    }
    {   // ---- refused, without an allocation
        Arrays B = small();
        B.masks[1] = 2;
        REFUSED(B);     // an entry other than 0 or 1
        B = small(), B.masks[6] = 255;
        REFUSED(B);
        B = small(), B.masks = {1, 0, 1, 0, 0, 0, 0, 0};
        REFUSED(B);     // a table with no lane set (nothing uses it)
        B = small(), B.node_mask[1] = 3;
        REFUSED(B);     // an index above n_masks
        B = small(), B.node_mask[0] = 0xFFFFFFFFu;
        REFUSED(B);
        B = small(), B.n_masks = 0;
        REFUSED(B);     // index 1 with no table at all
        B = small(), B.n_masks = SGFHE_CIRCUIT_MAX_MASKS + 1;
        REFUSED(B);     // (refused before a table is read)
        B = family(0, true), B.node_mask[4] = 1;
        REFUSED(B);     // a mask on a sibling
        B = small(), B.shift[1] = 4;
        REFUSED(B);     // what sgfhe_circuit_create_routed refuses stays refused
        B = small(), B.n_routes = 1, B.routes = {0, 1, 2, 4};
        REFUSED(B);
        {
            const Arrays A = small();
            CircuitPlan P;
            P.slots = 77;
            CircuitSpec S = A.spec();
            S.masks.masks = nullptr;
            const size_t before = g_allocs;
            CHECK(circuit_plan(S, P) == SGFHE_ERR_INVALID_ARG);   // NULL masks
            CHECK(g_allocs == before && P.slots == 77);
        }
        {   // a masked LUT node that leads a LIVE sibling: known after pruning, the plan is reset
            CircuitPlan P;
            P.slots = 77;
            CHECK(family(1, true).plan(P) == SGFHE_ERR_INVALID_ARG && P.slots == 0 && P.image.empty() && P.order.empty());
            g_compared++;
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
