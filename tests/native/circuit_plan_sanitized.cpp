// csrc/circuit.h (the planner of sgfhe_circuit_run) under AddressSanitizer and UndefinedBehaviorSanitizer
// on the CPU (tests/test_circuit_plan.py).  Over seeded random DAGs it checks, against a plain restatement
// of the rules of include/sgfhe_hip.h:
//   - pruning: the live nodes are exactly those some output reaches;
//   - levels: every live node is 1 + the largest level of its input nodes, `order` is level by level in
//     ascending index, widest is the largest level;
//   - slots: a simulated run (every call of every level gathers, then scatters) never writes a slot while
//     the wire in it is still to be read, every read finds the wire it expects, output wires survive to
//     the end, and only wires something reads have a slot;
//   - rows and calls: row = rank * instances + instance, calls of at most SGFHE_CIRCUIT_CALL_ROWS rows;
//   - tables: every live node is a classic node of the caller's two terms, and the node table, the pack stage's
//     pseudo-level, the job table and the image hold together (tests/native/circuit_tables.h);
//   - malformed circuits are refused.
// Prints a digest of all plans (the plain build must print the same).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "circuit.h"
#include "circuit_tables.h"

using namespace sgfhe;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(next_u64() % n); }

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "check failed at line %d: %s (case %d)\n", __LINE__, #cond, cs); \
            abort();                                                                         \
        }                                                                                    \
    } while (0)

static int cs = -1;

static uint32_t random_ref(uint32_t n_inputs, uint32_t before_gate) {
    const uint32_t pick = below(16);
    uint32_t id;
    if (pick == 0 || (n_inputs == 0 && before_gate == 0)) id = CIRC_FALSE;
    else if (before_gate == 0 || (n_inputs && pick < 6)) id = below(n_inputs);
    else {
        // mostly recent nodes (deep circuits), sometimes any earlier one
        const uint32_t back = pick < 12 ? below(before_gate < 8 ? before_gate : 8) : below(before_gate);
        id = n_inputs + 3 * (before_gate - 1 - back) + below(3);
    }
    return id | (below(2) ? CIRC_NOT : 0u);
}

int main() {
    uint64_t digest = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { digest = (digest ^ v) * 1099511628211ull; };
    // ---- malformed circuits
    {
        CircuitPlan P;
        const uint32_t own[2] = {2, 0}, later[4] = {0, 5, 0, 1}, past[2] = {0, 9}, notpast[2] = {0, 9u | CIRC_NOT};
        const uint32_t outs[1] = {2};
        CHECK(circuit_plan(spec_gates(2, own, 1, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(2, later, 2, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(2, past, 1, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(2, notpast, 1, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(2, nullptr, 1, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(2, past, 0, outs, 0), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(2, past, 0, nullptr, 1), P) == SGFHE_ERR_INVALID_ARG);
        const uint32_t bad_out[1] = {5};
        CHECK(circuit_plan(spec_gates(2, past, 0, bad_out, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(0x80000000u, past, 0, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
        CHECK(circuit_plan(spec_gates(0x7FFFFFF0u, past, 10, outs, 1), P) == SGFHE_ERR_INVALID_ARG);
    }
    for (cs = 0; cs < 3000; cs++) {
        const uint32_t n_inputs = below(cs % 10 == 0 ? 3 : 24);
        const uint32_t n_gates = cs % 7 == 0 ? below(4) : below(cs % 50 == 0 ? 1500 : 120);
        const uint32_t n_outputs = 1 + below(12);
        std::vector<uint32_t> gates(2 * (size_t)n_gates), outs(n_outputs);
        for (uint32_t g = 0; g < n_gates; g++)
            for (int j = 0; j < 2; j++) gates[2 * g + j] = random_ref(n_inputs, g);
        for (auto &o : outs) o = random_ref(n_inputs, n_gates);
        CircuitPlan P;
        CHECK(circuit_plan(spec_gates(n_inputs, gates.data(), n_gates, outs.data(), n_outputs), P) == SGFHE_OK);
        const uint32_t n_wires = n_inputs + 3 * n_gates;
        auto id_of = [](uint32_t ref) { return ref & ~CIRC_NOT; };
        auto node_of = [&](uint32_t id) -> int64_t {
            return (id == CIRC_FALSE || id < n_inputs) ? -1 : (int64_t)((id - n_inputs) / 3);
        };
        // ---- pruning: reachability from the outputs (depth-first, restated)
        std::vector<uint8_t> reach(n_gates, 0);
        std::vector<uint32_t> stack;
        for (uint32_t o : outs)
            if (node_of(id_of(o)) >= 0) stack.push_back((uint32_t)node_of(id_of(o)));
        while (!stack.empty()) {
            const uint32_t g = stack.back();
            stack.pop_back();
            if (reach[g]) continue;
            reach[g] = 1;
            for (int j = 0; j < 2; j++)
                if (node_of(id_of(gates[2 * g + j])) >= 0) stack.push_back((uint32_t)node_of(id_of(gates[2 * g + j])));
        }
        size_t n_live = 0;
        for (uint32_t g = 0; g < n_gates; g++) {
            CHECK((P.level[g] != 0) == (reach[g] != 0));
            n_live += reach[g];
        }
        CHECK(P.live() == n_live);
        // ---- levels and order
        uint32_t maxl = 0, widest = 0;
        for (uint32_t g = 0; g < n_gates; g++) {
            if (!reach[g]) continue;
            uint32_t want = 1;
            for (int j = 0; j < 2; j++) {
                const int64_t h = node_of(id_of(gates[2 * g + j]));
                if (h >= 0) want = P.level[h] + 1 > want ? P.level[h] + 1 : want;
            }
            CHECK(P.level[g] == want);
            maxl = want > maxl ? want : maxl;
        }
        CHECK(P.levels == maxl);
        CHECK(P.level_start.size() == (size_t)maxl + 2 && P.level_start[0] == 0 && P.level_start[1] == 0);
        for (uint32_t L = 1; L <= maxl; L++) {
            const uint32_t w = P.level_start[L + 1] - P.level_start[L];
            CHECK(w > 0);
            widest = w > widest ? w : widest;
            for (uint32_t k = P.level_start[L]; k < P.level_start[L + 1]; k++) {
                CHECK(P.level[P.order[k]] == L);
                if (k > P.level_start[L]) CHECK(P.order[k] > P.order[k - 1]);
            }
        }
        CHECK(P.widest == widest);
        // ---- tables
        check_plan_tables(P);
        for (size_t k = 0; k < P.live(); k++) check_node_terms(P, k, 0, 2, &gates[2 * P.order[k]], nullptr, nullptr);
        // ---- which wires are read, and until when
        std::vector<uint32_t> readers_left(n_wires, 0);
        std::vector<uint8_t> is_out(n_wires, 0);
        for (size_t k = 0; k < P.live(); k++)
            for (int j = 0; j < 2; j++)
                if (id_of(gates[2 * P.order[k] + j]) != CIRC_FALSE) readers_left[id_of(gates[2 * P.order[k] + j])]++;
        for (uint32_t o : outs)
            if (id_of(o) != CIRC_FALSE) is_out[id_of(o)] = 1;
        for (uint32_t i = 0; i < n_inputs; i++) CHECK((P.input_slot[i] != CIRC_NONE) == (readers_left[i] || is_out[i]));
        for (size_t k = 0; k < P.live(); k++)
            for (uint32_t w = 0; w < 3; w++) {
                const uint32_t id = n_inputs + 3 * P.order[k] + w;
                CHECK((P.out_slot[3 * k + w] != CIRC_NONE) == (readers_left[id] || is_out[id]));
                if (P.out_slot[3 * k + w] != CIRC_NONE) CHECK(P.out_slot[3 * k + w] < P.slots);
            }
        // ---- simulated run over `inst` instances: slot contents are wire ids; every call gathers its rows,
        // then scatters them, calls of at most CALL_ROWS rows in row order
        const uint32_t inst = 1 + below(cs % 25 == 0 ? 9000 : 5);
        const uint32_t NONE = 0xFFFFFFFFu;
        std::vector<uint32_t> content(P.slots, NONE);
        for (uint32_t i = 0; i < n_inputs; i++)
            if (P.input_slot[i] != CIRC_NONE) {
                CHECK(P.input_slot[i] < P.slots && content[P.input_slot[i]] == NONE);
                content[P.input_slot[i]] = i;
            }
        auto expect_ref = [&](uint32_t slot_ref, uint32_t wire_ref) {
            CHECK((slot_ref & CIRC_NOT) == (wire_ref & CIRC_NOT));
            if (id_of(wire_ref) == CIRC_FALSE) { CHECK(id_of(slot_ref) == CIRC_FALSE); return; }
            CHECK(id_of(slot_ref) < P.slots && content[id_of(slot_ref)] == id_of(wire_ref));
        };
        uint64_t calls = 0;
        for (uint32_t L = 1; L <= P.levels; L++) {
            const uint32_t k0 = P.level_start[L];
            const uint64_t rows_total = P.level_rows(L, inst);
            CHECK(rows_total == (uint64_t)(P.level_start[L + 1] - k0) * inst);
            for (uint64_t row0 = 0; row0 < rows_total; row0 += SGFHE_CIRCUIT_CALL_ROWS) {
                const uint64_t rows = rows_total - row0 < SGFHE_CIRCUIT_CALL_ROWS ? rows_total - row0 : SGFHE_CIRCUIT_CALL_ROWS;
                calls++;
                // the nodes a call touches: ranks row0 / inst .. (row0 + rows - 1) / inst
                const uint32_t r0 = (uint32_t)(row0 / inst), r1 = (uint32_t)((row0 + rows - 1) / inst);
                CHECK(r1 < P.level_start[L + 1] - k0);
                for (uint32_t rk = r0; rk <= r1; rk++)   // gather
                    for (int j = 0; j < 2; j++)
                        expect_ref(P.term_ref[P.term_start[k0 + rk] + j], gates[2 * P.order[k0 + rk] + j]);
                for (uint32_t rk = r0; rk <= r1; rk++)   // scatter: the slot may not hold a wire still to be read
                    for (uint32_t w = 0; w < 3; w++) {
                        const uint32_t s = P.out_slot[3 * (k0 + rk) + w];
                        if (s == CIRC_NONE) continue;
                        const uint32_t id = n_inputs + 3 * P.order[k0 + rk] + w;
                        const uint32_t prev = content[s];
                        if (prev != id) {   // first call writing this wire (a node may span several calls)
                            CHECK(prev == NONE || (readers_left[prev] == 0 && !is_out[prev]));
                            content[s] = id;
                        }
                    }
            }
            // the level is done: its reads are spent
            for (uint32_t k = k0; k < P.level_start[L + 1]; k++)
                for (int j = 0; j < 2; j++)
                    if (id_of(gates[2 * P.order[k] + j]) != CIRC_FALSE) readers_left[id_of(gates[2 * P.order[k] + j])]--;
        }
        for (size_t o = 0; o < n_outputs; o++) expect_ref(P.out_ref[o], outs[o]);   // outputs survive to the end
        mix(P.levels); mix(P.live()); mix(P.widest); mix(P.slots); mix(calls);
        for (uint32_t v : P.term_ref) mix(v);
        for (uint32_t v : P.out_slot) mix(v);
    }
    printf("%016llx\n", (unsigned long long)digest);
    return 0;
}
