// circuit_script_calls of csrc/circuit.h -- the layout of a scripted run (sgfhe_debug_circuit_script): which calls a
// script holds, of how many rows each, reduced or not -- under AddressSanitizer and UndefinedBehaviorSanitizer on the
// CPU (tests/test_circuit_script_host.py).  A stand-alone program.
//   - stdin, per case: a line
//         name n count ct stepped steps emit pack flags n_inputs n_regs n_gates n_outputs
//     (`emit`: one 0 / 1 per step, or "-" for none), then the [n_gates][2] references of the classic nodes, the
//     n_outputs output references and the n_regs next-state references, as decimal numbers.
//   - stdout, per case: "name calls rows:raw rows:raw ...", for the test to hold against the restatement in Python
//     (tests/circuit_script_cases.py: script_calls, from Circuit.schedule() and CALL_ROWS).
// Here the list is held to the functions it is made of: counting alone gives the list's length; the level calls are
// those of circuit_level_call in the engine's walk, un-reduced exactly when the run is direct and the call has jobs;
// the refresh calls are those of circuit_pack_runs, n rows per refreshed ciphertext, none with lift; a step that is
// not emitted has no refresh call; a run that does not pack has none at all.
// Ends with "ok <cases>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

static std::vector<uint32_t> read_refs(size_t count) {
    std::vector<uint32_t> v(count);
    for (uint32_t &x : v) {
        unsigned long long t;
        CHECK(scanf(" %llu", &t) == 1);
        x = (uint32_t)t;
    }
    return v;
}

int main() {
    char name[64], emit_text[256];
    unsigned long long n, count, steps;
    int ct, stepped, pack;
    unsigned flags, n_inputs, n_regs, n_gates, n_outputs;
    size_t cases = 0;
    while (scanf(" %63s %llu %llu %d %d %llu %255s %d %u %u %u %u %u", name, &n, &count, &ct, &stepped, &steps, emit_text, &pack,
                 &flags, &n_inputs, &n_regs, &n_gates, &n_outputs) == 13) {
        const std::vector<uint32_t> gates = read_refs(2 * (size_t)n_gates), outputs = read_refs(n_outputs),
                                    next_ref = read_refs(n_regs);
        CircuitSpec S = spec_gates(n_inputs, gates.data(), n_gates, outputs.data(), n_outputs);
        S.regs.n_regs = n_regs, S.regs.next_ref = next_ref.data();
        CircuitPlan P;
        CHECK(circuit_plan(S, P) == SGFHE_OK);
        std::vector<uint8_t> emit;
        if (strcmp(emit_text, "-"))
            for (const char *p = emit_text; *p; p++) emit.push_back(*p == '1');
        CHECK(emit.empty() || (stepped && emit.size() == steps));
        CircuitRequest q;
        CircuitScript X;
        uint64_t some = 0;
        if (pack) X.tail_in = &some;   // (a flag to the layout: never read through)
        q.script = &X, q.ct = ct, q.stepped = stepped, q.count = (size_t)count, q.steps = stepped ? (size_t)steps : 1;
        q.emit = emit.empty() ? nullptr : emit.data(), q.flags = ct ? flags : 0u;
        const uint64_t instances = ct ? count * n : count;
        std::vector<CircuitScriptCall> calls(5);   // (stale content: the function clears it)
        const size_t got = circuit_script_calls(P, q, (size_t)n, instances, &calls);
        CHECK(got == calls.size() && got == circuit_script_calls(P, q, (size_t)n, instances, nullptr));
        // the engine's walk, from the functions the list is made of
        const bool packs = ct && pack, direct = packs && (flags & SGFHE_CIRCUIT_PACK_DIRECT),
                   lift = direct && (flags & SGFHE_CIRCUIT_PACK_LIFT);
        const CircuitRunSizes Z = circuit_run_sizes(P, instances, (size_t)n, ct ? (size_t)count : 0, packs, direct, lift);
        size_t at = 0;
        for (size_t s = 0; s < q.steps; s++) {
            for (uint32_t L = 1; L <= P.levels; L++) {
                uint64_t rows = 0;
                for (uint64_t row0 = 0; row0 < P.level_rows(L, instances); row0 += SGFHE_CIRCUIT_CALL_ROWS, at++) {
                    const CircuitCall C = circuit_level_call(P, L, row0, instances);
                    CHECK(at < got && calls[at].rows == C.rows && calls[at].raw == (direct && C.j1 > C.j0) && !calls[at].lut);
                    CHECK(calls[at].rows >= 1 && calls[at].rows <= SGFHE_CIRCUIT_CALL_ROWS);
                    rows += C.rows;
                }
                CHECK(rows == P.level_rows(L, instances));
            }
            if (!emit.empty() && !emit[s]) continue;
            for (size_t q0 = 0; q0 < Z.n_ct; q0 += Z.cpc) {
                const size_t fresh = circuit_pack_runs(P, (size_t)count, q0, std::min(Z.cpc, Z.n_ct - q0), !direct, nullptr);
                if (lift || !fresh) continue;
                CHECK(at < got && calls[at].rows == fresh * n && calls[at].raw && !calls[at].lut);
                CHECK(fresh <= Z.max_ref && (uint64_t)calls[at].rows <= Z.work_rows);
                at++;
            }
        }
        CHECK(at == got);
        if (!packs)
            for (const CircuitScriptCall &C : calls) CHECK(!C.raw);
        printf("%s %zu", name, got);
        for (const CircuitScriptCall &C : calls) printf(" %u:%d", C.rows, (int)C.raw);
        printf("\n");
        cases++;
    }
    printf("ok %zu\n", cases);
    return 0;
}
