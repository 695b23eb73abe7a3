// circuit_plain_bits of csrc/circuit.h (the plaintext wire evaluation of sgfhe_circuit_run_probe) under
// AddressSanitizer and UndefinedBehaviorSanitizer on the CPU (tests/test_noise_host.py).
// Reads one circuit and its input bits from stdin:
//   n_inputs n_gates n_outputs instances
//   n_gates lines "x y" (wire references, decimal uint32), one line of n_outputs references,
//   n_inputs lines of `instances` characters 0 / 1
// and prints one line per probe row: "<wire id> <bits of the instances>".  It also checks, on its own, the
// numbering of the probe rows against the plan (term_row names the row of the wire the node reads) and that an
// instance count of 0 and NULL bits are handled.
#include <stdio.h>
#include <stdlib.h>

#include <string>
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

int main() {
    unsigned n_inputs, n_gates, n_outputs;
    size_t instances;
    CHECK(scanf("%u %u %u %zu", &n_inputs, &n_gates, &n_outputs, &instances) == 4);
    std::vector<uint32_t> gates(2 * (size_t)n_gates), outs(n_outputs);
    for (auto &g : gates) CHECK(scanf("%u", &g) == 1);
    for (auto &o : outs) CHECK(scanf("%u", &o) == 1);
    std::vector<uint8_t> bits((size_t)n_inputs * instances);
    for (unsigned i = 0; i < n_inputs; i++) {
        std::vector<char> line(instances + 2);
        CHECK(scanf("%s", line.data()) == 1);
        CHECK(std::string(line.data()).size() == instances);
        for (size_t t = 0; t < instances; t++) bits[i * instances + t] = (uint8_t)(line[t] - '0');
    }
    CircuitPlan P;
    CHECK(circuit_plan(spec_gates(n_inputs, gates.data(), n_gates, outs.data(), n_outputs), P) == SGFHE_OK);
    // the probe rows: inputs, then the three wires of every live node in `order`; term_row names them
    check_plan_tables(P);
    for (size_t k = 0; k < P.live(); k++) check_node_terms(P, k, 0, 2, &gates[2 * P.order[k]], nullptr, nullptr);
    std::vector<uint64_t> table;
    CHECK(circuit_plain_bits(P, bits.data(), instances, table) == SGFHE_OK);
    const size_t wpr = circuit_bit_words(instances);
    CHECK(table.size() == circuit_probe_rows(P) * wpr);
    for (size_t row = 0; row < circuit_probe_rows(P); row++) {
        printf("%u ", circuit_probe_wire(P, row));
        for (size_t t = 0; t < instances; t++) putchar('0' + (int)((table[row * wpr + t / 64] >> (t % 64)) & 1));
        putchar('\n');
    }
    std::vector<uint64_t> none;
    CHECK(circuit_plain_bits(P, nullptr, 0, none) == SGFHE_OK && none.empty());
    if (n_inputs && instances) CHECK(circuit_plain_bits(P, nullptr, instances, none) == SGFHE_ERR_INVALID_ARG);
    return 0;
}
