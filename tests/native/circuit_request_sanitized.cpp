// circuit_request_check of csrc/circuit.h -- the one judge of a run's arguments -- under AddressSanitizer and
// UndefinedBehaviorSanitizer on the CPU (tests/test_circuit_request_host.py).  A stand-alone program.
//   - stdin: a line "env n M split_tiles", then the cases of tests/run_error_cases.py, one per line:
//         entry case plan circ key pack_exact ct stepped probe device with_data count steps N flags mask
//     (`mask`: bit i set when pointer i of PTRS below is given).  Each becomes a CircuitRequest against the named small
//     plan; every pointer given is a dummy address that must never be read -- which is what running this under ASan
//     shows.  stdout: "entry case code message" per case, for the test to hold against the recorded fixture.
//   - every case again with `device` flipped and with a stream: the same verdict.
//   - a seeded sweep of accepted requests: the verdict's instances are count (LWE forms) or count * n (ct forms).
//   - the scripted form (CircuitRequest::script, sgfhe_debug_circuit_script): every case again with a script -- the
//     probe and device forms are refused as such, every other case has the verdict of the same request on a ctx with a
//     key, since the key is the one thing a scripted run does not need -- and every request of the sweep without a
//     key, with tail_in in place of out_w / out_v, with a NULL array of the script, and on a plan with a live LUT
//     sibling; the refusals are printed as "script <case> code message".
// Ends with "ok <cases> <sweep>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

struct Arrays {
    uint32_t n_inputs = 2, group = 1, n_planes = 0, n_regs = 0;
    std::vector<uint32_t> kind, start, ref, table, outputs, next_ref, reg_scale;
    std::vector<int32_t> shift, weight;
    void plan(CircuitPlan &P) const {
        CircuitSpec S = spec_csr(5, n_inputs, n_planes, kind.data(), start.data(), ref.data(), shift.data(), weight.data(),
                                 table.data(), kind.size(), outputs.data(), nullptr, outputs.size(), group);
        S.regs.n_regs = n_regs, S.regs.next_ref = next_ref.data(), S.regs.reg_scale = reg_scale.data();
        CHECK(circuit_plan(S, P) == SGFHE_OK);
    }
};

// the plans of run_error_cases.make_plans: wires 0, 1 the inputs, node g's wires 2 + 3 g ..
static Arrays named(const std::string &name) {
    Arrays A;
    A.kind = {0}, A.table = {0}, A.start = {0, 2}, A.ref = {0, 1}, A.outputs = {2};
    if (name == "group8") A.group = 8;
    else if (name == "group48") A.group = 48;
    else if (name == "regs") A.n_regs = 1, A.next_ref = {4}, A.reg_scale = {0};
    else if (name == "regs1") {
        A.kind = {2}, A.table = {0x96}, A.start = {0, 3}, A.ref = {CIRC_FALSE, 0, 1};
        A.n_regs = 1, A.next_ref = {3}, A.reg_scale = {1};
    } else if (name == "planes") {
        A.n_planes = 1, A.kind = {0, 4}, A.table = {0, 0}, A.start = {0, 2, 5};
        A.ref = {0, 1, CIRC_FALSE, CIRC_FALSE, 2}, A.outputs = {5};
    } else if (name == "wide") {
        A.kind = {0, 0, 0}, A.table = {0, 0, 0}, A.start = {0, 2, 4, 6};
        A.ref = {0, 1, 0, 1 | CIRC_NOT, 0 | CIRC_NOT, 1}, A.outputs = {2, 5, 8};
    } else if (name == "family") {   // a LUT node and a live sibling of it
        A.kind = {2, 3}, A.table = {0x96, 0xE8}, A.start = {0, 3, 3}, A.ref = {CIRC_FALSE, CIRC_FALSE, 0}, A.outputs = {5};
    } else CHECK(name == "plain");
    A.shift.assign(A.ref.size(), 0), A.weight.assign(A.ref.size(), 1);
    return A;
}

template <class T>
static T *dummy(bool given, uintptr_t k) { return given ? reinterpret_cast<T *>((uintptr_t)0x1000 * (k + 1)) : nullptr; }

// PTRS: in in_a in_b state_in state_a state_b data emit out out_w out_v state_out sk in_bits stats
static void set_pointers(CircuitRequest &q, unsigned long mask) {
    const auto bit = [&](int i) { return (mask >> i & 1) != 0; };
    q.in = dummy<const uint64_t>(bit(0), 0), q.in_a = dummy<const uint64_t>(bit(1), 1), q.in_b = dummy<const uint64_t>(bit(2), 2);
    q.state_in = dummy<const uint64_t>(bit(3), 3), q.state_a = dummy<const uint64_t>(bit(4), 4);
    q.state_b = dummy<const uint64_t>(bit(5), 5), q.data = dummy<const uint8_t>(bit(6), 6), q.emit = dummy<const uint8_t>(bit(7), 7);
    q.out = dummy<uint64_t>(bit(8), 8), q.out_w = dummy<uint64_t>(bit(9), 9), q.out_v = dummy<uint64_t>(bit(10), 10);
    q.state_out = dummy<uint64_t>(bit(11), 11), q.sk = dummy<const uint64_t>(bit(12), 12);
    q.in_bits = dummy<const uint8_t>(bit(13), 13), q.stats = dummy<uint64_t>(bit(14), 14);
}

static bool same(const CircuitVerdict &a, const CircuitVerdict &b) {
    return a.what == b.what && a.code == b.code && a.message == b.message && a.instances == b.instances;
}

static uint64_t g_state = 0x13198A2E03707344ull;
static uint64_t rnd(uint64_t below) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % below;
}

int main() {
    CircuitEnv env;
    unsigned long long en, eM;
    unsigned tiles;
    CHECK(scanf(" env %llu %llu %u", &en, &eM, &tiles) == 3);
    env.n = (size_t)en, env.M = (size_t)eM, env.split_tiles = tiles;
    char entry[64], name[64], plan[32];
    int circ, key, exact, ct, stepped, probe, device, with_data;
    unsigned long long count, steps, N;
    unsigned flags;
    unsigned long mask;
    size_t cases = 0;
    while (scanf(" %63s %63s %31s %d %d %d %d %d %d %d %d %llu %llu %llu %u %lu", entry, name, plan, &circ, &key, &exact, &ct,
                 &stepped, &probe, &device, &with_data, &count, &steps, &N, &flags, &mask) == 16) {
        CircuitPlan P;
        named(plan).plan(P);
        CircuitRequest q;
        q.ct = ct, q.stepped = stepped, q.probe = probe, q.device = device, q.with_data = with_data;
        q.count = (size_t)count, q.steps = (size_t)steps, q.N = (size_t)N, q.flags = flags;
        set_pointers(q, mask);
        env.have_key = key, env.pack_exact = exact;
        const CircuitVerdict v = circuit_request_check(circ ? &P : nullptr, q, env);
        CHECK((v.what == CircuitVerdict::REFUSED) == (v.code != SGFHE_OK) && (v.code != SGFHE_OK) == !v.message.empty());
        CHECK(v.what == CircuitVerdict::RUN || v.instances == 0);
        printf("%s %s %d %s\n", entry, name, v.code, v.message.c_str());
        // neither `device` nor the stream is judged
        CircuitRequest d = q;
        d.device = !q.device;
        CHECK(same(circuit_request_check(circ ? &P : nullptr, d, env), v));
        d = q, d.stream = dummy<void>(true, 15);
        CHECK(same(circuit_request_check(circ ? &P : nullptr, d, env), v));
        // the scripted form: no probe, no device form; otherwise the verdict of a ctx that has a key
        CircuitScript X;
        X.results = dummy<const uint64_t>(true, 16), X.staged = dummy<uint64_t>(true, 17), X.lut = dummy<uint32_t>(true, 18);
        d = q, d.script = &X;
        const CircuitVerdict sv = circuit_request_check(circ ? &P : nullptr, d, env);
        if (q.probe || q.device) {
            CHECK(sv.what == CircuitVerdict::REFUSED && sv.code == SGFHE_ERR_INVALID_ARG);
            CHECK(sv.message == "sgfhe_debug_circuit_script: the host forms only: no probe, no device form");
        } else {
            CircuitEnv keyed = env;
            keyed.have_key = true;
            CHECK(same(sv, circuit_request_check(circ ? &P : nullptr, q, keyed)));
        }
        cases++;
    }
    // accepted requests: every form on every plan it admits, counts the limits and the lane group allow
    env.have_key = env.pack_exact = true;
    size_t sweep = 0;
    for (const char *pl : {"plain", "group8", "regs", "planes", "wide"})
        for (int form = 0; form < 4; form++)
            for (int rep = 0; rep < 50; rep++) {
                CircuitPlan P;
                named(pl).plan(P);
                CircuitRequest q;
                q.ct = form & 1, q.stepped = (form & 2) != 0, q.with_data = true, q.device = rnd(2);
                if (P.n_regs && !q.stepped) continue;
                const uint64_t most = (q.ct ? 0x7FFFFFFFull / env.n : 0x7FFFFFFFull) / P.widest / P.group;
                q.count = (size_t)(1 + rnd(rnd(2) ? 64 : most)) * (q.ct ? 1 : P.group);
                q.steps = (size_t)(1 + rnd(5)), q.N = rnd(2) ? env.n : env.M;
                static const uint32_t FLAGS[3] = {0u, SGFHE_CIRCUIT_PACK_DIRECT, SGFHE_CIRCUIT_PACK_DIRECT | SGFHE_CIRCUIT_PACK_LIFT};
                q.flags = q.ct ? FLAGS[rnd(3)] : 0u;
                set_pointers(q, q.ct ? 0x746ul : 0x941ul);   // in_a in_b data out_w out_v | in data out state_out
                const CircuitVerdict v = circuit_request_check(&P, q, env);
                CHECK(v.what == CircuitVerdict::RUN && v.code == SGFHE_OK && v.message.empty());
                CHECK(v.instances == (q.ct ? q.count * env.n : q.count));
                sweep++;
                // scripted: no key needed; tail_in stands for out_w / out_v; each array of the script is needed
                CircuitScript X;
                X.results = dummy<const uint64_t>(true, 16), X.staged = dummy<uint64_t>(true, 17), X.lut = dummy<uint32_t>(true, 18);
                CircuitRequest s = q;
                s.script = &X, s.device = false;
                CircuitEnv bare = env;
                bare.have_key = false;
                CHECK(same(circuit_request_check(&P, s, bare), v));
                if (q.ct) {
                    s.out_w = s.out_v = nullptr;
                    CHECK(same(circuit_request_check(&P, s, bare), v) && !s.packs());   // (the LWE outputs alone)
                    s.out = nullptr;
                    CHECK(circuit_request_check(&P, s, bare).what == CircuitVerdict::REFUSED);   // no output form
                    X.tail_in = dummy<uint64_t>(true, 19);
                    CHECK(same(circuit_request_check(&P, s, bare), v) && s.packs());
                    bare.pack_exact = false;
                    CHECK(circuit_request_check(&P, s, bare).code == SGFHE_ERR_UNSUPPORTED);
                    bare.pack_exact = true;
                }
                for (int hole = 0; hole < 3; hole++) {
                    CircuitScript Y = X;
                    if (hole == 0) Y.results = nullptr;
                    if (hole == 1) Y.staged = nullptr;
                    if (hole == 2) Y.lut = nullptr;
                    s.script = &Y;
                    const CircuitVerdict h = circuit_request_check(&P, s, bare);
                    CHECK(h.what == CircuitVerdict::REFUSED && h.code == SGFHE_ERR_INVALID_ARG);
                    if (sweep == 1 && hole == 0) printf("script null_script %d %s\n", h.code, h.message.c_str());
                }
            }
    {   // a plan with a live LUT sibling: run by the entries, refused by the hook
        CircuitPlan P;
        named("family").plan(P);
        CHECK(P.siblings() == 1);
        CircuitRequest q;
        q.with_data = true, q.count = 8;
        set_pointers(q, 0x101ul);   // in out
        CHECK(circuit_request_check(&P, q, env).what == CircuitVerdict::RUN);
        CircuitScript X;
        X.results = dummy<const uint64_t>(true, 16), X.staged = dummy<uint64_t>(true, 17), X.lut = dummy<uint32_t>(true, 18);
        q.script = &X;
        const CircuitVerdict h = circuit_request_check(&P, q, env);
        CHECK(h.what == CircuitVerdict::REFUSED && h.code == SGFHE_ERR_INVALID_ARG);
        printf("script live_sibling %d %s\n", h.code, h.message.c_str());
        q.probe = true;
        printf("script probe_form %d %s\n", circuit_request_check(&P, q, env).code, circuit_request_check(&P, q, env).message.c_str());
    }
    printf("ok %zu %zu\n", cases, sweep);
    return 0;
}
