// The call arithmetic of a run in csrc/circuit.h -- circuit_level_call, circuit_job_chunk, circuit_pack_runs,
// circuit_run_sizes -- under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU (tests/test_circuit_calls_host.py).
// A stand-alone program, no input.  Plans: classic, lanes, three-input, sum nodes, pruned nodes, outputs that name
// inputs, the constant, LOW wires, shifted wires and one gate wire twice; instances from 1 to 2736 (3 nodes x 2736 =
// 8208 rows: a level of two calls whose boundary lies inside a node), n = 1, 8, 64 and 20000 (one ciphertext per group).
// Every function is compared with a restatement that knows rows only:
//   - row R of a level belongs to call R / CALL_ROWS and to node k0 + R / instances; a call's nodes are those of its
//     rows, its jobs those whose job_k is among them, it holds a sum node when one of them is one;
//   - the calls of a level partition its rows, their job ranges the level's jobs (a job whose node straddles two calls
//     belongs to both: its rows come from both);
//   - the chunks of a job range cover it once, at most 65535 grid rows each, the wire block in the first only (also on
//     synthetic ranges of up to 200000 jobs);
//   - the runs of a pack group are the maximal runs of ciphertexts that are not direct, ranks counted from 0; with
//     "all" the group is one run;
//   - max_ref is the maximum over the groups, 0 with lift; max_rows, n_ct, cpc and work_rows by their definitions;
//   - walking a run the way the engine does consumes the closed-form number of call numbers: the sum of
//     ceil(rows / CALL_ROWS) over the levels; per pack group one (plain form, lift) or one plus one if it refreshes
//     anything (direct).  This walk is written out HERE, from the functions' results; the engine's own branches
//     (CircuitRun::pack_group: lift, else bootstrap if anything is refreshed, a fresh number for the tail only under
//     direct) are not run by this program.  What they number is guarded on the device alone
//     (tests/test_gpu_pack_direct.py, test_gpu_pack_lift.py: bytes in the randomised mode and the next call's number).
// Prints a digest of everything the functions returned (the plain build must print the same).
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "circuit.h"
#include "circuit_tables.h"

using namespace sgfhe;

#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            fprintf(stderr, "check failed at line %d: %s (plan %d)\n", __LINE__, #cond, cs);  \
            abort();                                                                          \
        }                                                                                     \
    } while (0)

static int cs = -1;
static uint64_t digest = 1469598103934665603ull;
static void mix(uint64_t v) { digest = (digest ^ v) * 1099511628211ull; }

static uint64_t rng_state = 0x6A09E667F3BCC908ull;
static uint32_t below(uint32_t n) {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

constexpr uint64_t CALL_ROWS = SGFHE_CIRCUIT_CALL_ROWS;

// ---- the chunking of a job range [j0, j1)
static void check_chunks(size_t j0, size_t j1) {
    size_t covered = j0, chunks = 0;
    for (size_t j = j0; j < j1; chunks++) {
        const CircuitJobChunk ch = circuit_job_chunk(j, j0, j1);
        CHECK(j == covered && ch.nj >= 1 && ch.wires == (chunks == 0 ? 1u : 0u));
        CHECK(ch.nj + ch.wires <= 65535u && j + ch.nj <= j1);
        if (j + ch.nj < j1) CHECK(ch.nj + ch.wires == 65535u);   // only the last grid is short
        covered = j += ch.nj;
        mix(ch.nj);
    }
    CHECK(covered == j1);
    CHECK(chunks == (j1 - j0 + 1 + 65534) / 65535);   // (jobs + the one wire block) / 65535, rounded up
}

// ---- the levels of a run over `instances`; returns the calls made
static uint64_t check_levels(const CircuitPlan &P, uint64_t instances) {
    uint64_t calls = 0;
    size_t jobs_seen = 0;   // jobs of the levels before this one
    for (uint32_t L = 1; L <= P.levels; L++) {
        const uint32_t k0 = P.level_start[L], k1 = P.level_start[L + 1];
        const uint64_t rows_total = (uint64_t)(k1 - k0) * instances;
        // row by row: the nodes of every call
        std::vector<std::set<uint32_t>> nodes((size_t)((rows_total + CALL_ROWS - 1) / CALL_ROWS));
        for (uint64_t R = 0; R < rows_total; R++) nodes[(size_t)(R / CALL_ROWS)].insert(k0 + (uint32_t)(R / instances));
        uint64_t next_row = 0;
        size_t level_j0 = P.job_k.size(), level_j1 = 0, prev_j0 = 0, prev_j1 = 0;   // prev: the last call with jobs
        for (uint64_t row0 = 0, ci = 0; row0 < rows_total; row0 += CALL_ROWS, ci++) {
            const CircuitCall C = circuit_level_call(P, L, row0, instances);
            CHECK(ci < nodes.size() && C.k0 == k0);
            CHECK(row0 == next_row && C.rows >= 1 && C.rows <= CALL_ROWS && row0 + C.rows <= rows_total);
            next_row = row0 + C.rows;
            const std::set<uint32_t> &want = nodes[(size_t)ci];
            CHECK(C.ka == *want.begin() && C.kb == *want.rbegin() && want.size() == C.kb - C.ka + 1);
            bool sum = false;
            for (uint32_t k : want) sum = sum || P.node_kind[k] != 0;
            CHECK(C.sum == sum);
            std::vector<size_t> jobs;
            for (size_t j = 0; j < P.job_k.size(); j++)
                if (want.count(P.job_k[j])) jobs.push_back(j);
            CHECK(C.j1 - C.j0 == jobs.size() && C.j0 <= C.j1 && C.j1 <= P.job_k.size());
            for (size_t i = 0; i < jobs.size(); i++) CHECK(jobs[i] == C.j0 + i);
            // every job's producing rows: rank in level (what the scatter kernel is told) inside the call's nodes
            for (size_t j = C.j0; j < C.j1; j++) CHECK(k0 + P.jobs[3 * j + 1] == P.job_k[j]);
            // consecutive calls: ranges ascend, and overlap only in the jobs of a node both calls hold
            if (level_j1 && !jobs.empty()) {
                CHECK(prev_j0 <= C.j0 && C.j0 <= prev_j1 && prev_j1 <= C.j1);
                for (size_t j = C.j0; j < prev_j1; j++) CHECK(P.job_k[j] == C.ka && nodes[(size_t)ci - 1].count(C.ka));
            }
            if (!jobs.empty()) {
                level_j0 = std::min(level_j0, C.j0);
                level_j1 = std::max(level_j1, C.j1);
                prev_j0 = C.j0, prev_j1 = C.j1;
                check_chunks(C.j0, C.j1);
            }
            calls++;
            mix(C.rows); mix(C.ka); mix(C.kb); mix(C.j0); mix(C.j1); mix(C.sum);
        }
        CHECK(next_row == rows_total);
        CHECK(calls > 0 && nodes.size() == (rows_total + CALL_ROWS - 1) / CALL_ROWS);
        // the level's jobs: exactly those of its nodes, a run of the table that follows the earlier levels' jobs
        size_t want_jobs = 0;
        for (uint32_t k : P.job_k) want_jobs += k >= k0 && k < k1;
        if (want_jobs) CHECK(level_j0 == jobs_seen && level_j1 == jobs_seen + want_jobs);
        else CHECK(level_j1 == 0);
        jobs_seen += want_jobs;
    }
    CHECK(jobs_seen == P.job_k.size());
    return calls;
}

// ---- the pack stage over `blocks` ciphertexts per output of n bits each; returns the call numbers it takes
static uint64_t check_pack(const CircuitPlan &P, uint64_t instances, size_t n, size_t blocks, bool direct, bool lift) {
    const CircuitRunSizes S = circuit_run_sizes(P, instances, n, blocks, true, direct, lift);
    const size_t n_ct = (size_t)P.n_outputs * blocks, per = std::max<size_t>(1, CALL_ROWS / n);
    CHECK(S.n_ct == n_ct && S.cpc == std::min(per, n_ct) && S.cpc >= 1);
    uint64_t max_rows = 0;
    for (uint32_t L = 1; L <= P.levels; L++)
        max_rows = std::max(max_rows, std::min<uint64_t>(CALL_ROWS, P.level_rows(L, instances)));
    CHECK(S.max_rows == max_rows);
    uint64_t calls = 0;
    size_t max_ref = 0;
    std::vector<CircuitPackRun> runs(3);   // (stale content: the function clears it)
    for (size_t q0 = 0; q0 < n_ct; q0 += S.cpc) {
        const size_t cnt = std::min(S.cpc, n_ct - q0);
        const size_t nref = circuit_pack_runs(P, blocks, q0, cnt, !direct, &runs);
        CHECK(circuit_pack_runs(P, blocks, q0, cnt, !direct, nullptr) == nref);
        // ciphertext by ciphertext: maximal runs of those that are not direct
        std::vector<CircuitPackRun> want;
        size_t rank = 0;
        for (size_t q = q0; q < q0 + cnt; q++) {
            const bool fresh = !direct || P.out_node[q / blocks] == CIRC_NONE;
            if (!fresh) continue;
            const bool opens = q == q0 || !(!direct || P.out_node[(q - 1) / blocks] == CIRC_NONE);
            if (opens) want.push_back({q, rank, 0});
            want.back().len++;
            rank++;
        }
        CHECK(rank == nref && runs.size() == want.size());
        for (size_t i = 0; i < want.size(); i++) {
            CHECK(runs[i].q == want[i].q && runs[i].rank == want[i].rank && runs[i].len == want[i].len && runs[i].len >= 1);
            if (i) CHECK(runs[i - 1].q + runs[i - 1].len < runs[i].q);   // maximal: a direct ciphertext between two runs
            mix(runs[i].q); mix(runs[i].rank); mix(runs[i].len);
        }
        if (!direct) CHECK(runs.size() == 1 && runs[0].q == q0 && runs[0].rank == 0 && runs[0].len == cnt);
        max_ref = std::max(max_ref, nref);
        // the engine's group: lift -> the tail alone; else a bootstrap call if anything is refreshed; direct -> the tail
        // takes a number of its own, plain -> it shares the bootstrap's
        if (direct) calls += (lift ? 0 : nref != 0) + 1;
        else calls += 1;
    }
    if (lift && direct) max_ref = 0;
    CHECK(S.max_ref == max_ref && S.max_ref <= S.cpc);
    CHECK(S.work_rows == std::max<uint64_t>(max_rows, (uint64_t)max_ref * n));
    // closed form
    uint64_t closed = 0;
    for (size_t q0 = 0; q0 < n_ct; q0 += S.cpc) {
        bool refreshes = false;
        for (size_t q = q0; q < std::min(q0 + S.cpc, n_ct); q++) refreshes = refreshes || P.out_node[q / blocks] == CIRC_NONE;
        closed += direct && !lift && refreshes ? 2 : 1;
    }
    CHECK(calls == closed);
    mix(S.max_rows); mix(S.n_ct); mix(S.cpc); mix(S.max_ref); mix(S.work_rows);
    return calls;
}

static void check_plan(const CircuitPlan &P, uint64_t instances, size_t n) {
    check_plan_tables(P);
    CHECK(instances % P.group == 0);
    const uint64_t level_calls = check_levels(P, instances);
    uint64_t closed = 0;
    for (uint32_t L = 1; L <= P.levels; L++) closed += (P.level_rows(L, instances) + CALL_ROWS - 1) / CALL_ROWS;
    CHECK(level_calls == closed);
    mix(level_calls);
    // the LWE form: no pack stage, nothing refreshed
    const CircuitRunSizes S0 = circuit_run_sizes(P, instances, n, 0, false, true, true);
    CHECK(S0.n_ct == 0 && S0.cpc == 0 && S0.max_ref == 0 && S0.work_rows == S0.max_rows);
    if (instances % n) return;
    const size_t blocks = (size_t)(instances / n);
    const uint64_t plain = check_pack(P, instances, n, blocks, false, false);
    const uint64_t direct = check_pack(P, instances, n, blocks, true, false);
    const uint64_t lifted = check_pack(P, instances, n, blocks, true, true);
    const CircuitRunSizes Sp = circuit_run_sizes(P, instances, n, blocks, true, false, false);
    const CircuitRunSizes Sl = circuit_run_sizes(P, instances, n, blocks, true, false, true);   // lift without direct: plain
    CHECK(Sp.max_ref == Sp.cpc && Sl.max_ref == Sp.max_ref && Sl.work_rows == Sp.work_rows);
    const uint64_t groups = (Sp.n_ct + Sp.cpc - 1) / Sp.cpc;
    CHECK(plain == groups && lifted == groups && direct >= groups && direct <= 2 * groups);
    mix(level_calls + plain); mix(level_calls + direct); mix(level_calls + lifted);
}

// ---- plans
struct Arrays {
    uint32_t n_inputs = 0;
    std::vector<uint32_t> kind, start{0}, refs, outs;
    std::vector<int32_t> shift, weight, oshift;
    uint32_t node(uint32_t k, std::initializer_list<uint32_t> r, std::initializer_list<int32_t> w,
                  std::initializer_list<int32_t> d = {}) {   // returns the node's first wire
        kind.push_back(k);
        refs.insert(refs.end(), r);
        weight.insert(weight.end(), w);
        shift.insert(shift.end(), d);
        shift.resize(refs.size(), 0);
        start.push_back((uint32_t)refs.size());
        return n_inputs + 3 * (uint32_t)(kind.size() - 1);
    }
    void out(uint32_t ref, int32_t d = 0) { outs.push_back(ref); oshift.push_back(d); }
    int32_t plan(uint32_t G, CircuitPlan &P) const {
        return circuit_plan(spec_csr(1, n_inputs, 0, kind.data(), start.data(), refs.data(), shift.data(), weight.data(),
                                     nullptr, kind.size(), outs.data(), oshift.data(), outs.size(), G), P);
    }
};

// three nodes on level 1 (a classic one, a three-input one, a sum node), two on level 2, one pruned; outputs: gate wires
// of the first and the last node of level 1, an input, a negated gate wire, the constant, a LOW wire, a shifted gate
// wire (G > 1), and the first one again
static Arrays fixed_circuit(uint32_t G) {
    Arrays A;
    A.n_inputs = 3;
    const uint32_t g0 = A.node(0, {0, 1}, {1, 1});
    const uint32_t g1 = A.node(1, {0, 1 | CIRC_NOT, 2}, {1, 1, 1});
    const uint32_t g2 = A.node(1, {2, 0}, {2, -1}, {G > 1 ? 1 : 0, 0});
    A.node(0, {g0, g1 + 1}, {1, 1});                                   // pruned: nothing names it
    const uint32_t g4 = A.node(0, {g0 + 2, g2 | CIRC_NOT}, {1, 1});
    const uint32_t g5 = A.node(1, {g1, g2 + 1, CIRC_FALSE | CIRC_NOT}, {2, 2, 1});
    A.out(g2 + 1); A.out(g0); A.out(1); A.out(g1 | CIRC_NOT); A.out(CIRC_FALSE | CIRC_NOT); A.out(g5 + 2);
    A.out(g4 + 1, G > 1 ? -1 : 0); A.out(g0); A.out(g5); A.out(g4 | CIRC_NOT);
    return A;
}

static Arrays random_circuit(uint32_t G) {
    static const int32_t W[4] = {-2, -1, 1, 2};
    Arrays A;
    A.n_inputs = 1 + below(5);
    const uint32_t n_gates = 1 + below(40);
    auto ref = [&](uint32_t wires, uint32_t recent) {
        uint32_t id = below(10) == 0 ? CIRC_FALSE : below(wires);
        if (recent && below(3) == 0) id = recent - 1 - below(std::min(recent, 6u)) + 0;   // deep chains too
        return id | (below(2) ? CIRC_NOT : 0u);
    };
    auto shift = [&]() -> int32_t { return G > 1 && below(3) == 0 ? (int32_t)below(2 * G - 1) - (int32_t)(G - 1) : 0; };
    for (uint32_t g = 0; g < n_gates; g++) {
        const uint32_t wires = A.n_inputs + 3 * g, pick = below(4);
        const uint32_t fan = pick == 0 ? 2 : pick == 1 ? 3 : 1 + below(6);
        A.kind.push_back(pick == 0 ? 0u : 1u);
        for (uint32_t j = 0; j < fan; j++) {
            A.refs.push_back(ref(wires, g ? wires : 0));
            A.shift.push_back(shift());
            A.weight.push_back(pick < 2 ? 1 : W[below(4)]);
        }
        A.start.push_back((uint32_t)A.refs.size());
    }
    const uint32_t n_outputs = 1 + below(9);
    for (uint32_t o = 0; o < n_outputs; o++) A.out(ref(A.n_inputs + 3 * n_gates, 0), below(4) == 0 ? shift() : 0);
    return A;
}

int main() {
    // ---- the chunking alone, on synthetic ranges
    for (size_t jobs : {(size_t)1, (size_t)2, (size_t)65533, (size_t)65534, (size_t)65535, (size_t)65536,
                        (size_t)131069, (size_t)131070, (size_t)200000})
        for (size_t j0 : {(size_t)0, (size_t)7, (size_t)70000}) check_chunks(j0, j0 + jobs);
    // ---- the fixed circuit: CSR entry (G = 1, 8), every form of output; 2736 instances put a call boundary inside
    // the third node of level 1 (3 x 2736 = 8208 rows)
    for (uint32_t G : {1u, 8u}) {
        CircuitPlan P;
        cs = -(int)G;
        CHECK(fixed_circuit(G).plan(G, P) == SGFHE_OK);
        CHECK(P.levels == 2 && P.live() == 5 && P.level_start[2] - P.level_start[1] == 3);
        CHECK(P.out_node[0] == 2 && P.out_node[1] == 0 && P.out_node[2] == CIRC_NONE && P.out_node[3] == 1);
        CHECK(P.out_node[4] == CIRC_NONE && P.out_node[5] == CIRC_NONE && P.out_node[7] == 0);
        CHECK((P.out_node[6] == CIRC_NONE) == (G > 1));
        for (uint64_t instances : {(uint64_t)8, (uint64_t)64, (uint64_t)2736, (uint64_t)8192, (uint64_t)8200})
            for (size_t n : {(size_t)1, (size_t)8, (size_t)64, (size_t)20000}) check_plan(P, instances, n);
        const CircuitCall C0 = circuit_level_call(P, 1, 0, 2736), C1 = circuit_level_call(P, 1, CALL_ROWS, 2736);
        CHECK(C0.rows == 8192 && C0.ka == 0 && C0.kb == 2 && C1.rows == 16 && C1.ka == 2 && C1.kb == 2);
        CHECK(C0.j0 == 0 && C1.j1 == C0.j1 && C1.j0 < C1.j1 && C1.j0 > C0.j0 && C0.sum && C1.sum);   // node 2's jobs: both calls
    }
    // ---- the classic and the three-input entries: same arithmetic over their plans
    {
        const uint32_t gates[8] = {0, 1, 1 | CIRC_NOT, 0, 2, 5, 3, 9}, outs[5] = {11, 0, 2 | CIRC_NOT, CIRC_FALSE, 11};
        CircuitPlan P;
        cs = -100;
        CHECK(circuit_plan(spec_gates(2, gates, 4, outs, 5), P) == SGFHE_OK);
        for (uint64_t instances : {(uint64_t)1, (uint64_t)5, (uint64_t)4200, (uint64_t)8192}) check_plan(P, instances, instances > 5 ? 8 : 1);
        const uint32_t g3[9] = {0, 1, 2, 0, 1 | CIRC_NOT, CIRC_NO_INPUT, 3, 6, 8}, o3[4] = {9, 5, 11 | CIRC_NOT, 2};
        const int32_t s3[9] = {0, 0, 0, 0, 0, 0, -1, 3, 0}, os3[4] = {0, 0, 0, 2};
        cs = -101;
        CHECK(circuit_plan(spec_arity(3, 3, g3, s3, 3, o3, os3, 4, 4), P) == SGFHE_OK);
        for (uint64_t instances : {(uint64_t)4, (uint64_t)64, (uint64_t)4100}) check_plan(P, instances, 4);
    }
    // ---- random circuits of every node kind, with and without lane groups
    for (cs = 0; cs < 400; cs++) {
        const uint32_t G = cs % 3 == 0 ? 1u : cs % 3 == 1 ? 4u : 16u;
        const Arrays A = random_circuit(G);
        CircuitPlan P;
        CHECK(A.plan(G, P) == SGFHE_OK);
        const size_t n = cs % 4 == 0 ? 16 : cs % 4 == 1 ? 64 : cs % 4 == 2 ? 1024 : 16384;
        const uint64_t blocks = 1 + below(cs % 10 == 0 ? 40 : 3);
        check_plan(P, cs % 5 == 4 ? (uint64_t)G * (1 + below(300)) : blocks * n, n);
    }
    printf("%016llx\n", (unsigned long long)digest);
    return 0;
}
