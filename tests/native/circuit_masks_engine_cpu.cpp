// Lane masks through the CPU build of the engine (csrc/engine.hip against tests/native/hipcpu; the flags of
// tests/engine_cpu.py) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_circuit_masks_host.py builds
// and runs it under both HIPCPU_FILL bytes.  A stand-alone program, no input.  It is the sanitizer run of the row
// decode (circ_row in k_circ_gather, k_circ_xor3 and k_circ_scatter) and of k_circ_mask_fill.
// Masked plans run through sgfhe_debug_circuit_script on a keyless ctx at Params(64), one-shot and stepped; the result
// rows of every call are this program's own words, and everything the run hands back is compared with integers
// computed here by a model that restates the contract of include/sgfhe_hip.h instance by instance:
//   - what every call staged (both inputs of every row, in the pair-major row order) and its LUT descriptors;
//   - the final wire table: every wire of every node is an output, plain or negated, so the collected outputs are the
//     table -- the rows a scatter wrote, LOW = U - 2 HI of the sum nodes, and all-zero rows on the off lanes, whatever
//     byte the device memory held before (the fill byte);
//   - the registers after the last step of a stepped run, one of them fed by a masked node.
// The plans: a small one of classic, sum and LUT nodes with shifts and NOTs on references to masked wires, at G = 4 over
// 8 instances; and one level of five classic nodes with 8, 3, 5, 8, 1 lanes set at G = 8 over 3200 instances, 10000
// rows in two calls, row 8192 inside the fourth node's pairs.
// Prints "ok <words compared>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/sgfhe_hip.h"

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #cond);    \
            abort();                                                              \
        }                                                                         \
    } while (0)

static const uint32_t FALSE_ID = SGFHE_CIRCUIT_FALSE, NOT = SGFHE_CIRCUIT_NOT;
static const size_t N = 64, ROW = N + 1;
static const uint64_t R = 1024;
static size_t g_compared = 0;

static uint64_t g_state = 0x452821E638D01377ull;
static uint64_t rnd(uint64_t below) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % below;
}

struct Term {
    uint32_t ref;
    int32_t shift, weight;
};
struct Node {
    uint32_t kind, table, level;   // kind 0 classic, 1 sum, 2 LUT; level as the planner gives it (1 ..)
    std::vector<Term> terms;
    std::vector<uint8_t> lanes;    // [G] 0 / 1; empty: every lane
};
struct Model {
    uint32_t n_inputs = 0, n_regs = 0, G = 1;
    std::vector<Node> nodes;
    std::vector<uint32_t> outputs;       // wire references, shift 0
    std::vector<uint32_t> next_ref;      // [n_regs]
    std::vector<int32_t> next_shift;
};

typedef std::vector<uint64_t> Rows;   // [instances][ROW]

// reference `ref` at the lane shift d, instance t, word e; NOT at the codeword `one`
static uint64_t read_word(const Model &M, const std::vector<Rows> &wires, uint32_t ref, int32_t d, size_t t, size_t e,
                          uint64_t one) {
    const uint32_t id = ref & ~NOT;
    const int64_t lane = (int64_t)(t % M.G) + d;
    uint64_t v = 0;
    if (id != FALSE_ID && lane >= 0 && lane < (int64_t)M.G) v = wires[id][(size_t)((int64_t)t + d) * ROW + e];
    if (!(ref & NOT)) return v;
    return ((e < N ? 0 : one) + R - v) & (R - 1);
}

struct Script {
    std::vector<uint64_t> results, staged;   // as the hook takes and fills them, call after call
    std::vector<uint32_t> lut;
};

// One step of the model: every level's rows in pair-major order, cut into calls; the inputs of every row appended to
// `want` (what the hook must have staged), the result rows drawn here and appended to the script, the wires written.
static void model_step(const Model &M, std::vector<Rows> &wires, size_t inst, Script &S, Script &want) {
    const size_t per = inst / M.G;
    uint32_t levels = 0;
    for (const Node &nd : M.nodes) levels = std::max(levels, nd.level);
    for (uint32_t L = 1; L <= levels; L++) {
        struct RowAt {
            size_t g, t;
        };
        std::vector<RowAt> rows;
        for (size_t g = 0; g < M.nodes.size(); g++) {
            if (M.nodes[g].level != L) continue;
            for (uint32_t l = 0; l < M.G; l++) {
                if (!M.nodes[g].lanes.empty() && !M.nodes[g].lanes[l]) continue;
                for (size_t grp = 0; grp < per; grp++) rows.push_back({g, grp * M.G + l});
            }
            for (uint32_t w = 0; w < 3; w++) wires[M.n_inputs + 3 * g + w].assign(inst * ROW, 0);   // off lanes: FALSE
        }
        for (size_t row0 = 0; row0 < rows.size(); row0 += SGFHE_CIRCUIT_CALL_ROWS) {
            const size_t cnt = std::min<size_t>(SGFHE_CIRCUIT_CALL_ROWS, rows.size() - row0);
            bool has_lut = false;
            for (size_t j = 0; j < cnt; j++) has_lut = has_lut || M.nodes[rows[row0 + j].g].kind == 2;
            for (size_t j = 0; j < cnt; j++) {
                const Node &nd = M.nodes[rows[row0 + j].g];
                const size_t t = rows[row0 + j].t;
                uint64_t u[ROW], v[ROW];
                for (size_t e = 0; e < ROW; e++) {
                    u[e] = v[e] = 0;
                    if (nd.kind == 0) {
                        u[e] = read_word(M, wires, nd.terms[0].ref, nd.terms[0].shift, t, e, R / 4);
                        v[e] = read_word(M, wires, nd.terms[1].ref, nd.terms[1].shift, t, e, R / 4);
                    } else if (nd.kind == 2) {
                        for (size_t p = 0; p < 3; p++)
                            u[e] += read_word(M, wires, nd.terms[p].ref, nd.terms[p].shift, t, e, (R / 4) >> (2 - p));
                        u[e] &= R - 1;
                    } else {
                        int64_t s = 0;
                        for (const Term &tm : nd.terms) s += tm.weight * (int64_t)read_word(M, wires, tm.ref, tm.shift, t, e, R / 4);
                        u[e] = (uint64_t)s & (R - 1);
                    }
                }
                want.staged.insert(want.staged.end(), u, u + ROW);
                want.staged.insert(want.staged.end(), v, v + ROW);
                want.lut.push_back(has_lut && nd.kind == 2 ? 0x100u | nd.table : 0u);
                // the call's result rows: this program's words; LOW of a sum node is U - 2 HI
                uint64_t res[3][ROW];
                for (auto &gate : res)
                    for (uint64_t &x : gate) x = rnd(R);
                for (size_t w = 0; w < 3; w++) S.results.insert(S.results.end(), res[w], res[w] + ROW);
                for (size_t e = 0; e < ROW; e++) {
                    if (nd.kind == 1) res[2][e] = (u[e] + v[e] - 2 * res[0][e]) & (R - 1);
                    for (size_t w = 0; w < 3; w++) wires[M.n_inputs + 3 * rows[row0 + j].g + w][t * ROW + e] = res[w][e];
                }
            }
        }
    }
}

struct Plan {
    sgfhe_circuit *h = nullptr;
    std::vector<uint32_t> kind, start, ref, table, node_mask, reg_scale;
    std::vector<int32_t> shift, weight;
    std::vector<uint8_t> masks;
};
static void make_plan(const Model &M, Plan &P) {
    uint32_t n_masks = 0;
    P.start.push_back(0);
    for (const Node &nd : M.nodes) {
        P.kind.push_back(nd.kind), P.table.push_back(nd.table);
        for (const Term &t : nd.terms) P.ref.push_back(t.ref), P.shift.push_back(t.shift), P.weight.push_back(t.weight);
        P.start.push_back((uint32_t)P.ref.size());
        if (nd.lanes.empty()) {
            P.node_mask.push_back(0);
            continue;
        }
        P.masks.insert(P.masks.end(), nd.lanes.begin(), nd.lanes.end());
        P.node_mask.push_back(++n_masks);
    }
    P.reg_scale.assign(M.n_regs + 1, 0);
    CHECK(sgfhe_circuit_create_masked(M.n_inputs, 0, P.kind.data(), P.start.data(), P.ref.data(), P.shift.data(),
                                      P.weight.data(), P.table.data(), M.nodes.size(), M.outputs.data(), nullptr,
                                      M.outputs.size(), M.G, M.n_regs, M.next_ref.data(), M.next_shift.data(),
                                      P.reg_scale.data(), 0, nullptr, nullptr, nullptr, nullptr, n_masks, P.masks.data(),
                                      P.node_mask.data(), &P.h) == SGFHE_OK);
    uint32_t nm = 0;
    uint64_t rows = 0, want = 0;
    for (const Node &nd : M.nodes) want += nd.lanes.empty() ? M.G : (uint64_t)std::count(nd.lanes.begin(), nd.lanes.end(), 1);
    CHECK(sgfhe_circuit_masks(P.h, &nm, &rows) == SGFHE_OK && nm == n_masks && rows == want);
}

static void same(const uint64_t *got, const std::vector<uint64_t> &want, int line) {
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i]) {
            fprintf(stderr, "line %d: word %zu of %zu is %llu, not %llu\n", line, i, want.size(), (unsigned long long)got[i],
                    (unsigned long long)want[i]);
            abort();
        }
    g_compared += want.size();
}
#define SAME(got, want) same((got).data(), want, __LINE__)

// the outputs of the model's wire table: reference o at every instance (shift 0), NOT at Dr
static void collect(const Model &M, const std::vector<Rows> &wires, size_t inst, std::vector<uint64_t> &out) {
    for (uint32_t ref : M.outputs)
        for (size_t t = 0; t < inst; t++)
            for (size_t e = 0; e < ROW; e++) out.push_back(read_word(M, wires, ref, 0, t, e, R / 4));
}

// every wire of every node as an output, then every one negated
static void all_wires_out(Model &M) {
    for (uint32_t neg : {0u, NOT})
        for (size_t g = 0; g < M.nodes.size(); g++)
            for (uint32_t w = 0; w < 3; w++) M.outputs.push_back((M.n_inputs + 3 * (uint32_t)g + w) | neg);
}

static void run(sgfhe_ctx *ctx, const Model &M, size_t inst, size_t steps) {
    Plan P;
    make_plan(M, P);
    const uint32_t n_stream = M.n_inputs - M.n_regs;
    std::vector<uint64_t> state((size_t)M.n_regs * inst * ROW + 1), stream(steps * n_stream * inst * ROW);
    for (auto &x : state) x = rnd(R);
    for (auto &x : stream) x = rnd(R);
    // the model, step by step
    std::vector<Rows> wires(M.n_inputs + 3 * M.nodes.size());
    Script S, want;
    std::vector<uint64_t> want_out, want_state(state.begin(), state.end() - 1);
    for (size_t s = 0; s < steps; s++) {
        for (uint32_t i = 0; i < M.n_regs; i++)
            wires[i].assign(want_state.begin() + (size_t)i * inst * ROW, want_state.begin() + (size_t)(i + 1) * inst * ROW);
        for (uint32_t i = 0; i < n_stream; i++) {
            const uint64_t *src = stream.data() + (s * n_stream + i) * inst * ROW;
            wires[M.n_regs + i].assign(src, src + inst * ROW);
        }
        model_step(M, wires, inst, S, want);
        collect(M, wires, inst, want_out);
        for (uint32_t i = 0; i < M.n_regs; i++)
            for (size_t t = 0; t < inst; t++)
                for (size_t e = 0; e < ROW; e++)
                    want_state[((size_t)i * inst + t) * ROW + e] = read_word(M, wires, M.next_ref[i], M.next_shift[i], t, e, R / 4);
    }
    // the hook
    const uint32_t form = M.n_regs ? SGFHE_SCRIPT_STEPPED : 0u;
    size_t n_calls = 0;
    CHECK(sgfhe_debug_circuit_script_calls(ctx, P.h, form, inst, steps, nullptr, 0, 0, &n_calls, nullptr, nullptr, 0) == SGFHE_OK);
    std::vector<uint32_t> call_rows(n_calls + 1);
    std::vector<uint8_t> call_raw(n_calls + 1);
    CHECK(sgfhe_debug_circuit_script_calls(ctx, P.h, form, inst, steps, nullptr, 0, 0, &n_calls, call_rows.data(),
                                           call_raw.data(), n_calls) == SGFHE_OK);
    size_t total = 0;
    for (size_t i = 0; i < n_calls; i++) {
        total += call_rows[i];
        CHECK(!call_raw[i]);
    }
    CHECK(total == want.lut.size() && S.results.size() == total * 3 * ROW);
    S.staged.assign(total * 2 * ROW, ~0ull), S.lut.assign(total, ~0u);
    std::vector<uint64_t> out(want_out.size(), ~0ull), state_out(want_state.size() + 1, ~0ull);
    const int32_t rc = sgfhe_debug_circuit_script(ctx, P.h, form, inst, steps, M.n_regs ? state.data() : nullptr, nullptr,
                                                  stream.data(), nullptr, 0, nullptr, nullptr, out.data(),
                                                  M.n_regs ? state_out.data() : nullptr, 0, S.results.data(), S.staged.data(),
                                                  S.lut.data(), nullptr);
    if (rc != SGFHE_OK) fprintf(stderr, "sgfhe_debug_circuit_script: %d %s\n", rc, sgfhe_last_error_string(ctx));
    CHECK(rc == SGFHE_OK);
    SAME(S.staged, want.staged);
    CHECK(S.lut == want.lut);
    SAME(out, want_out);
    if (M.n_regs) SAME(state_out, want_state);
    // the probe entries refuse the plan before anything runs
    if (!M.n_regs) {
        std::vector<uint64_t> sk(N, 0), stats((M.n_inputs + 3 * M.nodes.size()) * 8, 7);
        std::vector<uint8_t> bits((size_t)M.n_inputs * inst, 0);
        std::fill(out.begin(), out.end(), ~0ull);
        CHECK(sgfhe_circuit_run_probe(ctx, P.h, inst, stream.data(), out.data(), sk.data(), bits.data(), stats.data()) ==
              SGFHE_ERR_UNSUPPORTED);
        CHECK(strstr(sgfhe_last_error_string(ctx), "lane masks"));
        CHECK(out[0] == ~0ull && stats[0] == 7);
    }
    sgfhe_circuit_destroy(P.h);
}

int main() {
    sgfhe_params par = {};   // Params(64)
    par.n = N, par.r = R, par.m = 512, par.ell = 2;
    par.Q[0] = 5494391545392009217ull, par.B[0] = 2348810240ull, par.DQ_tilde[0] = 686798943174001152ull;
    sgfhe_ctx *ctx = nullptr;
    CHECK(sgfhe_ctx_create(&par, 0, &ctx) == SGFHE_OK);
    {   // G = 4, 8 instances: inputs x = 0, y = 1
        Model M;
        M.n_inputs = 2, M.G = 4;
        M.nodes = {
            {0, 0, 1, {{0, 0, 1}, {1 | NOT, 1, 1}}, {1, 0, 1, 0}},                 // wires 2, 3, 4: lanes 0 and 2
            {1, 0, 1, {{0, 0, 2}, {1, -1, -1}, {FALSE_ID | NOT, 0, 1}}, {0, 0, 0, 1}},   // wires 5, 6, 7: lane 3 only
            {0, 0, 2, {{2, 1, 1}, {7 | NOT, -1, 1}}, {}},                          // wires 8, 9, 10: reads off lanes
            {2, 0x96, 2, {{FALSE_ID, 0, 1}, {FALSE_ID | NOT, 0, 1}, {3 | NOT, 0, 1}}, {0, 1, 1, 1}},   // wires 11, 12, 13
            {1, 0, 3, {{8, 0, 1}, {11 | NOT, 2, 2}, {5, -3, -2}}, {0, 1, 0, 0}},   // wires 14, 15, 16: lane 1 only
            {2, 0xE8, 3, {{13 | NOT, 0, 1}, {12, -1, 1}, {9, 1, 1}}, {1, 1, 1, 0}},   // wires 17, 18, 19: reads scales 2, 1, 0
        };
        // every scale-0 wire as an output, plain and negated
        for (uint32_t neg : {0u, NOT})
            for (uint32_t w : {2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 10u, 11u, 14u, 15u, 16u, 17u}) M.outputs.push_back(w | neg);
        run(ctx, M, 8, 1);
        // stepped: x is a register fed by the masked node 0's AND wire at a shift, 3 steps
        Model T = M;
        T.n_regs = 1, T.next_ref = {2 | NOT}, T.next_shift = {-1};
        run(ctx, T, 8, 3);
    }
    {   // one level, G = 8, 3200 instances: 25 pairs of 400 groups, 10000 rows, row 8192 inside the fourth node
        Model M;
        M.n_inputs = 2, M.G = 8;
        const uint32_t set[5] = {8, 3, 5, 8, 1};
        for (uint32_t g = 0; g < 5; g++) {
            Node nd = {0, 0, 1, {{0u | (g & 1 ? NOT : 0u), (int32_t)g - 2, 1}, {1, 0, 1}}, {}};
            if (set[g] < 8)
                for (uint32_t l = 0; l < 8; l++) nd.lanes.push_back((l * 3 + g) % 8 < set[g]);
            M.nodes.push_back(nd);
        }
        all_wires_out(M);
        run(ctx, M, 3200, 1);
    }
    CHECK(sgfhe_ctx_destroy(ctx) == SGFHE_OK);
    printf("ok %zu\n", g_compared);
    return 0;
}
