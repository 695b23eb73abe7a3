// The chunk policy of a bootstrap call in csrc/chunking.h -- default_chunk, call_chunks, chunk_rows, max_chunk_rows --
// under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU (tests/test_chunking_host.py).
// A stand-alone program, no input.
//   - The worked cases of the comments in chunking.h, at default chunk 256, two lanes, small_max 24, small_lanes_max 24,
//     logm 13, no fused kernel: 256 = 128 + 128, 384 = 192 + 192, 640 in chunks of 160, 4096 in chunks of 256,
//     49 = 32 + 17, 48 one chunk, 8 = 4 + 4, 12 = 6 + 6, 24 = 12 + 12, 7 one chunk.  With a fused cap of 12: 8 to 12 one
//     chunk, 13 = 7 + 6.  With logm 11, or small_lanes off: 8 to 24 one chunk.  One lane: never split.  A user chunk:
//     that chunk, whatever the batch.
//   - Over batch 1..10000 x default chunk {8, 64, 256, 1024, 4096} x lanes {1, 2} x small_max {16, 24} x logm {11..14}
//     x fused cap {0, 12} x user chunk {0, 104}: chunk >= 1; walking the groups the way bootstrap_device does
//     (g0 += stride, one chunk per lane in use) covers the batch exactly once; two_lanes == (lanes == 2 && batch >
//     chunk); outside the small-lanes form every chunk but the last is a multiple of 8; chunk <= the user chunk when
//     one is set.
//   - The work buffers of a circuit run: CircuitRun::grow sizes them once with max_chunk_rows(policy, work_rows), so
//     that no call of the run regrows them: no call of at most work_rows bootstraps needs more rows (chunk_rows) than
//     that, for every work_rows of the sweep.  The figure is round_up8(min(work_rows, user or default chunk)) wherever
//     that bound holds by itself, and never below it.  (It does not hold by itself where the halves of the small-lanes
//     form exceed the default chunk: default chunk 8, 17 to 24 gates.  `-v` lists those settings.)
// Prints "ok <cases>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "chunking.h"

using namespace sgfhe;

#define CHECK(cond)                                                                                                  \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            fprintf(stderr, "check failed at line %d: %s (batch %zu, user %u, default %u, lanes %u, small_max %u, "  \
                    "small_lanes %d, small_lanes_max %u, logm %d, fused cap %u)\n", __LINE__, #cond, cur_batch,       \
                    P.user_chunk, P.default_chunk, P.lanes, P.small_max, (int)P.small_lanes, P.small_lanes_max,      \
                    P.logm, P.fused_cap);                                                                            \
            abort();                                                                                                 \
        }                                                                                                            \
    } while (0)

static ChunkPolicy P;
static size_t cur_batch = 0;
static unsigned long long cases = 0;

// the chunks of a call, walked as bootstrap_device walks them: {first chunk, second chunk, chunks in all}
struct Walk {
    size_t first, second, count;
};
static Walk walk(const CallChunks &cc, size_t batch, bool small_form) {
    Walk w = {0, 0, 0};
    size_t next = 0;   // the first bootstrap no chunk has taken yet
    CHECK(cc.stride >= 1);
    for (size_t g0 = 0; g0 < batch; g0 += cc.stride)
        for (int li = 0; li < (cc.two_lanes ? 2 : 1); li++) {
            const size_t c0 = g0 + (size_t)li * cc.chunk;
            if (c0 >= batch) break;
            const size_t cb = batch - c0 < cc.chunk ? batch - c0 : cc.chunk;
            CHECK(c0 == next && cb >= 1);
            next = c0 + cb;
            if (next < batch && !small_form) CHECK(cb % 8 == 0);   // every chunk but the last
            if (w.count == 0) w.first = cb;
            if (w.count == 1) w.second = cb;
            w.count++;
        }
    CHECK(next == batch);
    return w;
}

// the condition of the small-lanes form, from the comments: automatic, two lanes, switched on, m >= 4096, from 8 gates
// (with a fused kernel: from one more than a launch of it takes) up to small_lanes_max, halves within the small-batch form
static bool small_lanes_form(size_t batch) {
    return !P.user_chunk && P.lanes == 2 && P.small_lanes && P.logm >= 12 && batch <= 2 * (size_t)P.small_max &&
           batch >= (P.fused_cap ? P.fused_cap + 1 : 8u) && batch <= P.small_lanes_max;
}

static void expect(size_t batch, uint32_t chunk, size_t first, size_t second, size_t count) {
    cur_batch = batch;
    const CallChunks cc = call_chunks(P, batch);
    const Walk w = walk(cc, batch, small_lanes_form(batch));
    CHECK(cc.chunk == chunk && w.first == first && w.second == second && w.count == count);
    CHECK(cc.two_lanes == (count > 1));
    cases++;
}
static void expect_one_chunk(size_t batch) {
    cur_batch = batch;
    const CallChunks cc = call_chunks(P, batch);
    const Walk w = walk(cc, batch, false);
    CHECK(w.count == 1 && w.first == batch && !cc.two_lanes && cc.stride == cc.chunk);
    cases++;
}

static void worked_cases() {
    const ChunkPolicy base = {0, 256, 2, 24, true, 24, 13, 0};
    P = base;
    expect(256, 128, 128, 128, 2);
    expect(384, 192, 192, 192, 2);
    expect(640, 160, 160, 160, 4);
    expect(4096, 256, 256, 256, 16);
    expect(49, 32, 32, 17, 2);
    expect_one_chunk(48);
    expect(8, 4, 4, 4, 2);
    expect(12, 6, 6, 6, 2);
    expect(24, 12, 12, 12, 2);
    expect_one_chunk(7);
    P.fused_cap = 12;
    for (size_t b = 8; b <= 12; b++) expect_one_chunk(b);
    expect(13, 7, 7, 6, 2);
    P = base, P.logm = 11;
    for (size_t b = 8; b <= 24; b++) expect_one_chunk(b);
    P = base, P.small_lanes = false;
    for (size_t b = 8; b <= 24; b++) expect_one_chunk(b);
    P = base, P.lanes = 1;
    for (size_t b = 1; b <= 10000; b++) {
        cur_batch = b;
        const CallChunks cc = call_chunks(P, b);
        CHECK(cc.chunk == 256 && !cc.two_lanes && cc.stride == 256);
        cases++;
    }
    for (uint32_t lanes = 1; lanes <= 2; lanes++) {
        P = base, P.lanes = lanes, P.user_chunk = 104;
        for (size_t b = 1; b <= 10000; b++) {
            cur_batch = b;
            const CallChunks cc = call_chunks(P, b);
            CHECK(cc.chunk == 104 && cc.two_lanes == (lanes == 2 && b > 104));
            cases++;
        }
    }
    // default_chunk: 160 MiB a lane with two lanes, 320 MiB with one; whole multiples of 256 from 256, of 8 below;
    // 8 to 4096
    cur_batch = 0;
    CHECK(default_chunk(2, (size_t)160 << 10) == 1024 && default_chunk(1, (size_t)160 << 10) == 2048);
    CHECK(default_chunk(2, ((size_t)160 << 20) / 300) == 256 && default_chunk(2, ((size_t)160 << 20) / 100) == 96);
    CHECK(default_chunk(2, (size_t)100 << 20) == 8 && default_chunk(1, 1) == 4096);
    cases += 6;
}

static void sweep(bool verbose) {
    const uint32_t defaults[] = {8, 64, 256, 1024, 4096}, users[] = {0, 104}, small_maxes[] = {16, 24}, caps[] = {0, 12};
    const size_t BATCH_MAX = 10000;
    for (uint32_t user : users)
        for (uint32_t dflt : defaults)
            for (uint32_t lanes = 1; lanes <= 2; lanes++)
                for (uint32_t small_max : small_maxes)
                    for (int logm = 11; logm <= 14; logm++)
                        for (uint32_t fused_cap : caps) {
                            P = {user, dflt, lanes, small_max, true, 24, logm, fused_cap};
                            uint32_t rows_max = 0;   // the most rows any call of at most `batch` bootstraps needs
                            size_t short_from = 0, short_to = 0;
                            for (size_t batch = 1; batch <= BATCH_MAX; batch++) {
                                cur_batch = batch;
                                const CallChunks cc = call_chunks(P, batch);
                                CHECK(cc.chunk >= 1);
                                CHECK(cc.two_lanes == (lanes == 2 && batch > cc.chunk));
                                CHECK(cc.stride == (size_t)cc.chunk * (cc.two_lanes ? 2 : 1));
                                if (user) CHECK(cc.chunk <= user);
                                const Walk w = walk(cc, batch, small_lanes_form(batch));
                                // the first chunk is the largest: the work buffers are sized for it
                                CHECK(w.first >= w.second && chunk_rows(cc, batch) == round_up8((uint32_t)w.first));
                                if (chunk_rows(cc, batch) > rows_max) rows_max = chunk_rows(cc, batch);
                                // a run whose largest call has `batch` bootstraps (work_rows = batch)
                                const uint32_t base = user ? user : dflt;
                                const uint32_t plain = round_up8((uint32_t)(batch < base ? batch : base));
                                const uint32_t got = max_chunk_rows(P, batch);
                                CHECK(rows_max <= got);
                                CHECK(got >= plain);
                                if (rows_max <= plain) CHECK(got == plain);
                                else if (!short_from) short_from = short_to = batch;
                                else short_to = batch;
                                cases++;
                            }
                            if (verbose && short_from)
                                printf("round_up8(min(work_rows, chunk)) falls short for work_rows %zu..%zu: default chunk "
                                       "%u, lanes %u, small_max %u, logm %d, fused cap %u\n", short_from, short_to, dflt,
                                       lanes, small_max, logm, fused_cap);
                        }
}

int main(int argc, char **argv) {
    worked_cases();
    sweep(argc > 1 && !strcmp(argv[1], "-v"));
    printf("ok %llu\n", cases);
    return 0;
}
