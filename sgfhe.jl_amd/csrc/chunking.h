// The chunk policy of a bootstrap call (engine.hip bootstrap_device): how large a chunk is by
// default, how a call of `batch` bootstraps is cut into chunks across the lanes, and how many rows the lanes' work
// buffers need for any call up to a given size (CircuitRun::grow).  Pure functions of a few numbers the ctx holds.
// Plain C++, no HIP: tests/native/chunking_sanitized.cpp drives it under ASan / UBSan on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sgfhe {

inline uint32_t round_up8(uint32_t x) { return (x + 7u) & ~7u; }

// Default chunk: the per-iteration working set (digits + residues) of a chunk stays near the size
// of the 256 MiB Infinity Cache while a launch is long enough to amortise its ramp-up and drain
// (about 9 us per k_extprod launch).  Measured at Params(1024) (tools/chunk_sweep.py, us of
// k_extprod per bootstrap and iteration): chunk 256 0.568, 408 0.553, 512 0.547, 608 0.572,
// 816 0.575.
inline uint32_t default_chunk(uint32_t lanes, size_t bytes_per_bootstrap) {
    // Two lanes (the default): half the budget per lane, so that the working sets of both chunks
    // stay near the Infinity Cache together.  Measured at Params(1024) with k_crt_lean
    // (profiles/r03_exp_lanes_sweep.txt): two lanes of 128 / 192 / 256 / 320 / 384 give
    // 1892 / 1916 / 1907 / 1825 / 1814 bootstraps/s against 1864 for one lane of 512.
    size_t budget = (size_t)(lanes == 2 ? 160 : 320) << 20;
    size_t k = budget / bytes_per_bootstrap;
    if (k >= 256) k = (k / 256) * 256;
    else k = (k / 8) * 8;
    if (k < 8) k = 8;
    if (k > 4096) k = 4096;
    return (uint32_t)k;
}

// What the policy reads of the ctx, at the flatten mode of the call.
struct ChunkPolicy {
    uint32_t user_chunk;        // sgfhe_set_chunk (a multiple of 8), 0: automatic
    uint32_t default_chunk;     // default_chunk() of the ctx
    uint32_t lanes;             // 1 or 2
    uint32_t small_max;         // chunks of at most this many bootstraps take the small-batch form
    bool small_lanes;           // a call of a few gates may run as two halves on the two lanes
    uint32_t small_lanes_max;   // ... up to this many gates
    int logm;
    uint32_t fused_cap;         // gates one launch of the fused quarter kernel takes, 0: no such kernel here
};

// How a call is cut: chunks of `chunk` bootstraps (the last one what is left), groups of one chunk per lane in use
// every `stride` bootstraps.
struct CallChunks {
    uint32_t chunk;
    bool two_lanes;
    size_t stride;
};

inline uint32_t base_chunk(const ChunkPolicy &p) { return p.user_chunk ? p.user_chunk : p.default_chunk; }

inline CallChunks call_chunks(const ChunkPolicy &p, size_t batch) {
    uint32_t chunk = base_chunk(p);
    if (!p.user_chunk && p.lanes == 2 && batch > 2 * (size_t)p.small_max) {
        // Automatic chunk size with two lanes: cut the batch into an even number of equal chunks no
        // larger than the default, so that both lanes are busy from the first bootstrap to the last
        // (a batch of 256 runs as 128 + 128 instead of one chunk on one lane, 384 as 192 + 192
        // instead of 256 + 128).  Measured at Params(1024) (profiles/r03_exp_mid_batches.txt):
        // 64 / 128 / 256 / 384 / 640 bootstraps 1158 -> 1401, 1555 -> 1858, 1875 -> 1981, 1847 -> 2071,
        // 1850 -> 2030 per second.  Halves that would fall to the small-batch form (batch <= 48) are not
        // split: 48 bootstraps run at 1277 per second as one chunk and at 1024 as 24 + 24.
        const size_t pairs = (batch + 2 * (size_t)chunk - 1) / (2 * (size_t)chunk);
        chunk = round_up8((uint32_t)((batch + 2 * pairs - 1) / (2 * pairs)));
    } else if (!p.user_chunk && p.lanes == 2 && p.small_lanes && p.logm >= 12 &&
               batch >= (p.fused_cap ? p.fused_cap + 1 : 8u) &&
               batch <= p.small_lanes_max && (batch + 1) / 2 <= p.small_max) {
        // A call of 8 to 24 gates in the latency form: two halves on the two lanes.  Each half is a chain of
        // dependent launches on a mostly idle device, and two chains overlap; the halves need no rounding
        // to 8 (the latency kernels index their gates directly), so 8 gates run as 4 + 4 and 12 as 6 + 6
        // in the quarter form.  Same call (profiles/r04_exp_small_lanes.txt): 8 / 10 / 12 / 16 / 20 / 24 gates
        // 20.8 / 21.6 / 22.8 / 27.4 / 27.8 / 29.7 ms against 23.4 / 25.2 / 27.0 / 27.8 / 30.5 / 31.4 as one chunk;
        // below 8 gates two chains cost more than they overlap (2 / 4 / 6 gates 18.3 / 18.3 / 19.0 against
        // 15.8 / 17.8 / 19.8), so those stay on one stream.
        // With the fused quarter kernel (m = 4096, 8192) one chain takes up to 12 gates at the cost of two
        // chains of half the size or less (8 / 10 / 12 gates 20.9 / 21.9 / 22.7 ms against 21.0 / 22.0 / 22.9;
        // Params(512) 7.7 / 8.0 / 8.3 against 9.1 / 9.0 / 9.2), and the halves of 13 to 24 gates take it
        // (profiles/r04_exp_fused.txt): two chains from 13 gates there.
        // Rings below m = 4096 stay on one chain: their launches are too short for two chains to overlap, and
        // the halves then cost their sum (Params(64) / (128) / (256), 8 to 24 gates: 1.4 / 2.75 / 5.4 ms as two
        // halves against 0.7 / 1.4 / 3.3 as one chunk, profiles/r04_exp_small_rings_lanes.txt).
        chunk = (uint32_t)((batch + 1) / 2);
    }
    const bool two_lanes = p.lanes == 2 && batch > chunk;
    return {chunk, two_lanes, (size_t)chunk * (two_lanes ? 2 : 1)};
}

// Rows of the lanes' work buffers that a call of `batch` bootstraps needs: its first (and largest) chunk, padded.
inline uint32_t chunk_rows(const CallChunks &cc, size_t batch) {
    return round_up8((uint32_t)(batch < cc.chunk ? batch : cc.chunk));
}

// ... and that any call of at most `max_batch` bootstraps needs.  No automatic cut exceeds the user's or the default
// chunk, except the two halves of the small-lanes form, which are cut from the batch alone: the largest of those is
// that of the largest batch that takes the form (it counts only where the default chunk is below half of
// small_lanes_max: SGFHE_SMALL_LANES=<n> with a raised small-batch limit on a large ring, not any default setting).
inline uint32_t max_chunk_rows(const ChunkPolicy &p, size_t max_batch) {
    const size_t base = base_chunk(p);
    uint32_t rows = round_up8((uint32_t)(max_batch < base ? max_batch : base));
    size_t halves = max_batch;   // the largest batch the small-lanes form could take
    if (halves > p.small_lanes_max) halves = p.small_lanes_max;
    if (halves > 2 * (size_t)p.small_max) halves = 2 * (size_t)p.small_max;
    const uint32_t rows_halves = chunk_rows(call_chunks(p, halves), halves);
    return rows_halves > rows ? rows_halves : rows;
}

}  // namespace sgfhe
