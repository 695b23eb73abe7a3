// The fill kernel of a plan with lane masks (sgfhe_circuit_create_masked; csrc/circuit.h).  It
// lives in a header of its own: kernels.h holds the kernels its CPU sessions launch one by one, and this one is driven
// by tests/native/circuit_masks_engine_cpu.cpp through a scripted run.
#pragma once

#include "kernels.h"

namespace sgfhe {

// The off lanes of a level's masked nodes, as zeros: for every off pair (node, lane) of the level -- `off_node` the
// rank in the level, whose three slots are out_slot[3 rank ..] -- and every wire of the node that has a slot, row
// group * G + lane of that slot for every group of the run is the trivial LWE (0, 0), all n + 1 words zero.  A reader --
// circ_ref_word of a gather, the lift, the collect, the next states -- then needs no mask test.
// One thread per 8-byte word, grid-stride over [off pair][wire][group][word]: consecutive threads write consecutive
// words of a row (coalesced 8-byte stores), offsets in 64 bits, no LDS.
// Queued once per level (per step in a stepped run) on the run's stream, and safe anywhere inside its level: no
// reference of a level reads a slot that the level writes -- a slot is free again only after the last level that reads
// its wire, which is why call 1's scatter may already precede call 2's gather -- and the rows written here are never
// rows of a scatter, which writes the pairs that are on.
__global__ void __launch_bounds__(256)
k_circ_mask_fill(uint64_t *__restrict__ wires, const uint32_t *__restrict__ out_slot,
                 const uint32_t *__restrict__ off_node, const uint32_t *__restrict__ off_lane, uint32_t n_off,
                 uint32_t per, uint32_t group, uint32_t instances, uint32_t n) {
    const size_t row = (size_t)n + 1, total = (size_t)n_off * 3 * per * row;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t e = t % row, x = t / row, grp = x % per, y = x / per;
        const uint32_t w = (uint32_t)(y % 3), p = (uint32_t)(y / 3);
        const uint32_t slot = out_slot[3 * (size_t)off_node[p] + w];
        if (slot == CIRC_SLOT_NONE) continue;
        wires[((size_t)slot * instances + grp * group + off_lane[p]) * row + e] = 0ull;
    }
}

}  // namespace sgfhe
