// pg_blocks_host.h — the host half of the synteny blocks (pg_blocks.hip): the stitch over the chunks' edges.  Plain C++ without
// a GPU call, so that a stand-alone program can hold it to a loop over the runs under the host sanitizers
// (tools/blocks_stitch_check.cpp).  The link rule is pg_blocks_link.h's, the one the kernel uses.
#pragma once
#include <vector>

#include "pg_blocks_link.h"

namespace pg {

// Contig c's chunks are [first[c], first[c + 1]), in order.  counts[chunk] is what the count pass left: every kept run of a chunk
// decided but the first.  This walk decides that one — its predecessor is the last kept run of the nearest chunk before it, in
// the same contig, that has one — and hands every chunk the exclusive offsets of the emit pass (BlockChunkOffs: starts and ends
// over all contigs, the three sums inside the contig, the carried predecessor).  A block's end is counted where the next block
// of the contig starts, and once more behind the contig's last chunk when it has a kept run at all.
// nblocks[c] = the blocks of contig c; returns their sum, or ~0 when a contig's starts and ends differ (never, by construction).
inline uint64_t blocks_stitch(uint32_t ncontigs, const uint64_t *first, const BlockChunkCount *counts, uint32_t max_gap,
                              uint32_t max_shift, const uint64_t *boff, uint32_t nb, BlockChunkOffs *offs, uint64_t *nblocks) {
    uint64_t nstarts = 0, nends = 0;
    for (uint32_t c = 0; c < ncontigs; ++c) {
        const uint64_t s0 = nstarts;
        uint32_t kmers = 0, runs = 0, shifted = 0, carry_e = 0, carry_ml = BLOCKS_NONE;
        for (uint64_t i = first[c]; i < first[c + 1]; ++i) {
            const BlockChunkCount &k = counts[i];
            offs[i] = BlockChunkOffs{nstarts, nends, kmers, runs, shifted, carry_e, carry_ml, 0u};
            if (k.kept == 0) continue;  // (all dropped: the carry passes through)
            bool sh = false;
            if (blocks_link(carry_e, carry_ml, k.first_s, k.first_m, max_gap, max_shift, boff, nb, &sh)) {
                shifted += sh ? 1u : 0u;
            } else {
                nstarts += 1;
                if (carry_ml != BLOCKS_NONE) nends += 1;
            }
            nstarts += k.starts;
            nends += k.starts;  // (every start decided inside a chunk has its predecessor there: it ends a block too)
            kmers += k.kmers;
            runs += k.kept;
            shifted += k.shifted;
            carry_e = k.last_e;
            carry_ml = k.last_ml;
        }
        if (carry_ml != BLOCKS_NONE) nends += 1;
        nblocks[c] = nstarts - s0;
        if (nstarts != nends) return ~0ull;
    }
    return nstarts;
}

}  // namespace pg
