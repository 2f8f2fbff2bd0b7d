// pg_tablescan.h — what the kernels that pass once over every slot of a pan table share (k_table_pair_counts in
// pg_tablestats.hip, k_table_screen in pg_screen.hip): how the slots are cut into chunks and the chunks dealt to waves, a lane's
// way from its slot of chunk 0 to its slot of every other chunk in all four layouts, and the grid.
//
// A chunk = the slots of 64 / slots-per-line whole lines (64 slots at 8 or 16 slots per line, 60 at the inline layout's 6, 56 at
// the byte-mask layout's 14), one slot per lane; wave w of block x takes chunks 4 x + w, 4 (x + blocks) + w, ...  Both layouts'
// arrays are affine in the line number, so a lane keeps two pointers and two steps.
#pragma once
#include "pg_kernels.h"
#include <algorithm>

namespace pg {

constexpr uint32_t TABLESTATS_BLOCKS = 2048;  // blocks per slice: 8 per CU of an MI355X
constexpr uint32_t TS_QCAP = 128;             // entries of a wave's queue: fewer than 64 left over + up to 64 of one chunk

// LDS writes of this wave's lanes before, its lanes' reads of them behind
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// this lane's slot of a chunk: slot s of the chunk's line number l
struct SlotWalk {
    const uint8_t *key0, *mask0;  // its key and its mask (word 0, or the byte of the byte-mask layout) in chunk 0
    uint64_t key_step, mask_step;  // the way from one chunk to the next
    uint64_t nchunks, nlines;
    uint32_t l, s, chunk_lines;
    bool mine, bm;  // the chunk has such a slot; byte-mask layout: a slot's mask is one byte in its line

    __device__ __forceinline__ SlotWalk(const SubTable &st, uint32_t lane, uint64_t nchunks_, uint32_t chunk_lines_)
        : nchunks(nchunks_), nlines(st.nbuckets), l(lane / st.slots), s(lane - (lane / st.slots) * st.slots), chunk_lines(chunk_lines_) {
        mine = l < chunk_lines;
        bm = st.layout == LAYOUT_BYTEMASK;
        key0 = reinterpret_cast<const uint8_t *>(key_ptr(st, mine ? l : 0, s));
        mask0 = bm ? mask_byte_ptr(st, mine ? l : 0, s) : reinterpret_cast<const uint8_t *>(mask_ptr(st, mine ? l : 0, s, 0));
        key_step = reinterpret_cast<const uint8_t *>(key_ptr(st, chunk_lines, 0)) - reinterpret_cast<const uint8_t *>(key_ptr(st, 0, 0));
        mask_step = bm ? key_step
                       : reinterpret_cast<const uint8_t *>(mask_ptr(st, chunk_lines, 0, 0)) - reinterpret_cast<const uint8_t *>(mask_ptr(st, 0, 0, 0));
    }
    // the key of this lane's slot of chunk c (EMPTY_KEY where the chunk has no such slot)
    __device__ __forceinline__ uint64_t key_of(uint64_t c) const {
        return c < nchunks && mine && c * chunk_lines + l < nlines ? *reinterpret_cast<const unsigned long long *>(key0 + c * key_step) : EMPTY_KEY;
    }
    // the mask of that slot, where key_of(c) found a key: its words (not in the byte-mask layout), its byte (there)
    __device__ __forceinline__ const uint32_t *mask_words(uint64_t c) const { return reinterpret_cast<const uint32_t *>(mask0 + c * mask_step); }
    __device__ __forceinline__ uint32_t mask_byte(uint64_t c) const { return mask0[c * mask_step]; }
    // the line of that slot
    __device__ __forceinline__ uint64_t line_of(uint64_t c) const { return c * chunk_lines + l; }
};

// the chunks of a table and the blocks (per slice) that pass over them: TABLESTATS_BLOCKS wherever the table has that many
// chunks, and more where that would leave a wave 2^24 chunks or more — so that a block visits fewer than 2^32 slots and 32-bit
// counters hold whatever it counts.  0 blocks: more than a grid takes.
inline uint64_t tablescan_blocks(const SubTable &t, uint32_t &chunk_lines, uint64_t &nchunks) {
    chunk_lines = 64 / t.slots;
    nchunks = (t.nbuckets + chunk_lines - 1) / chunk_lines;
    const uint64_t per_wave_cap = (1ull << 24) - 1;
    const uint64_t blocks = std::max<uint64_t>(std::min<uint64_t>((nchunks + 3) / 4, TABLESTATS_BLOCKS), (nchunks + 4 * per_wave_cap - 1) / (4 * per_wave_cap));
    return blocks > 0x7FFFFFFFull ? 0 : blocks;
}

}  // namespace pg
