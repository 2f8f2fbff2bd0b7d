// pg_blocks_link.h — the link rule of the synteny blocks and the per-chunk records that k_run_blocks (pg_blocks.hip) and the host
// stitch (pg_blocks_host.h) exchange.  Included by both halves and by tools/blocks_stitch_check.cpp, which has no HIP: this is
// the tree's ONE link rule (the definitions are at the top of pg_blocks.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_BLOCKS_HD __host__ __device__ inline
#else
#define PG_BLOCKS_HD inline
#endif

namespace pg {

constexpr uint32_t RUN_CHUNK = 4096;          // runs per chunk, a multiple of 256
constexpr uint32_t BLOCKS_NONE = 0xFFFFFFFFu;  // in place of a last mate word: no kept run before this one (no run's ml is this)
constexpr uint32_t BLOCKS_MAX_GAP = 0x7FFFFFFFu;

// what the count pass leaves per chunk: the chunk's FIRST kept run is decided by nobody here (its predecessor lies any number
// of chunks back), so `starts` and `shifted` leave it out; first_* / last_* are link operands, unset when kept == 0
struct BlockChunkCount {
    uint32_t kept, starts, kmers, shifted;
    uint32_t first_s, first_m;  // start and mate word of the first kept run
    uint32_t last_e, last_ml;   // exclusive end and last mate word of the last kept run
};
static_assert(sizeof(BlockChunkCount) == 32, "two 16-byte stores");

// what the emit pass takes per chunk: the starts / ends of all chunks before it (all contigs), the contig's sums over the kept
// runs before it (k-mers, kept runs, shifted links: the link into the chunk's first kept run is NOT in `shifted`, the kernel
// evaluates it again), and the last kept run before the chunk in its contig (carry_ml == BLOCKS_NONE: none)
struct BlockChunkOffs {
    uint64_t soff, eoff;
    uint32_t kmers, runs, shifted;
    uint32_t carry_e, carry_ml, pad;
};
static_assert(sizeof(BlockChunkOffs) == 40, "five 8-byte words");

// the links as variants (pg_variants.hip): what its count pass leaves per chunk — the links of classes 0..5 (same, snp, mnp, ins,
// del, complex) and the records, which are the links of classes 1..5.  A lane compares at most VARIANTS_MAX_GAP / 32 words.
constexpr uint32_t VARIANTS_MAX_GAP = 65536;
struct VariantChunkCount {
    uint32_t records, cls[6], pad;
};
static_assert(sizeof(VariantChunkCount) == 32, "two 16-byte stores");

// the mate word of the last k-mer of a run of n >= 1 k-mers whose first mate word is m (the host has checked that the run lies
// inside B: nothing wraps, and the result is never BLOCKS_NONE)
PG_BLOCKS_HD uint32_t blocks_last_mate(uint32_t m, uint32_t n) {
    const uint64_t d = 2ull * (uint64_t)(n - 1);
    return (uint32_t)((m & 1u) ? (uint64_t)m - d : (uint64_t)m + d);
}

// how many of the n ascending offsets are <= p: at most 32 halvings (n < 2^32)
PG_BLOCKS_HD uint32_t blocks_rank(const uint64_t *offs, uint32_t n, uint64_t p) {
    uint32_t lo = 0, hi = n;
    for (uint32_t it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offs[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// does kept run j (start s_j, mate word m_j) link to its predecessor i (exclusive end e_i, last mate word ml_i)?  boff: the nb
// offsets of B's contigs, ascending (contig c of B holds global positions [boff[c], boff[c + 1]); empty contigs repeat an
// offset).  *shifted: dA != dB, set only for a link.  The same-contig search runs last, for a pair that passed all else.
PG_BLOCKS_HD bool blocks_link(uint32_t e_i, uint32_t ml_i, uint32_t s_j, uint32_t m_j, uint32_t max_gap, uint32_t max_shift,
                              const uint64_t *boff, uint32_t nb, bool *shifted) {
    if (ml_i == BLOCKS_NONE || ((ml_i ^ m_j) & 1u)) return false;
    const int64_t dA = (int64_t)s_j - ((int64_t)e_i - 1);
    const int64_t bl = (int64_t)(ml_i >> 1), b = (int64_t)(m_j >> 1);
    const int64_t dB = (m_j & 1u) ? bl - b : b - bl;
    if (dA < 1 || dA > (int64_t)max_gap || dB < 1 || dB > (int64_t)max_gap) return false;
    const int64_t shift = dA > dB ? dA - dB : dB - dA;
    if (shift > (int64_t)max_shift) return false;
    if (blocks_rank(boff, nb, (uint64_t)bl) != blocks_rank(boff, nb, (uint64_t)b)) return false;
    *shifted = dA != dB;
    return true;
}

}  // namespace pg
