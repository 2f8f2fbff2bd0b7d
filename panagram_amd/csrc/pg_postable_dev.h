// pg_postable_dev.h — what the kernels on a position table share: the slot, the canonical key with its strand bit, and the rule by
// which a word continues its predecessor's run (k_mate_runs in pg_synteny.hip, k_hit_runs in pg_locate.hip).  How the table is
// walked: pg_keytable_dev.h.  Device code only.
#pragma once
#include "pg_keytable_dev.h"

namespace pg {

struct PosSlot {
    unsigned long long key;
    uint32_t word[2];
};
static_assert(sizeof(PosSlot) == POS_SLOT_BYTES, "16-byte slots");
__device__ __forceinline__ const unsigned long long &slot_key(const PosSlot &slot) { return slot.key; }

// X > B: the reverse complement's value is the smaller one
__device__ __forceinline__ bool kmer_key_rc(const uint64_t *seqw, uint64_t p, int k, uint64_t &key) {
    const uint64_t X = extract_bases(seqw, p) & kmer_mask(k);
    const uint64_t B = revcomp_le(X, k);
    key = canonical_from_xb(X, B, k);
    return X > B;
}

// does the mate `m` of a position continue the run of its predecessor's mate `prev`?  (64-bit sums: nothing wraps)
__device__ __forceinline__ bool mate_continues(uint32_t prev, uint32_t m) {
    if (m == NO_MATE || prev == NO_MATE) return false;
    return (m & 1u) ? (uint64_t)m + 2 == (uint64_t)prev : (uint64_t)m == (uint64_t)prev + 2;
}

}  // namespace pg
