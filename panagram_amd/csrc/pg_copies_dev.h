// pg_copies_dev.h — what the kernels that read a count table share (pg_copies.hip builds it, counts into it and profiles along it;
// pg_place.hip joins one of its planes with finished bitmap rows): the key of a position and the bounded walk to its slot.  The
// validity of a position is extract_nmask's (pg_device.h), as everywhere.
#pragma once
#include "pg_device.h"

namespace pg {

constexpr uint32_t SLOT_INVALID = 0xFFFFFFFFu, SLOT_ABSENT = 0xFFFFFFFEu;  // (slots are below 2^31)

__device__ __forceinline__ uint64_t copy_key(const uint64_t *seqw, uint64_t p, int k) { return canonical_from_le(extract_bases(seqw, p), k); }

// the slot of `key` in a table that is not being written: its number, or SLOT_ABSENT
__device__ __forceinline__ uint32_t copy_lookup(const unsigned long long *__restrict__ keys, uint64_t smask, uint32_t max_probe, uint64_t key) {
    uint64_t s = sketch_hash(key) & smask;
    for (uint32_t probes = 0; probes < max_probe; ++probes, s = (s + 1) & smask) {
        const unsigned long long cur = keys[s];
        if (cur == EMPTY_KEY) break;
        if (cur == key) return (uint32_t)s;
    }
    return SLOT_ABSENT;
}

}  // namespace pg
