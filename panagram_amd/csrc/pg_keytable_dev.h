// pg_keytable_dev.h — how a table of canonical k-mers in HBM is laid out and walked, for every kernel that builds or reads one: the
// position table (16-byte PosSlots, pg_postable_dev.h: pg_synteny.hip, pg_locate.hip) and the count table (8-byte keys with counter
// planes beside them: pg_copies.hip, pg_place.hip).  pg_keytable_host.h is the host's half.  Device code only.
//
// The policy: `nslots` slots, a power of two; a slot is free while its key is EMPTY_KEY (no canonical k-mer, pg_device.h); the home
// slot of a key is sketch_hash(key) & (nslots - 1); linear probing, over at most `max_probe` slots — no walk is unbounded.  A lane
// whose claim reaches the bound gets KEY_ABSENT and its kernel raises the table's overflow flag, which the host makes sticky: a
// table that overflowed answers nothing any more, so a lookup that walks as far has no hit to miss.
// Tables are never read while they are written: key_claim reads atomically, key_find plainly.
// One reader keeps key_find's walk written out, for its speed: hit_word of pg_locate.hip.  A change of the policy goes there too.
//
// Beside the walk, what the kernels over a seqset's k-mer positions share: the view of one contig with the validity of a window,
// and the sum of per-wave counts that a block adds to a counter in HBM.
#pragma once
#include "pg_kernels.h"

namespace pg {

// ---- one contig of a seqset: its packed bases, its non-ACGT mask, its k-mer positions (the contig holds at least k bases) ----
struct ContigView {
    const uint64_t *seqw;
    const uint32_t *nmw;
    uint64_t nkmers;
    bool hasn;
};

__device__ __forceinline__ ContigView contig_view(const SeqDesc *__restrict__ sd, uint32_t contig, const uint64_t *seqw_all,
                                                  const uint32_t *nmw_all, const uint32_t *has_n, int k) {
    const SeqDesc d = sd[contig];
    return {seqw_all + d.seq_off, nmw_all + d.seq_off, d.len - (uint64_t)k + 1, has_n[contig] != 0};
}

// does the window of k bases at position p exist (no non-ACGT base in it)?  p below v.nkmers
__device__ __forceinline__ bool window_valid(const ContigView &v, uint64_t p, int k) { return !(v.hasn && extract_nmask(v.nmw, p, k)); }

// ---- the probe ----
constexpr uint64_t KEY_ABSENT = ~0ull;  // (no slot number: a table holds at most 2^33 slots)

// the key of a slot (PosSlot's: pg_postable_dev.h)
__device__ __forceinline__ const unsigned long long &slot_key(const unsigned long long &slot) { return slot; }

// the slot of `key` in a table that is not being written, or `absent`.  Index: the width the caller keeps slot numbers in — 64
// bits, or 32 with a mark of its own for a table known to hold fewer slots than that (the count table: its readers come out
// instruction for instruction as they were with a 32-bit walk of their own, and longer with the 64-bit number narrowed).
// hit: where the found slot's contents go, as the walk read them.  A reader that wants what stands beside the key takes it from
// there: a table far larger than the caches gives the slot's line up between the walk and a second read of it, and k_pos_mates
// was a quarter slower reading the words behind the walk (profiles/keytable_ab.txt).
template <class Index = uint64_t, class Slot>
__device__ __forceinline__ Index key_find(const Slot *__restrict__ slots, uint64_t smask, uint32_t max_probe, uint64_t key,
                                          Index absent = (Index)KEY_ABSENT, Slot *hit = nullptr) {
    uint64_t s = sketch_hash(key) & smask;
    for (uint32_t probes = 0; probes < max_probe; ++probes, s = (s + 1) & smask) {
        const Slot cur = slots[s];
        if (slot_key(cur) == EMPTY_KEY) break;
        if (slot_key(cur) == key) {
            if (hit) *hit = cur;
            return (Index)s;
        }
    }
    return absent;
}

// the slot of `key` in a table under construction — claimed by a 64-bit CAS (EMPTY -> key), `claimed` then, or found to hold the
// key already — or KEY_ABSENT when max_probe slots hold other keys
template <class Slot>
__device__ __forceinline__ uint64_t key_claim(Slot *slots, uint64_t smask, uint32_t max_probe, uint64_t key, bool &claimed) {
    claimed = false;
    uint64_t s = sketch_hash(key) & smask;
    for (uint32_t probes = 0; probes < max_probe; ++probes, s = (s + 1) & smask) {
        unsigned long long *kp = const_cast<unsigned long long *>(&slot_key(slots[s]));  // (the caller's slots are not const)
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY_KEY) {
            cur = atomicCAS(kp, (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            if (cur == EMPTY_KEY) {
                claimed = true;
                cur = key;
            }
        }
        if (cur == key) return s;
    }
    return KEY_ABSENT;
}

// ---- the count table's keys and the 32-bit slot marks its readers keep (its slots are below 2^31: COPIES_MAX_SLOTS) ----
constexpr uint32_t SLOT_INVALID = 0xFFFFFFFFu, SLOT_ABSENT = 0xFFFFFFFEu;

__device__ __forceinline__ uint64_t copy_key(const uint64_t *seqw, uint64_t p, int k) { return canonical_from_le(extract_bases(seqw, p), k); }

// the slot of `key` in a count table that is not being written: its number, or SLOT_ABSENT
__device__ __forceinline__ uint32_t copy_lookup(const unsigned long long *__restrict__ keys, uint64_t smask, uint32_t max_probe, uint64_t key) {
    return key_find<uint32_t>(keys, smask, max_probe, key, SLOT_ABSENT);
}

// ---- a block's count: *dst += the sum of the four waves' n (every lane of a wave passes its wave's sum).  EVERY lane of the
// block must reach this call (a barrier), and a kernel calls it once (one static LDS array) ----
__device__ __forceinline__ void block_add(uint32_t n_per_wave, unsigned long long *dst) {
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n_per_wave;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (n) atomicAdd(dst, (unsigned long long)n);
    }
}

}  // namespace pg
