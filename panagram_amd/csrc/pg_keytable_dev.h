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
// the two folds a wave takes over its lanes before it touches a counter (equal slots, equal bins), and the sums of per-wave counts
// that a block adds to counters in HBM.
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

// ---- the folds of one wave.  Both are loops with wave-uniform bounds: every lane of the wave reaches the call, whatever its flag ----
// one value of lane `src`, in every lane (a 64-bit one takes two shuffles)
__device__ __forceinline__ uint32_t wave_read(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src); }
__device__ __forceinline__ uint64_t wave_read(uint64_t v, int src) {
    return (uint64_t)wave_read((uint32_t)v, src) | ((uint64_t)wave_read((uint32_t)(v >> 32), src) << 32);
}

// slots a wave folds before its lanes add for themselves (a satellite of period p: at most p)
constexpr uint32_t FOLD_TURNS = 8;

// add(id, n) for every distinct `id` among the lanes that are `on`, n the lanes that have it — the counter of a slot that many lanes
// hit gets ONE atomic, not one per lane (a homopolymer puts all 64 lanes on one slot, a satellite of period p on at most p:
// profiles/copies_rate.txt).  Turns: the first lane left takes every lane that has its id and adds their number.  A turn that finds
// its lane alone — ids scattered over the table — ends the folding, as turn TURNS does: the lanes left add 1 each.  A wave with no
// lane on does nothing.  id: 32 or 64 bits.
template <uint32_t TURNS = FOLD_TURNS, class Id, class Add>
__device__ __forceinline__ void wave_fold_add(bool on, Id id, uint32_t lane, Add add) {
    uint64_t todo = __ballot(on);
    for (uint32_t turn = 0; turn < TURNS && todo; ++turn) {
        const uint32_t first = (uint32_t)__builtin_ctzll(todo);
        const Id i0 = wave_read(id, (int)first);
        const uint64_t m = __ballot(on && id == i0);
        const uint32_t n = (uint32_t)__popcll(m);
        if (lane == first) add(i0, n);
        todo &= ~m;
        if (n == 1) break;
    }
    if ((todo >> lane) & 1ull) add(id, 1u);
}

// each(b, m) once per distinct `bin` among the wave's `act` lanes, m the ballot of the lanes that have it: one turn per bin, 64 at
// the most (depths along a gene are few).  each is called by the whole wave with the same (b, m) in every lane: it may take
// ballots of its own, and leaves its add to one lane.
template <class Each>
__device__ __forceinline__ void wave_fold_bins(bool act, uint32_t bin, Each each) {
    uint64_t todo = __ballot(act);
    while (todo) {
        const uint32_t b = wave_read(bin, (int)__builtin_ctzll(todo));
        const uint64_t m = __ballot(act && bin == b);
        each(b, m);
        todo &= ~m;
    }
}

// ---- a block's counts: dst[i] += the sum of the four waves' n[i] (every lane of a wave passes its wave's sums).  EVERY lane of
// the block must reach this call (a barrier), and a kernel calls it once (one static LDS array): its counters go in one call ----
template <uint32_t N>
__device__ __forceinline__ void block_add(const uint32_t (&n_per_wave)[N], unsigned long long *dst) {
    static_assert(N >= 1 && N <= 64, "thread i of the block adds counter i");
    __shared__ uint32_t wsum[N][4];
    if ((threadIdx.x & 63) == 0)
        for (uint32_t i = 0; i < N; ++i) wsum[i][threadIdx.x >> 6] = n_per_wave[i];
    __syncthreads();
    if (threadIdx.x < N) {
        const uint32_t n = wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
        if (n) atomicAdd(dst + threadIdx.x, (unsigned long long)n);
    }
}
__device__ __forceinline__ void block_add(uint32_t n_per_wave, unsigned long long *dst) {
    const uint32_t n[1] = {n_per_wave};
    block_add(n, dst);
}

}  // namespace pg
