// pg_patterns.hip — the presence/absence pattern SPECTRUM of a finished bitmap's rows ON THE GPU (gfx950): which patterns
// occur in these rows at all, and how many rows does each hold?  (query_bitmap followed by DataFrame.value_counts(): the table
// an UpSet plot or a core / shell / private breakdown is drawn from, without nkmers x N bytes on the host.)
//
// The rule: `select` is a set of m genomes, 1 <= m <= 64, as ceil(N / 32) mask words.  The caller clears the words' bits at and
// past N, so the bits past N in a row's last byte never reach a key.  A row's KEY is a uint64: bit i of the key is the row's bit
// for the i-th selected genome, in ascending column order.  A window is a range [s, e) of SAMPLED rows of one contig, as in
// pg_find.hip: sampled row j is row j * stride of the contig's rows.  The result is ONE spectrum over all windows of the call:
// for every distinct key the number of sampled rows, over all windows, that have it; a row that two windows cover counts twice.
// No row outside a window is read.
//
// The host cuts every window into chunks of PATTERN_CHUNK consecutive sampled rows; chunk = {window, first sampled row}.
// grid = chunks (of all windows), 256 threads: a block takes its chunk tile by tile (256 sampled rows, one per lane).
//   key        FAST (the selected genomes are columns 0..m-1, the default of an index of up to 64 genomes): the row's first
//              min(8, nbytes) bytes zero-extended, cut to m bits.  Otherwise, per row word with a selected bit, every maximal
//              run of selected bits moves as one field (selection words staged in LDS; the loop is the same in every lane).
//   run heads  rows of similar genomes come in long runs of equal keys.  A lane is a HEAD if it is lane 0 of its wave or its
//              key differs from lane - 1's (one shuffle); its WEIGHT is the distance to the next head in the wave's ballot of
//              heads, cut at the wave's last valid row.  Lane 0 always being a head costs at most one extra insert per 64
//              rows and leaves nothing to carry between waves, tiles or chunks.
//   LDS table  heads add (key, weight) to the block's table of PAT_LSLOTS slots: open addressing, a 64-bit LDS
//              compare-and-swap claims a slot for a key, a 32-bit LDS add counts.  A head that finds no slot within PAT_LPROBE
//              probes goes straight to the global table.  No barrier inside the tile loop.
//   flush      at the chunk's end every claimed LDS slot goes to the global table: a 64-bit compare-and-swap claims the key's
//              slot (linear probing that wraps round the table; a plain look first — a slot only ever goes from empty to one
//              key, so whatever key a look sees is the slot's key for good, and a stale "empty" only leads to the
//              compare-and-swap that tells), a 64-bit add counts.  Both at agent scope: workgroups on different XCDs share the
//              table.  Claiming a fresh slot bumps ctr[0] (`placed`); a key that finds no slot in a full wrap adds its weight
//              to ctr[1] (`overflow`).
//   capacity   the table has at least 2 * cap slots.  `placed` only ever counts distinct keys, so a look that sees placed > cap
//              proves that the call ends as "exceeded" whatever else happens: from then on inserts are dropped and blocks
//              leave at once, which bounds the cost of a call whose capacity was too small.  While placed <= cap the table is
//              at most half full and no key is dropped, so distinct <= cap gives the exact spectrum and distinct > cap ends
//              with placed > cap, on every run.
//   sentinel   the all-ones word marks an empty slot.  With m < 64 it is no key.  With m = 64 it is the row every genome holds:
//              heads with that key add their weights to one LDS word, and the block adds it to ctr[2] once at the chunk's end;
//              the host appends it as the spectrum's last (largest) key.
// Counts are integers: the result does not depend on the order of the atomics.
#include "pg_kernels.h"
#include "pg_rowread.h"

namespace pg {

constexpr uint32_t PAT_TILE = 256;     // sampled rows per tile: one per lane
constexpr uint32_t PAT_LSLOTS = 1024;  // slots of a block's LDS table (12 KiB with the counts)
constexpr uint32_t PAT_LPROBE = 8;     // LDS slots a head tries before it goes to the global table
constexpr unsigned long long PAT_EMPTY = ~0ull;
static_assert(PATTERN_CHUNK % PAT_TILE == 0, "a chunk is a whole number of tiles");
static_assert((PAT_LSLOTS & (PAT_LSLOTS - 1)) == 0, "the LDS table is indexed by the hash's low bits");

// the key of the row at p under the selection words sel[ndw] (uniform: every lane walks the same fields)
__device__ __forceinline__ uint64_t pat_key_select(const uint8_t *__restrict__ p, uint32_t nbytes, uint32_t ndw, const uint32_t *sel) {
    uint64_t key = 0;
    uint32_t pos = 0;
    for (uint32_t d = 0; d < ndw; ++d) {
        uint32_t mk = sel[d];
        if (!mk) continue;
        const uint32_t w = row_word(p, d, nbytes);
        while (mk) {  // one maximal run of selected bits [b, b + len) per turn
            const uint32_t b = (uint32_t)__builtin_ctz(mk);
            const uint32_t t = ~(mk >> b);  // (0 only for b = 0 and a word of 32 selected bits)
            const uint32_t len = t ? (uint32_t)__builtin_ctz(t) : 32u;
            const uint64_t field = (1ull << len) - 1ull;
            key |= ((uint64_t)(w >> b) & field) << pos;  // (pos + len <= m <= 64, and pos < 64 here)
            pos += len;
            mk &= ~(uint32_t)(field << b);
        }
    }
    return key;
}

__device__ __forceinline__ uint64_t pat_hash(uint64_t k) {  // (the 64-bit finalizer of MurmurHash3)
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// counts[slot of key] += w in the global table of gmask + 1 slots; see "flush" and "capacity" above
__device__ __forceinline__ void pat_global_add(unsigned long long key, unsigned long long w, uint64_t h, unsigned long long *gkeys,
                                               unsigned long long *gcnt, uint64_t gmask, uint64_t cap, unsigned long long *ctr) {
    if (__hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap) return;
    uint64_t s = h & gmask;
    for (uint64_t probe = 0; probe <= gmask; ++probe, s = (s + 1) & gmask) {
        if ((probe & 31u) == 31u && __hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap) return;
        unsigned long long cur = __hip_atomic_load(&gkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == PAT_EMPTY) {
            if (__hip_atomic_compare_exchange_strong(&gkeys[s], &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_fetch_add(&ctr[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                cur = key;
            }  // (else cur holds the key that got there first)
        }
        if (cur == key) {
            __hip_atomic_fetch_add(&gcnt[s], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    __hip_atomic_fetch_add(&ctr[1], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool FAST>
__global__ __launch_bounds__(256) void k_pattern_counts(uint32_t N, const uint8_t *__restrict__ rows, uint32_t stride,
                                                        const uint64_t *__restrict__ base,
                                                        const uint64_t *__restrict__ ends, const uint2 *__restrict__ chunks,
                                                        const uint32_t *__restrict__ select, uint32_t m, uint64_t cap,
                                                        unsigned long long *gkeys, unsigned long long *gcnt, uint64_t gmask,
                                                        unsigned long long *ctr) {
    __shared__ unsigned long long lkeys[PAT_LSLOTS];
    __shared__ uint32_t lcnt[PAT_LSLOTS];
    __shared__ uint32_t lsel[PATTERN_MAX_GENOMES / 32];
    __shared__ uint32_t lones, lleave;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    for (uint32_t i = tid; i < PAT_LSLOTS; i += 256) {
        lkeys[i] = PAT_EMPTY;
        lcnt[i] = 0;
    }
    if (!FAST)
        for (uint32_t i = tid; i < ndw; i += 256) lsel[i] = select[i];
    if (tid == 0) {
        lones = 0;
        lleave = __hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap ? 1u : 0u;
    }
    __syncthreads();
    if (lleave) return;  // (the whole block: the call has exceeded its capacity already)
    const uint2 ck = chunks[blockIdx.x];
    const uint8_t *crow = rows + base[ck.x];
    const uint64_t e = ends[ck.x];
    const uint64_t c0 = ck.y, ce = min(c0 + (uint64_t)PATTERN_CHUNK, e);  // this chunk: sampled rows [c0, ce) of its window
    const uint64_t low = m >= 64 ? ~0ull : (1ull << m) - 1ull;
    for (uint64_t t0 = c0; t0 < ce; t0 += PAT_TILE) {
        const uint64_t j = t0 + tid;
        const bool valid = j < ce;
        uint64_t key = 0;
        if (valid) {
            const uint8_t *p = crow + j * stride * nbytes;
            key = FAST ? row_low(p, nbytes) & low : pat_key_select(p, nbytes, ndw, lsel);
        }
        const uint64_t before = __shfl_up((unsigned long long)key, 1);
        const bool head = valid && (lane == 0 || key != before);
        const uint64_t heads = __ballot(head);
        if (head) {
            const uint32_t nvalid = (uint32_t)min((uint64_t)64, ce - (t0 + (tid & ~63u)));  // valid rows of this wave: lanes 0..nvalid-1
            const uint64_t above = (heads >> lane) >> 1;
            const uint32_t w = above ? (uint32_t)__builtin_ctzll(above) + 1u : nvalid - lane;
            if (key == PAT_EMPTY) {  // (m = 64 only)
                atomicAdd(&lones, w);
            } else {
                const uint64_t h = pat_hash(key);
                uint32_t s = (uint32_t)(h >> 32) & (PAT_LSLOTS - 1);
                bool done = false;
                for (uint32_t probe = 0; probe < PAT_LPROBE && !done; ++probe, s = (s + 1) & (PAT_LSLOTS - 1)) {
                    const unsigned long long was = atomicCAS(&lkeys[s], PAT_EMPTY, (unsigned long long)key);
                    if (was == PAT_EMPTY || was == key) {
                        atomicAdd(&lcnt[s], w);
                        done = true;
                    }
                }
                if (!done) pat_global_add(key, w, h, gkeys, gcnt, gmask, cap, ctr);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < PAT_LSLOTS; i += 256) {
        const unsigned long long key = lkeys[i];
        if (key != PAT_EMPTY) pat_global_add(key, lcnt[i], pat_hash(key), gkeys, gcnt, gmask, cap, ctr);
    }
    if (tid == 0 && lones) __hip_atomic_fetch_add(&ctr[2], (unsigned long long)lones, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_pattern_counts(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, const uint64_t *base,
                                 const uint64_t *ends, const uint2 *chunks, uint32_t nchunks,
                                 const uint32_t *select, uint32_t nselected, bool low_columns, uint64_t cap,
                                 unsigned long long *keys, unsigned long long *counts, uint64_t slots, unsigned long long *ctr) {
    if (nchunks == 0) return hipSuccess;
    if (ngenomes < 1 || ngenomes > PATTERN_MAX_GENOMES || nselected < 1 || nselected > 64 || nselected > ngenomes)
        return hipErrorInvalidValue;
    if (slots < 2 || (slots & (slots - 1)) || slots < 2 * cap || !keys || !counts || !ctr || !select) return hipErrorInvalidValue;
    if (low_columns)
        hipLaunchKernelGGL((k_pattern_counts<true>), dim3(nchunks), dim3(256), 0, st, ngenomes, rows, stride, base, ends, chunks,
                           select, nselected, cap, keys, counts, slots - 1, ctr);
    else
        hipLaunchKernelGGL((k_pattern_counts<false>), dim3(nchunks), dim3(256), 0, st, ngenomes, rows, stride, base, ends, chunks,
                           select, nselected, cap, keys, counts, slots - 1, ctr);
    return hipGetLastError();
}

}  // namespace pg
