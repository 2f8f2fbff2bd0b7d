// pg_novel.hip — WHAT does a sample hold that no indexed genome does (gfx950)?  pg_screen.hip counts a sample per slot of the pan
// table: what of the index the sample holds.  This unit is the reverse: the sample's windows that MISS the pan table go into a
// key table of their own, built while the sample streams and grown between sequence sets, with a 32-bit depth beside every key;
// one pass over that table gives the distinct novel k-mers, the solid ones among them and the depth spectrum; and for an
// assembly the runs of novel positions along its contigs say where the novel sequence lies.
//
// Definitions (tests/novel_ref.py is the same in numpy):
//   valid window   as everywhere: a window holding a non-ACGT base does not exist, a contig shorter than k has none.
//   novel key      the canonical key of a valid window of the sample that the pan table does not hold.  depth(key) = the valid
//                  windows of the sample with that key — both strands, every set added since the table was created or cleared —
//                  exact in 32 bits (the host holds a handle below 2^32 windows).  solid: depth >= min_count.
//   novel run      a maximal [a, b) of consecutive valid k-mer positions of ONE contig whose keys are all novel: contig ends and
//                  invalid windows cut runs.  left_held = position a - 1 exists, is valid and the pan table holds its key;
//                  right_held the same of position b.
//
// The novel table: `nslots` (a power of two, at most COPIES_MAX_SLOTS) 8-byte keys — a key table, laid out and walked as
// pg_keytable_dev.h says — and beside them nslots u32 depths.  The host keeps its load at or below 0.5 by growing it BEFORE a
// launch, so no claim runs out of probes; one that does raises the overflow flag all the same.
//   k_novel_count  one launch over the (contig, piece) jobs of a sequence set, the pan table read-only.  A valid window probes the
//                  pan table (lane_find); a miss claims its key's slot in the novel table (key_claim) and adds 1 to the slot's
//                  depth.  Equal slots are folded inside the wave first (wave_fold_add, pg_keytable_dev.h).  A wave without a
//                  miss skips the claim and the fold.  ctr: the valid windows, the pan hits, the keys newly claimed, the claims
//                  that gave up — a ballot per wave, one atomic per block each (one block_add of four counters).
//   k_novel_grow   one lane per slot of the old table: its key claimed in the new one (twice the slots or more), its depth copied
//                  by a plain store — a key stands once in the old table, so every new slot has one writer.
//   k_novel_scan   one pass over the slots and their depths, a run of consecutive slots per block (novel_scan_per_block).  Count: nkeys, solid,
//                  solid_windows (the sum of the solid depths, 64 bits) and depth_hist[64] by min(d, 63) — the histogram folded
//                  per wave (wave_fold_bins, pg_keytable_dev.h) into the block's counters in LDS, which are flushed once per
//                  block — and the solid keys of every block's slots.  Emit, after the host's exclusive scan of
//                  those: the solid keys and their depths in slot order, the same on every call.
//   k_novel_runs   the run scan that pg_runscan.h describes (its loop written out here, for its speed) over chunks of NOVEL_CHUNK
//                  positions of one contig; a position's value is its state, one of invalid, held, novel (a probe of the pan
//                  table; the novel table is not touched), the halo ONE extra probe of position c0 - 1.  With V = novel, P =
//                  predecessor novel:
//                    run starts  V & ~P  (left_held: the predecessor is held)     run ends (exclusive)  P & ~V  (right_held:
//                    this position is held), and one at the contig's end when its last is novel
//                  counts[chunk] = {valid, starts, ends, novel}.
// Every write to HBM is a vector store or a vector atomic.
#include "pg_kernels.h"
#include "pg_keytable_dev.h"  // contig_view, window_valid, copy_key, key_claim, the wave folds, block_add
#include "pg_runscan.h"  // what k_novel_runs' loop is a copy of; RUNSCAN_TILE

namespace pg {

static_assert(NOVEL_CHUNK % RUNSCAN_TILE == 0, "a chunk is a whole number of tiles");
constexpr uint32_t NOVEL_SCAN_UNROLL = 8;  // tiles of k_novel_scan whose loads are in flight together
static_assert(NOVEL_SCAN_SLOTS % (256 * NOVEL_SCAN_UNROLL) == 0, "a block's slots are a whole number of tile groups");
static_assert(NOVEL_BINS == 64, "one bin per lane of a wave");

// job = positions [y * NOVEL_JOB, (y + 1) * NOVEL_JOB) of contig x, which holds at least k bases
__global__ __launch_bounds__(256) void k_novel_count(SubTable st, int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                     const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                     unsigned long long *keys, uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                                                     unsigned long long *ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint2 job = jobs[blockIdx.x];
    const ContigView v = contig_view(sd, job.x, seqw_all, nmw_all, has_n, k);
    const uint64_t p0 = (uint64_t)job.y * NOVEL_JOB, p1 = min(v.nkmers, p0 + NOVEL_JOB);
    const uint64_t smask = nslots - 1;
    uint32_t nvalid = 0, found = 0, nclaimed = 0, ngaveup = 0;  // (per wave)
    for (uint64_t q = p0; q < p1; q += 256) {  // (bounds uniform over the block)
        const uint64_t p = q + threadIdx.x;
        const bool valid = p < p1 && window_valid(v, p, k);
        const uint64_t key = valid ? copy_key(v.seqw, p, k) : 0ull;
        uint32_t line = 0, pslot = 0;
        const bool hit = valid && lane_find(st, key, line, pslot);
        nvalid += (uint32_t)__popcll(__ballot(valid));
        found += (uint32_t)__popcll(__ballot(hit));
        const bool miss = valid && !hit;
        if (__ballot(miss) == 0) continue;  // (wave-uniform)
        bool claimed = false;
        const uint64_t s64 = miss ? key_claim(keys, smask, max_probe, key, claimed) : KEY_ABSENT;
        const bool ok = s64 != KEY_ABSENT;
        const uint32_t slot = (uint32_t)s64;  // (below 2^31: COPIES_MAX_SLOTS)
        nclaimed += (uint32_t)__popcll(__ballot(claimed));
        ngaveup += (uint32_t)__popcll(__ballot(miss && !ok));
        wave_fold_add(ok, slot, lane, [&](uint32_t s, uint32_t n) { atomicAdd(&depth[s], n); });
    }
    const uint32_t sums[4] = {nvalid, found, nclaimed, ngaveup};
    block_add(sums, ctr);
}

// slot i of the old table into the new one; flag[0] becomes nonzero when a claim gave up
__global__ __launch_bounds__(256) void k_novel_grow(const unsigned long long *__restrict__ old_keys, const uint32_t *__restrict__ old_depth,
                                                    uint64_t old_slots, unsigned long long *keys, uint32_t *depth, uint64_t nslots,
                                                    uint32_t max_probe, unsigned long long *flag) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= old_slots) return;
    const unsigned long long key = old_keys[i];
    if (key == EMPTY_KEY) return;
    bool claimed = false;
    const uint64_t s = key_claim(keys, nslots - 1, max_probe, key, claimed);
    if (s == KEY_ABSENT)
        atomicOr(reinterpret_cast<unsigned int *>(flag), 1u);
    else
        depth[s] = old_depth[i];
}

// block b: slots [b * per, (b + 1) * per), per = novel_scan_per_block(nslots), cut at nslots — at most NOVEL_SCAN_BLOCKS blocks: every
// block ends in atomics on the same few words of `out`, and 131 072 blocks of 4096 slots took 6.43 ms over a table of 2^29 slots that
// 2048 blocks pass over in 1.06 ms, the time a plain reduction streams as many bytes in (profiles/novel_rate.txt: the A/B).
//   EMIT false  out (zeroed by the caller, accumulated into): nkeys, solid, solid_windows, depth_hist [64]; block_solid[b] = the
//               block's solid keys
//   EMIT true   offs[b] = the solid keys of all blocks before b; key and depth of the solid slots, in slot order, to out_keys /
//               out_depth from there on (entries at or past cap are never written)
template <bool EMIT>
__global__ __launch_bounds__(256) void k_novel_scan(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ depth,
                                                    uint64_t nslots, uint32_t min_count, unsigned long long *__restrict__ out,
                                                    uint32_t *__restrict__ block_solid, const uint64_t *__restrict__ offs, uint64_t cap,
                                                    unsigned long long *__restrict__ out_keys, uint32_t *__restrict__ out_depth) {
    __shared__ uint32_t hist_s[NOVEL_BINS];
    __shared__ uint32_t nkeys_s, solid_s;
    __shared__ unsigned long long sw_s;
    __shared__ uint32_t wsolid[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t per = novel_scan_per_block(nslots), s0 = (uint64_t)blockIdx.x * per, s1 = min(nslots, s0 + per);
    if (!EMIT) {
        if (tid < NOVEL_BINS) hist_s[tid] = 0;
        if (tid == 0) {
            nkeys_s = solid_s = 0;
            sw_s = 0;
        }
        __syncthreads();
    }
    uint32_t nk = 0, ns = 0;         // (per wave)
    unsigned long long sw = 0;       // this lane's solid depths
    uint64_t at0 = EMIT ? offs[blockIdx.x] : 0;  // where the tile's first solid key goes
    // NOVEL_SCAN_UNROLL tiles at a time: their keys are loaded before the first is looked at, then the depths of the slots that
    // hold one — a wave has that many loads in flight, not one
    for (uint64_t g0 = s0; g0 < s1; g0 += 256 * NOVEL_SCAN_UNROLL) {  // (bounds uniform over the block: every lane reaches the barriers)
        unsigned long long gkey[NOVEL_SCAN_UNROLL];
        uint32_t gd[NOVEL_SCAN_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < NOVEL_SCAN_UNROLL; ++u) {
            const uint64_t s = g0 + 256 * u + tid;
            gkey[u] = s < s1 ? keys[s] : EMPTY_KEY;
        }
#pragma unroll
        for (uint32_t u = 0; u < NOVEL_SCAN_UNROLL; ++u) gd[u] = gkey[u] != EMPTY_KEY ? depth[g0 + 256 * u + tid] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < NOVEL_SCAN_UNROLL; ++u) {
            const unsigned long long key = gkey[u];
            const bool act = key != EMPTY_KEY;
            const uint32_t d = gd[u];
            const bool solid = act && d >= min_count;
            const uint64_t sm = __ballot(solid);
            if (EMIT) {
                if (lane == 0) wsolid[wave] = (uint32_t)__popcll(sm);
                __syncthreads();
                uint32_t below = 0, tile = 0;
#pragma unroll
                for (uint32_t w = 0; w < 4; ++w) {
                    if (w == wave) below = tile;
                    tile += wsolid[w];
                }
                if (solid) {
                    const uint64_t at = at0 + below + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
                    if (at < cap) {
                        out_keys[at] = key;
                        out_depth[at] = d;
                    }
                }
                at0 += tile;
                __syncthreads();  // (wsolid is read before the next tile writes it)
            } else {
                const uint64_t am = __ballot(act);
                if (am == 0) continue;  // (wave-uniform)
                nk += (uint32_t)__popcll(am);
                ns += (uint32_t)__popcll(sm);
                if (solid) sw += d;
                // the depth bins: one turn per distinct bin among the wave's keys, 64 at the most
                const uint32_t bin = min(d, NOVEL_BINS - 1);
                wave_fold_bins(act, bin, [&](uint32_t b, uint64_t m) {
                    if (lane == 0) atomicAdd(&hist_s[b], (uint32_t)__popcll(m));
                });
            }
        }
    }
    if (!EMIT) {
        // the wave's sum of solid depths: halved six times
        for (int off = 32; off; off >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)sw, off), hi = (uint32_t)__shfl_down((int)(uint32_t)(sw >> 32), off);
            sw += (unsigned long long)lo | ((unsigned long long)hi << 32);
        }
        if (lane == 0) {
            if (nk) atomicAdd(&nkeys_s, nk);
            if (ns) atomicAdd(&solid_s, ns);
            if (sw) atomicAdd(&sw_s, sw);
        }
        __syncthreads();
        if (tid < NOVEL_BINS && hist_s[tid]) atomicAdd(&out[3 + tid], (unsigned long long)hist_s[tid]);
        if (tid == 64) {
            if (nkeys_s) atomicAdd(&out[0], (unsigned long long)nkeys_s);
            if (solid_s) atomicAdd(&out[1], (unsigned long long)solid_s);
            if (sw_s) atomicAdd(&out[2], sw_s);
            block_solid[blockIdx.x] = solid_s;
        }
    }
}

// the state of position p of a contig (p below its k-mer positions)
constexpr uint32_t NS_INVALID = 0, NS_HELD = 1, NS_NOVEL = 2;
__device__ __forceinline__ uint32_t novel_state(const SubTable &st, int k, const ContigView v, uint64_t p) {
    if (!window_valid(v, p, k)) return NS_INVALID;
    uint32_t line, slot;
    return lane_find(st, copy_key(v.seqw, p, k), line, slot) ? NS_HELD : NS_NOVEL;
}

// chunk = {contig, first position}: a contig of at least k bases, 0 <= first position < its k-mer positions.
// chunk_runs' loop (pg_runscan.h), written out: through chunk_runs this kernel took 1.794 ms against 1.747 ms over an assembly of
// 100 Mb on the MI355X (profiles/stream_refactor_ab.txt: the probe's scalar registers are at their limit, and the inlined functors
// spill more of them).  A change to the run scan comes here too.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_novel_runs(SubTable st, int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ chunks,
                                                    const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                    uint4 *__restrict__ counts, const ulonglong2 *__restrict__ offs, uint64_t total,
                                                    uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_end,
                                                    uint8_t *__restrict__ left_held, uint8_t *__restrict__ right_held) {
    __shared__ uint32_t lasts[4];  // the state of every wave's last lane
    __shared__ uint4 wcnt[4];      // {starts, ends, valid, novel} of every wave
    __shared__ uint32_t tails;     // the state of the chunk's last position
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint2 ck = chunks[blockIdx.x];
    const ContigView v = contig_view(sd, ck.x, seqw_all, nmw_all, has_n, k);
    // this chunk: positions [c0, ce), 0 <= c0 < ce <= nk <= 2^32 - 1 (64-bit: c0 + NOVEL_CHUNK may pass 2^32)
    const uint64_t nk = v.nkmers, c0 = ck.y, ce = min(c0 + NOVEL_CHUNK, nk);
    // the chunk's halo: the state of position c0 - 1 (every lane the same probe: broadcast loads)
    uint32_t carry = c0 > 0 ? novel_state(st, k, v, c0 - 1) : NS_INVALID;
    uint32_t nvalid = 0, nnovel = 0, nstarts = 0, nends = 0;
    uint64_t soff = 0, eoff = 0;
    if (EMIT) {
        const ulonglong2 o = offs[blockIdx.x];
        soff = o.x;
        eoff = o.y;
    }
    for (uint64_t t0 = c0; t0 < ce; t0 += RUNSCAN_TILE) {  // (bounds uniform over the block: every lane reaches the barriers)
        const uint64_t j = t0 + tid;
        const bool act = j < ce;
        const uint32_t s = act ? novel_state(st, k, v, j) : NS_INVALID;
        if (lane == 63) lasts[wave] = s;
        if (j == ce - 1) tails = s;
        __syncthreads();
        uint32_t prev = (uint32_t)__shfl_up((int)s, 1);
        if (lane == 0) prev = wave ? lasts[wave - 1] : carry;
        carry = lasts[3];
        const uint64_t sm = __ballot(act && s == NS_NOVEL && prev != NS_NOVEL);
        const uint64_t em = __ballot(act && prev == NS_NOVEL && s != NS_NOVEL);
        const uint64_t vm = __ballot(act && s != NS_INVALID), nm = __ballot(act && s == NS_NOVEL);
        if (lane == 0) wcnt[wave] = make_uint4((uint32_t)__popcll(sm), (uint32_t)__popcll(em), (uint32_t)__popcll(vm), (uint32_t)__popcll(nm));
        __syncthreads();
        uint32_t sbelow = 0, ebelow = 0, stile = 0, etile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint4 c = wcnt[w];
            if (w == wave) {
                sbelow = stile;
                ebelow = etile;
            }
            stile += c.x;
            etile += c.y;
            nvalid += c.z;
            nnovel += c.w;
        }
        if (EMIT) {
            const uint64_t below = (1ull << lane) - 1ull;
            if ((sm >> lane) & 1ull) {
                const uint64_t at = soff + nstarts + sbelow + (uint32_t)__popcll(sm & below);
                if (at < total) {
                    run_start[at] = (uint32_t)j;
                    left_held[at] = prev == NS_HELD ? 1 : 0;
                }
            }
            if ((em >> lane) & 1ull) {
                const uint64_t at = eoff + nends + ebelow + (uint32_t)__popcll(em & below);
                if (at < total) {
                    run_end[at] = (uint32_t)j;
                    right_held[at] = s == NS_HELD ? 1 : 0;
                }
            }
        }
        nstarts += stile;
        nends += etile;
    }
    // the contig's last chunk: a run that reaches the contig's last position ends at nk
    if (ce == nk && tails == NS_NOVEL) {
        if (EMIT && tid == 0) {
            const uint64_t at = eoff + nends;
            if (at < total) {
                run_end[at] = (uint32_t)nk;
                right_held[at] = 0;
            }
        }
        nends += 1;
    }
    if (!EMIT && tid == 0) counts[blockIdx.x] = make_uint4(nvalid, nstarts, nends, nnovel);
}

static bool pan_ok(const SubTable &t) { return t.k >= 1 && t.k <= 32 && t.nbuckets != 0 && t.slots >= 1 && t.slots <= 64 && t.buckets; }
static bool novel_ok(uint64_t nslots, const void *keys, const void *depth) {
    return nslots != 0 && !(nslots & (nslots - 1)) && nslots <= COPIES_MAX_SLOTS && keys && depth;
}

hipError_t launch_novel_count(hipStream_t st, const SubTable &t, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                              const uint32_t *nmw, const uint32_t *has_n, unsigned long long *keys, uint32_t *depth, uint64_t nslots,
                              uint32_t max_probe, unsigned long long *ctr) {
    if (njobs == 0) return hipSuccess;
    if (!pan_ok(t) || !novel_ok(nslots, keys, depth) || !ctr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_novel_count, dim3(njobs), dim3(256), 0, st, t, (int)t.k, sd, jobs, seqw, nmw, has_n, keys, depth, nslots, max_probe,
                       ctr);
    return hipGetLastError();
}

hipError_t launch_novel_grow(hipStream_t st, const unsigned long long *old_keys, const uint32_t *old_depth, uint64_t old_slots,
                             unsigned long long *keys, uint32_t *depth, uint64_t nslots, uint32_t max_probe, unsigned long long *flag) {
    if (!novel_ok(old_slots, old_keys, old_depth) || !novel_ok(nslots, keys, depth) || nslots < 2 * old_slots || !flag)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_novel_grow, dim3((uint32_t)((old_slots + 255) / 256)), dim3(256), 0, st, old_keys, old_depth, old_slots, keys, depth,
                       nslots, max_probe, flag);
    return hipGetLastError();
}

hipError_t launch_novel_scan(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t min_count,
                             unsigned long long *out, uint32_t *block_solid, const uint64_t *offs, uint64_t cap,
                             unsigned long long *out_keys, uint32_t *out_depth) {
    const bool emit = offs != nullptr;
    if (!novel_ok(nslots, keys, depth) || min_count < 1 || (emit ? (!out_keys || !out_depth) : (!out || !block_solid)))
        return hipErrorInvalidValue;
    const uint32_t blocks = novel_scan_blocks(nslots);
    if (emit)
        hipLaunchKernelGGL(k_novel_scan<true>, dim3(blocks), dim3(256), 0, st, keys, depth, nslots, min_count, out, block_solid, offs, cap,
                           out_keys, out_depth);
    else
        hipLaunchKernelGGL(k_novel_scan<false>, dim3(blocks), dim3(256), 0, st, keys, depth, nslots, min_count, out, block_solid, offs, cap,
                           out_keys, out_depth);
    return hipGetLastError();
}

hipError_t launch_novel_runs(hipStream_t st, const SubTable &t, const SeqDesc *sd, const uint2 *chunks, uint32_t nchunks, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, uint4 *counts, const ulonglong2 *offs, uint64_t total,
                             uint32_t *run_start, uint32_t *run_end, uint8_t *left_held, uint8_t *right_held) {
    if (nchunks == 0) return hipSuccess;
    const bool emit = offs != nullptr;
    if (!pan_ok(t) || !sd || !chunks || !seqw || !nmw || !has_n || (emit ? (!run_start || !run_end || !left_held || !right_held) : !counts))
        return hipErrorInvalidValue;
    if (emit)
        hipLaunchKernelGGL(k_novel_runs<true>, dim3(nchunks), dim3(256), 0, st, t, (int)t.k, sd, chunks, seqw, nmw, has_n, counts, offs, total,
                           run_start, run_end, left_held, right_held);
    else
        hipLaunchKernelGGL(k_novel_runs<false>, dim3(nchunks), dim3(256), 0, st, t, (int)t.k, sd, chunks, seqw, nmw, has_n, counts, offs, total,
                           run_start, run_end, left_held, right_held);
    return hipGetLastError();
}

}  // namespace pg
