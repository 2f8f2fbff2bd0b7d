// pg_runscan.h — the runs of one chunk of a contig's positions, for the kernels whose position has a 32-bit VALUE and whose runs
// are decided from a position's value and its predecessor's: the mate runs (pg_synteny.hip) and the hit runs (pg_locate.hip) call
// chunk_runs; the novel runs (pg_novel.hip) keep the same loop written out, for a measured reason given there.  Device code only;
// pg_runs_host.h is the host's half (the scans between the two passes).
//
// A chunk is positions [c0, min(c0 + CHUNK, nk)) of a contig of nk positions; a block of 256 threads takes it tile by tile (256
// positions, one per lane) in order.  Per tile:
//   value        a lane evaluates its position (load); a lane past the chunk's end has `none`.
//   predecessor  the value of the position before: from the lane below (a shuffle), for a wave's lane 0 from the wave below (LDS
//                last[4], written in front of the tile's FIRST barrier), for the tile's first lane from the tile before (carry =
//                last[3]), and at the chunk's first position from the caller's ONE evaluation of position c0 - 1, the chunk's halo
//                — `none` at a contig's first position, where nothing is evaluated.
//   edges        a run starts at a position, and ends (exclusive) at one, as the caller's edges(act, prev, cur) says: both
//                need the predecessor only, hence one halo position per chunk and none behind it.  The contig's last chunk adds
//                one end at nk when open(value of position nk - 1) — tail, written in front of the last tile's first barrier.
//   numbering    the waves' ballot counts go through LDS wcnt[4] behind the tile's SECOND barrier; a start's number is the
//                chunk's offset + the starts of the tiles before + of the waves below + of the lanes below, and the ends are
//                numbered the same way on their own: the i-th start and the i-th end of a contig are one run, so a run may begin
//                in one chunk and end in another without the chunks exchanging anything, and the output is sorted by (contig,
//                start) by construction — the same on every call.  An entry at or past `total` is never written.
// One LDS buffer each is enough: last is read between the two barriers and written again behind the second, wcnt is read behind
// the second and written again behind the next tile's first.  The tile loop's bounds are uniform over the block: every lane
// reaches both barriers, and EVERY lane of the block must reach the call.  A kernel calls it once (static LDS).
//
// Two passes, no block waits for another: count (EMIT false) returns the chunk's {tally a, starts, ends, tally b} for
// counts[chunk]; the host's runs_stitch turns those into the chunks' offsets; emit (EMIT true) evaluates again and stores.
//
// NOT for a kernel whose position is one BIT (k_find_runs of pg_find.hip, the absence runs of pg_gaps.hip): there a wave's ballot
// is a 64-row word, every lane scans the four waves' words, and the edges are word arithmetic (m & ~prev) — another skeleton,
// with one barrier per tile.  A new kernel over bits follows pg_find.hip; one over values calls chunk_runs.
#pragma once
#include <type_traits>

#include "pg_kernels.h"

namespace pg {

constexpr uint32_t RUNSCAN_TILE = 256;

struct no_tally {  // (the tally of a kernel that counts one thing only: its word of the chunk's counts stays 0)
    __device__ __forceinline__ bool operator()(uint32_t) const { return false; }
};

// Pos: the width the caller keeps positions in (32 bits where c0 + CHUNK cannot pass 2^32, 64 otherwise).
//   load(j)                       the value of position j, c0 <= j < the chunk's end
//   edges(act, prev, cur, starts, ends)   the two predicates — one functor: what they share is evaluated once.  act is false in
//                                 a lane past the chunk's end: BOTH must come out false there, and a functor that puts `act &&`
//                                 in front of what it evaluates keeps that lane out of it (as the kernels did before they shared
//                                 this loop: their assembly is what it was).  open(tail): whether a run reaches the contig's end
//   tally_a(cur), tally_b(cur)    what is counted beside the runs (no_tally: nothing)
//   put_start(at, j, prev, cur), put_end(at, j, prev, cur)   the stores of run number `at`; at the contig's end put_end(at, nk,
//                                 tail, none) from thread 0
// carry: the halo's value; off: the chunk's {starts, ends} before it (emit).
template <bool EMIT, uint32_t CHUNK, class Pos, class Load, class Edges, class Open, class TallyA, class TallyB, class PutStart,
          class PutEnd>
__device__ __forceinline__ uint4 chunk_runs(Pos c0, Pos nk, uint32_t none, uint32_t carry, ulonglong2 off, uint64_t total, Load load,
                                            Edges edges, Open open, TallyA tally_a, TallyB tally_b, PutStart put_start, PutEnd put_end) {
    static_assert(CHUNK % RUNSCAN_TILE == 0, "a chunk is a whole number of tiles");
    constexpr bool HAS_B = !std::is_same<TallyB, no_tally>::value;
    __shared__ uint32_t last[4];  // the value of every wave's last lane
    __shared__ uint4 wcnt[4];     // {starts, ends, tally a, tally b} of every wave
    __shared__ uint32_t tail;     // the value of the chunk's last position
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Pos ce = min((Pos)(c0 + CHUNK), nk);  // this chunk: positions [c0, ce), 0 <= c0 < ce <= nk
    uint32_t na = 0, nb = 0, nstarts = 0, nends = 0;
    for (Pos t0 = c0; t0 < ce; t0 += RUNSCAN_TILE) {
        const Pos j = t0 + tid;
        const bool act = j < ce;
        const uint32_t cur = act ? load(j) : none;
        if (lane == 63) last[wave] = cur;
        if (j == ce - 1) tail = cur;
        __syncthreads();
        uint32_t prev = (uint32_t)__shfl_up((int)cur, 1);
        if (lane == 0) prev = wave ? last[wave - 1] : carry;
        carry = last[3];
        bool starts, ends;
        edges(act, prev, cur, starts, ends);
        const uint64_t sm = __ballot(starts);
        const uint64_t em = __ballot(ends);
        const uint64_t am = __ballot(act && tally_a(cur));
        const uint64_t bm = __ballot(act && tally_b(cur));
        if (lane == 0) wcnt[wave] = make_uint4((uint32_t)__popcll(sm), (uint32_t)__popcll(em), (uint32_t)__popcll(am), (uint32_t)__popcll(bm));
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
            na += c.z;
            if (HAS_B) nb += c.w;
        }
        if (EMIT) {
            const uint64_t below = (1ull << lane) - 1ull;
            if ((sm >> lane) & 1ull) {
                const uint64_t at = off.x + nstarts + sbelow + (uint32_t)__popcll(sm & below);
                if (at < total) put_start(at, j, prev, cur);
            }
            if ((em >> lane) & 1ull) {
                const uint64_t at = off.y + nends + ebelow + (uint32_t)__popcll(em & below);
                if (at < total) put_end(at, j, prev, cur);
            }
        }
        nstarts += stile;
        nends += etile;
    }
    // the contig's last chunk: a run that reaches the contig's last position ends at nk (every lane has passed the barrier
    // behind tail's write)
    if (ce == nk && open(tail)) {
        if (EMIT && tid == 0) {
            const uint64_t at = off.y + nends;
            if (at < total) put_end(at, nk, tail, none);
        }
        nends += 1;
    }
    return make_uint4(na, nstarts, nends, nb);
}

}  // namespace pg
