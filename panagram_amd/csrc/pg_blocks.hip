// pg_blocks.hip — the runs of pg_synteny.hip chained into gap-tolerant BLOCKS (gfx950): a block bridges substitutions and small
// insertions and deletions, and a stray unique match elsewhere in B does not break it.  The runs stay in HBM, only blocks leave.
//
// Definitions (tests/blocks_ref.py is the same in numpy):
//   run          what k_mate_runs emits: the contig c of A, k-mer positions [s, e) of that contig, n = e - s, the mate word m of
//                position s, the strand σ = m & 1, b = m >> 1.  The B position of the run's last k-mer is bl = b + (n - 1) on
//                strand 0 and bl = b - (n - 1) on strand 1; its mate word is ml = bl << 1 | σ.  Runs are sorted by (c, s).
//   kept         a run with n >= min_run.  Dropped runs do not exist for anything below.
//   predecessor  of a kept run j: the nearest kept run i before it in the same contig of A, any number of dropped runs between.
//   link i -> j  dA = s_j - (e_i - 1), always >= 1; dB = b_j - bl_i on strand 0, bl_i - b_j on strand 1; signed, in 64-bit
//                arithmetic.  The link exists iff  σ_i == σ_j,  1 <= dA <= max_gap,  1 <= dB <= max_gap,  |dA - dB| <= max_shift,
//                and the global B positions bl_i and b_j lie in the same contig of B.
//                A substitution gives dA = dB = k + 1; an insertion of L bases in B dA = k, dB = k + L; a deletion of d bases
//                from B dA = k + d, dB = k.
//   same/shifted a link is same when dA == dB, shifted otherwise.
//   block        a maximal chain of kept runs, each linked to its predecessor.  Its fields: the contig of A, start = s of the first
//                run, end = e of the last, mate_first = m of the first run, mate_last = ml of the last, kmers = the sum of n over
//                its runs, runs = their number, shifted = its shifted links.  Blocks are sorted by (contig, start), the same on
//                every call.  dB >= 1 makes B monotone inside a block: its B range is [mate_first >> 1, (mate_last >> 1) + k) on
//                strand 0 and [mate_last >> 1, (mate_first >> 1) + k) on strand 1.
//   With min_run = 1 and max_gap = 1 the blocks are exactly the runs (a link with dA = dB = 1 would be one run).
//
// k_run_blocks<EMIT> has the structure of k_mate_runs and k_find_runs: chunks of RUN_CHUNK runs of one contig of A, tiles of 256,
// waves of 64, one run per lane.  The predecessor is the LAST KEPT run before the lane, not the lane below: inside a wave the
// highest set bit of the kept-ballot below the lane and a shuffle from that lane; below the wave the last kept run of the waves
// before it in the tile (LDS), then of the tiles before (a register every lane holds).  A chunk takes no halo: the predecessor
// of its first kept run may lie any number of chunks back.
//   count (EMIT = false)  per chunk a BlockChunkCount (pg_blocks_link.h); the chunk's first kept run is left undecided.
//   host                  blocks_stitch (pg_blocks_host.h) decides it with the same blocks_link and scans the counts.
//   emit                  starts and ends are numbered separately: the i-th start and the i-th end of a contig are one block.  A
//                         kept run without a link writes the START record of its block {s, m, and the contig's sums over the kept
//                         runs before it: k-mers, runs, shifted links} and, when it has a predecessor, the END record of the
//                         block before {e, ml of the predecessor, the same three sums}; the contig's last kept run ends the last
//                         block at the contig's last chunk.  kmers, runs and shifted of a block are end record - start record.
// No atomics, no unbounded loop (the tile loop runs over a chunk, blocks_rank halves at most 32 times), every barrier is reached
// by every lane, every write to HBM is a vector store.
#include "pg_kernels.h"

#include "pg_blocks_pred.h"

namespace pg {

constexpr uint32_t RUN_TILE = 256;
static_assert(RUN_CHUNK % RUN_TILE == 0, "a chunk is a whole number of tiles");

// contigs[c] = {first run of contig c in the run arrays, its runs}; chunk = {contig, first run inside the contig}.  out: 10
// planes of `total` entries — start, mate_first, and the three sums of the start records; end, mate_last and those of the ends.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_run_blocks(const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ run_end,
                                                    const uint32_t *__restrict__ run_mate, const uint2 *__restrict__ contigs,
                                                    const uint2 *__restrict__ chunks, const uint64_t *__restrict__ boff, uint32_t nb,
                                                    uint32_t min_run, uint32_t max_gap, uint32_t max_shift,
                                                    BlockChunkCount *__restrict__ counts, const BlockChunkOffs *__restrict__ offs,
                                                    uint64_t total, uint32_t *__restrict__ out) {
    __shared__ uint2 wlast[4];   // {e, ml} of every wave's last kept run (ml BLOCKS_NONE: the wave has none)
    __shared__ uint2 wfirst[4];  // {s, m} of every wave's first kept run (read only where wlast says there is one)
    __shared__ uint4 wcnt[4];    // {starts, ends, kept, shifted links} of every wave
    __shared__ uint32_t wkm[4];  // the k-mers of every wave's kept runs
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint2 ck = chunks[blockIdx.x];
    const uint2 cd = contigs[ck.x];
    const uint32_t *rs = run_start + cd.x, *re = run_end + cd.x, *rm = run_mate + cd.x;
    const uint32_t nr = cd.y, c0 = ck.y, ce = min(c0 + RUN_CHUNK, nr);  // this chunk: runs [c0, ce) of the contig, c0 < ce <= nr
    uint32_t carry_e = 0, carry_ml = BLOCKS_NONE;  // the last kept run before the tile (count: inside the chunk only)
    uint32_t nstarts = 0, nends = 0, kept_n = 0, kmers = 0, shifted_n = 0;  // of the tiles before
    uint32_t first_s = 0, first_m = 0;
    bool have_first = false;
    uint64_t soff = 0, eoff = 0;
    if (EMIT) {
        const BlockChunkOffs o = offs[blockIdx.x];
        soff = o.soff;
        eoff = o.eoff;
        kmers = o.kmers;
        kept_n = o.runs;
        shifted_n = o.shifted;
        carry_e = o.carry_e;
        carry_ml = o.carry_ml;
    }
    for (uint32_t t0 = c0; t0 < ce; t0 += RUN_TILE) {  // (bounds uniform over the block)
        const uint32_t j = t0 + tid;
        const bool act = j < ce;
        const uint32_t s = act ? rs[j] : 0u, e = act ? re[j] : 1u, m = act ? rm[j] : 0u;
        const uint32_t n = e - s;
        const bool kept = act && n >= min_run;
        const uint32_t ml = blocks_last_mate(m, n);
        // the last kept run before the lane (pg_blocks_pred.h: one barrier inside)
        const RunPred pr = blocks_pred<!EMIT>(kept, s, e, m, ml, wlast, wfirst, carry_e, carry_ml, first_s, first_m, have_first);
        const uint64_t kb = pr.kb, kbelow = pr.kbelow, below = (1ull << lane) - 1ull;
        const uint32_t pe = pr.pe, pml = pr.pml;
        bool shifted = false;
        const bool link = kept && blocks_link(pe, pml, s, m, max_gap, max_shift, boff, nb, &shifted);
        const bool pred = pml != BLOCKS_NONE;
        const bool start = kept && !link && (EMIT || pred);  // (count: the chunk's first kept run is the host's to decide)
        const uint64_t sm = __ballot(start);
        const uint64_t em = __ballot(start && pred);
        const uint64_t hm = __ballot(link && shifted);
        // the k-mers of the kept runs up to and with this lane (n <= 2^31 - 1 in a contig: the sums of one contig do not wrap)
        uint32_t kin = kept ? n : 0u;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)kin, d);
            if (lane >= d) kin += up;
        }
        if (lane == 63) wkm[wave] = kin;
        if (lane == 0) wcnt[wave] = make_uint4((uint32_t)__popcll(sm), (uint32_t)__popcll(em), (uint32_t)__popcll(kb), (uint32_t)__popcll(hm));
        __syncthreads();
        // (one buffer each: wlast and wfirst are read between the two barriers and written again behind the second, wcnt and wkm
        // are read behind the second and written again behind the next tile's first)
        uint4 under = make_uint4(0u, 0u, 0u, 0u), tile = make_uint4(0u, 0u, 0u, 0u);
        uint32_t kunder = 0, ktile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint4 c = wcnt[w];
            if (w == wave) under = tile, kunder = ktile;
            tile.x += c.x, tile.y += c.y, tile.z += c.z, tile.w += c.w;
            ktile += wkm[w];
        }
        if (EMIT && ((sm >> lane) & 1ull)) {
            // the contig's sums over the kept runs before this one; a start has no link, so `shifted` at it and before it agree
            const uint32_t pk = kmers + kunder + kin - n;
            const uint32_t prn = kept_n + under.z + (uint32_t)__popcll(kbelow);
            const uint32_t ps = shifted_n + under.w + (uint32_t)__popcll(hm & below);
            const uint64_t at = soff + nstarts + under.x + (uint32_t)__popcll(sm & below);
            if (at < total) {
                out[at] = s;
                out[total + at] = m;
                out[2 * total + at] = pk;
                out[3 * total + at] = prn;
                out[4 * total + at] = ps;
            }
            if (pred) {
                const uint64_t ea = eoff + nends + under.y + (uint32_t)__popcll(em & below);
                if (ea < total) {
                    out[5 * total + ea] = pe;
                    out[6 * total + ea] = pml;
                    out[7 * total + ea] = pk;
                    out[8 * total + ea] = prn;
                    out[9 * total + ea] = ps;
                }
            }
        }
        nstarts += tile.x;
        nends += tile.y;
        kept_n += tile.z;
        shifted_n += tile.w;
        kmers += ktile;
    }
    if (tid != 0) return;  // (behind the last barrier)
    if (EMIT) {
        // the contig's last chunk: its last kept run, in this chunk or before it, ends the contig's last block
        if (ce == nr && carry_ml != BLOCKS_NONE) {
            const uint64_t ea = eoff + nends;
            if (ea < total) {
                out[5 * total + ea] = carry_e;
                out[6 * total + ea] = carry_ml;
                out[7 * total + ea] = kmers;
                out[8 * total + ea] = kept_n;
                out[9 * total + ea] = shifted_n;
            }
        }
    } else {
        BlockChunkCount c;
        c.kept = kept_n, c.starts = nstarts, c.kmers = kmers, c.shifted = shifted_n;
        c.first_s = first_s, c.first_m = first_m, c.last_e = carry_e, c.last_ml = carry_ml;
        counts[blockIdx.x] = c;
    }
}

hipError_t launch_run_blocks(hipStream_t st, const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate,
                             const uint2 *contigs, const uint2 *chunks, uint32_t nchunks, const uint64_t *boff, uint32_t nb,
                             uint32_t min_run, uint32_t max_gap, uint32_t max_shift, BlockChunkCount *counts,
                             const BlockChunkOffs *offs, uint64_t total, uint32_t *out) {
    if (nchunks == 0) return hipSuccess;
    const bool emit = offs != nullptr;
    if (!run_start || !run_end || !run_mate || !contigs || !chunks || !boff || min_run < 1 || max_gap < 1 || max_gap > BLOCKS_MAX_GAP ||
        max_shift > BLOCKS_MAX_GAP || (emit ? !out : !counts))
        return hipErrorInvalidValue;
    if (emit)
        hipLaunchKernelGGL(k_run_blocks<true>, dim3(nchunks), dim3(256), 0, st, run_start, run_end, run_mate, contigs, chunks, boff, nb,
                           min_run, max_gap, max_shift, counts, offs, total, out);
    else
        hipLaunchKernelGGL(k_run_blocks<false>, dim3(nchunks), dim3(256), 0, st, run_start, run_end, run_mate, contigs, chunks, boff, nb,
                           min_run, max_gap, max_shift, counts, offs, total, out);
    return hipGetLastError();
}

}  // namespace pg
