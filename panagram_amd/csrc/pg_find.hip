// pg_find.hip — presence/absence pattern runs of a finished bitmap's rows ON THE GPU (gfx950): where are the k-mers that THESE
// genomes hold and THOSE genomes lack?  (scripts/query_index.py's "custom" branch: np.flatnonzero((kmers[:,0]==1) &
// (kmers[:,1]==0) & ...) over a chromosome unpacked to one byte per bit on the host.)
//
// The rule: two masks of ceil(N / 32) words, `have` (H) and `lack` (L), and two thresholds.  A row MATCHES iff
//   popcount(row & H) >= min_have  and  popcount(row & L) <= max_lack.
// The caller clears the masks' bits at and past N, so the bits past N in a row's last byte never count on either side.
// A window is a range [s, e) of SAMPLED rows of one contig, as in pg_bins.hip: sampled row j is row j * stride of the contig's
// rows.  A RUN is a maximal range [a, b) of consecutive sampled rows of a window that all match; the window's edges cut
// runs — no row outside [s, e) is read, not even to decide where a run begins or ends.
//
// The host cuts every window into chunks of FIND_CHUNK consecutive sampled rows; chunk = {window, first sampled row}.
// grid = chunks (of all windows), 256 threads: a block takes its chunk tile by tile (256 sampled rows, one per lane) in order.
//   evaluate   a lane loads its row and applies the rule; the wave's ballot of the match bit is a 64-row word.  The four
//              waves leave their words in LDS (two buffers: one barrier per tile) and every thread reads all four back, so
//              what follows is the same in every lane of the block (scalar work).
//   edges      carry = the match bit of the sampled row before the word's first: the top bit of the previous wave's word,
//              of the previous tile's last word, at the chunk's first row ONE more row evaluation (row c0 - 1, the chunk's
//              halo), and 0 at the window's first row, where no load is made.  With prev = m << 1 | carry:
//                run starts  m & ~prev
//                run ends    ~m & prev & (rows of the chunk): a non-matching row whose predecessor matches ends a run at
//                            its own number (exclusive), and the window's last chunk adds one end at e when row e - 1 matches.
//              Both need the predecessor only, hence one halo row per chunk and none behind it.
// Two passes over the rows, and no workgroup ever waits for another (no look-back, no polling):
//   count  (EMIT = false)  counts[chunk] = {matching rows, run starts, run ends, 0}: one 16-byte vector store per block, no
//                          atomics.  The host sums them per window and takes the exclusive scans of the starts and the ends.
//   emit   (EMIT = true)   the same evaluation; a lane that holds a start writes its sampled row number to run_start[the
//                          chunk's start offset + starts of the chunk so far + starts below the lane], and the ends go to
//                          run_end the same way from the chunk's end offset.  Starts and ends are counted separately: the
//                          i-th start and the i-th end of a window are the same run, so a run may begin in one chunk and end
//                          in another without the chunks exchanging anything, and the output is sorted by (window, start)
//                          by construction — the same on every run.
// A sampled row number fits 32 bits: a contig's rows are counted in 32 bits (AnchorDesc::nkmers), and so does an exclusive end.
// N <= 128 (k_find_runs<4, .>): the masks in registers, a row's words loaded once; beyond, up to FIND_MAX_GENOMES
// (k_find_runs<0, .>), word by word against masks staged in LDS.
#include "pg_kernels.h"
#include "pg_rowread.h"

namespace pg {

constexpr uint32_t FIND_TILE = 256;  // sampled rows per tile: one 64-row word per wave
static_assert(FIND_CHUNK % FIND_TILE == 0, "a chunk is a whole number of tiles");

// does the row at p match?  MAXW: hw / lw are the masks' words in registers; 0: msk = [have words][lack words] in LDS
template <uint32_t MAXW>
__device__ __forceinline__ bool find_match(const uint8_t *__restrict__ p, uint32_t nbytes, uint32_t ndw, const uint32_t *hw,
                                           const uint32_t *lw, const uint32_t *msk, uint32_t min_have, uint32_t max_lack) {
    uint32_t ch = 0, cl = 0;
    if (MAXW) {
#pragma unroll
        for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
            if (d < ndw) {
                const uint32_t w = row_word(p, d, nbytes);
                ch += (uint32_t)__popc(w & hw[d]);
                cl += (uint32_t)__popc(w & lw[d]);
            }
        }
    } else {
        for (uint32_t d = 0; d < ndw; ++d) {
            const uint32_t w = row_word(p, d, nbytes);
            ch += (uint32_t)__popc(w & msk[d]);
            cl += (uint32_t)__popc(w & msk[ndw + d]);
        }
    }
    return ch >= min_have && cl <= max_lack;
}

template <uint32_t MAXW, bool EMIT>
__global__ __launch_bounds__(256) void k_find_runs(uint32_t N, const uint8_t *__restrict__ rows, uint32_t stride,
                                                   const uint64_t *__restrict__ base, const uint64_t *__restrict__ starts,
                                                   const uint64_t *__restrict__ ends, const uint2 *__restrict__ chunks,
                                                   const uint32_t *__restrict__ have, const uint32_t *__restrict__ lack,
                                                   uint32_t min_have, uint32_t max_lack, uint4 *__restrict__ counts,
                                                   const ulonglong2 *__restrict__ offs, uint64_t total,
                                                   uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_end) {
    extern __shared__ __align__(16) uint32_t fsm[];  // [2 buffers][4 waves] 64-row words, then (MAXW = 0) the masks' 2 ndw words
    uint64_t *words = reinterpret_cast<uint64_t *>(fsm);
    uint32_t *msk = fsm + 16;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    uint32_t hw[MAXW ? MAXW : 1], lw[MAXW ? MAXW : 1];
#pragma unroll
    for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
        hw[d] = MAXW && d < ndw ? have[d] : 0u;
        lw[d] = MAXW && d < ndw ? lack[d] : 0u;
    }
    if (!MAXW) {
        for (uint32_t i = tid; i < 2 * ndw; i += 256) msk[i] = i < ndw ? have[i] : lack[i - ndw];
        __syncthreads();
    }
    const uint2 ck = chunks[blockIdx.x];
    const uint8_t *crow = rows + base[ck.x];
    const uint64_t s = starts[ck.x], e = ends[ck.x];
    const uint64_t c0 = ck.y, ce = min(c0 + (uint64_t)FIND_CHUNK, e);  // this chunk: sampled rows [c0, ce), s <= c0 < ce <= e
    // the chunk's halo: the match bit of sampled row c0 - 1 (every lane the same row: one broadcast load)
    uint64_t carry = 0;
    if (c0 > s)
        carry = __ballot(find_match<MAXW>(crow + (c0 - 1) * stride * nbytes, nbytes, ndw, hw, lw, msk, min_have, max_lack)) ? 1 : 0;
    uint32_t matched = 0, nstarts = 0, nends = 0;
    uint64_t soff = 0, eoff = 0;
    if (EMIT) {
        const ulonglong2 o = offs[blockIdx.x];
        soff = o.x;
        eoff = o.y;
    }
    uint32_t buf = 0;
    for (uint64_t t0 = c0; t0 < ce; t0 += FIND_TILE, buf ^= 1) {
        const uint64_t j = t0 + tid;
        const bool m = j < ce && find_match<MAXW>(crow + j * stride * nbytes, nbytes, ndw, hw, lw, msk, min_have, max_lack);
        const uint64_t mine = __ballot(m);
        if (lane == 0) words[4 * buf + wave] = mine;
        __syncthreads();
        // (no second barrier: the next tile's words go to the other buffer, and this one is written again only behind the
        // next tile's barrier, which every wave passes after these reads)
        const uint32_t valid = (uint32_t)min((uint64_t)FIND_TILE, ce - t0);
        uint32_t sbelow = 0, ebelow = 0;  // starts / ends of this tile in the waves below this one
        uint64_t smine = 0, emine = 0;
        uint32_t stile = 0, etile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint64_t b = words[4 * buf + w];
            const uint64_t act = valid >= 64 * (w + 1) ? ~0ull : valid <= 64 * w ? 0ull : (1ull << (valid - 64 * w)) - 1ull;
            const uint64_t prev = (b << 1) | carry;
            const uint64_t sm = b & ~prev, em = ~b & prev & act;
            if (w == wave) {
                smine = sm;
                emine = em;
                sbelow = stile;
                ebelow = etile;
            }
            stile += (uint32_t)__popcll(sm);
            etile += (uint32_t)__popcll(em);
            matched += (uint32_t)__popcll(b);
            carry = b >> 63;
        }
        if (EMIT) {
            const uint64_t below = (1ull << lane) - 1ull;
            if ((smine >> lane) & 1ull) {
                const uint64_t at = soff + nstarts + sbelow + (uint32_t)__popcll(smine & below);
                if (at < total) run_start[at] = (uint32_t)j;
            }
            if ((emine >> lane) & 1ull) {
                const uint64_t at = eoff + nends + ebelow + (uint32_t)__popcll(emine & below);
                if (at < total) run_end[at] = (uint32_t)j;
            }
        }
        nstarts += stile;
        nends += etile;
    }
    // the window's last chunk: does row e - 1 match?  Not `carry`: a partly filled last tile leaves it 0, the rows past ce being
    // no matches.  The bit is in the last tile's words, which the loop's final `buf ^= 1` has left in the other buffer.
    if (ce == e) {
        const uint32_t last = (uint32_t)((ce - 1 - c0) % FIND_TILE);
        const uint64_t b = words[4 * (buf ^ 1) + last / 64];
        if ((b >> (last % 64)) & 1ull) {  // the window ends inside a run
            if (EMIT && tid == 0) {
                const uint64_t at = eoff + nends;
                if (at < total) run_end[at] = (uint32_t)e;
            }
            nends += 1;
        }
    }
    if (!EMIT && tid == 0) counts[blockIdx.x] = make_uint4(matched, nstarts, nends, 0u);
}

hipError_t launch_find_runs(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, const uint64_t *base,
                            const uint64_t *starts, const uint64_t *ends, const uint2 *chunks, uint32_t nchunks,
                            const uint32_t *have, const uint32_t *lack, uint32_t min_have, uint32_t max_lack, uint4 *counts,
                            const ulonglong2 *offs, uint64_t total, uint32_t *run_start, uint32_t *run_end) {
    if (nchunks == 0) return hipSuccess;
    if (ngenomes < 1 || ngenomes > FIND_MAX_GENOMES) return hipErrorInvalidValue;
    const bool emit = offs != nullptr;
    if (emit ? (!run_start || !run_end) : !counts) return hipErrorInvalidValue;
    const uint32_t ndw = (ngenomes + 31) / 32;
    const size_t lds = 64 + (ngenomes <= 128 ? 0 : (size_t)2 * ndw * 4);
#define PG_FIND_LAUNCH(MAXW, EMIT)                                                                                              \
    hipLaunchKernelGGL((k_find_runs<MAXW, EMIT>), dim3(nchunks), dim3(256), lds, st, ngenomes, rows, stride, base, starts, ends, \
                       chunks, have, lack, min_have, max_lack, counts, offs, total, run_start, run_end)
    if (ngenomes <= 128) {
        if (emit)
            PG_FIND_LAUNCH(4, true);
        else
            PG_FIND_LAUNCH(4, false);
    } else {
        if (emit)
            PG_FIND_LAUNCH(0, true);
        else
            PG_FIND_LAUNCH(0, false);
    }
#undef PG_FIND_LAUNCH
    return hipGetLastError();
}

}  // namespace pg
