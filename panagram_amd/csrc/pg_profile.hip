// pg_profile.hip — the presence profile of windows of a finished bitmap's rows ON THE GPU (gfx950): per window and genome g,
// how much of the window genome g holds and in how many pieces — the answer to "which of these genomes carry this query
// sequence, and how completely" once the query's k-mers have been anchored (panagram_amd/search.py).  Row r of a window is the
// k-mer at the window's bases [r, r + k); per genome the kernel leaves what the six fields of include/panagram_hip.h
// (pg_result_presence_profile: hits, runs, longest, first, end, covered) are folded from.
// Every row is read ONCE and all N columns are followed at the same time.  No atomics, no histogram, no records: a block
// writes one partial per genome and one {all, none} pair, and nothing else.
//
// Windows and chunks as in pg_gaps.hip, at stride 1: a window is rows [s, e) of one contig, the host cuts it into chunks of
// PROFILE_CHUNK consecutive rows (chunk = {window, first row}), grid = chunks (of all windows), 256 threads; a block takes its
// chunk tile by tile (256 rows, one per lane) in order.
//   transpose  as k_absence_runs: a lane loads its row (pg_rowread.h; the bits at and past N never count, the columns outside
//              `select` are cleared here), the ballot of bit c over the wave IS the 64-row word of column c (pairs_ballot_word,
//              pg_pairblocks.h), the four waves leave their words in LDS: tile[wave][c], two buffers, one barrier per tile.
//   rows       before the transpose a lane knows whether its row holds every selected genome's bit, or none: two ballots per
//              wave and tile, their popcounts kept wave-uniform and summed over the four waves at the chunk's end.
//   walk       thread c owns column c for the whole chunk (N > 256: c + 256 too), its state in registers.  Per 64-row word:
//              hits = popcount; runs = popcount of the run starts, w & ~(w << 1 | the last bit of the word before); first and
//              end from ctz / clz of the first / last word with a bit; the present rows from the chunk's first row on from ctz
//              of the complement.  The longest run and the clipped gap sum need the runs themselves: they come off run by run
//              with ctz of the word and of its complement, a word without a bit in one step.
//   partial    {hits, runs, longest, first, end, gapsum, head, tail} per (chunk, genome), all chunk-relative: gapsum = the sum of
//              min(k - 1, L) over the runs of L absent rows between two set rows OF THE CHUNK; head / tail = the present rows
//              from the chunk's first row on / up to its last row.  The absent rows at the two edges are first and rows - end; a
//              chunk is all absent when hits == 0 and all present when hits == rows.  32 bytes: two 16-byte stores.
// The stitch of a window's chunks is HOST code (pg_profile_host.h), as the absence runs' is; a window of one chunk — a gene, a
// transcript — needs none.  A row number inside a chunk, and every count of a partial, fits 32 bits with room to spare
// (gapsum <= 31 * 2048).
// N <= 128 (k_presence_profile<4, 1>): a lane loads its row's words once, into registers, before the ballots; beyond, up to
// PROFILE_MAX_GENOMES, word by word (<0, 1> up to 256 columns, <0, 2> two columns per thread).
#include "pg_kernels.h"
#include "pg_rowread.h"
#include "pg_pairblocks.h"

namespace pg {

constexpr uint32_t PROFILE_TILE = 256;  // rows per tile: one 64-row word per wave
static_assert(PROFILE_CHUNK % PROFILE_TILE == 0, "a chunk is a whole number of tiles");

struct ProfileColumn {
    uint32_t hits, runs, longest, first, end, gapsum, head;
    uint32_t open_p;  // rows of the present run open at the end of the rows walked so far
    uint32_t open_a;  // absent rows since the last set row (all rows so far when none is set)
    uint32_t carry;   // the last row's bit
    bool seen;        // a set row has been walked
    bool at_head;     // every row so far is set
};

// one 64-row word `w` of a column (nv rows exist, the bits at and past nv are 0; bit 0 is row row0 of the chunk; a word before
// the chunk's last one has nv == 64)
__device__ __forceinline__ void profile_walk_word(uint64_t w, uint32_t nv, uint32_t row0, uint32_t k1, ProfileColumn &s) {
    if (w == 0) {
        s.open_a += nv;
        s.open_p = 0;
        s.carry = 0;
        s.at_head = false;
        return;
    }
    s.hits += (uint32_t)__popcll(w);
    s.runs += (uint32_t)__popcll(w & ~((w << 1) | (uint64_t)s.carry));
    s.carry = (uint32_t)(w >> 63);
    if (!s.seen) s.first = row0 + (uint32_t)__builtin_ctzll(w);
    s.end = row0 + 64u - (uint32_t)__builtin_clzll(w);
    if (s.at_head) {
        const uint64_t inv = ~w;
        const uint32_t t = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;  // (t <= nv: the bits past nv are 0)
        s.head += t;
        s.at_head = t == nv;
    }
    uint32_t p = 0;
    while (p < nv) {
        const uint64_t x = w >> p;
        if (x & 1ull) {
            const uint64_t inv = ~x;
            const uint32_t ones = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;  // (p + ones <= nv, as above)
            if (!s.open_p && s.seen) s.gapsum += min(k1, s.open_a);  // a gap between two set rows ends here
            s.seen = true;
            s.open_p += ones;
            s.open_a = 0;
            s.longest = max(s.longest, s.open_p);
            p += ones;
        } else {
            const uint32_t zeros = x ? (uint32_t)__builtin_ctzll(x) : nv - p;
            s.open_a += zeros;
            s.open_p = 0;
            p += zeros;
        }
    }
}

template <uint32_t MAXW, uint32_t NQ>
__global__ __launch_bounds__(256) void k_presence_profile(uint32_t N, const uint8_t *__restrict__ rows,
                                                          const uint64_t *__restrict__ base, const uint64_t *__restrict__ ends,
                                                          const uint2 *__restrict__ chunks, const uint32_t *__restrict__ select,
                                                          uint32_t k1, uint4 *__restrict__ partial, uint2 *__restrict__ allnone) {
    // [2 buffers][4 waves][NC] column words, then [4 waves] {rows with every selected bit, rows with none}
    extern __shared__ __align__(16) uint64_t psm[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    const uint32_t NC = (N + 63) & ~63u;
    uint2 *lrows = reinterpret_cast<uint2 *>(psm + (size_t)2 * 4 * NC);
    const uint2 ck = chunks[blockIdx.x];
    const uint32_t win = ck.x;
    const uint8_t *crow = rows + base[win];
    const uint64_t c0 = ck.y, ce = min(c0 + (uint64_t)PROFILE_CHUNK, ends[win]);  // this chunk: rows [c0, ce), c0 < ce
    ProfileColumn s[NQ];
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) s[q] = ProfileColumn{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, false, true};
    uint32_t sw[MAXW ? MAXW : 1];
#pragma unroll
    for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) sw[d] = MAXW && d < ndw ? select[d] & valid_bits(N, d) : 0u;
    uint32_t nall = 0, nnone = 0;  // (wave-uniform)
    uint32_t buf = 0;
    for (uint64_t t0 = c0; t0 < ce; t0 += PROFILE_TILE, buf ^= 1) {
        const uint64_t j = t0 + tid;
        const bool act = j < ce;
        const uint8_t *p = crow + j * nbytes;
        uint64_t *tile = psm + (size_t)buf * 4 * NC;
        uint64_t *mycols = tile + wave * NC;
        bool every = act, any = false;
        if (MAXW) {
            uint32_t w[MAXW ? MAXW : 1];
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
                w[d] = act && d < ndw ? row_word(p, d, nbytes) & sw[d] : 0u;
                every = every && w[d] == sw[d];
                any = any || w[d];
            }
            uint64_t word = 0;
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
                if (d < ndw) word = pairs_ballot_word(w[d], d, N, lane, word);
                if ((d & 1) && 32 * (d - 1) < NC) {
                    mycols[32 * (d - 1) + lane] = word;
                    word = 0;
                }
            }
        } else {
            for (uint32_t q = 0; 64 * q < NC; ++q) {
                uint64_t word = 0;
                for (uint32_t d = 2 * q; d < min(2 * q + 2, ndw); ++d) {
                    const uint32_t m = select[d] & valid_bits(N, d);
                    const uint32_t w = act ? row_word(p, d, nbytes) & m : 0u;
                    every = every && w == m;
                    any = any || w;
                    word = pairs_ballot_word(w, d, N, lane, word);
                }
                mycols[64 * q + lane] = word;
            }
        }
        nall += (uint32_t)__popcll(__ballot(every));
        nnone += (uint32_t)__popcll(__ballot(act && !any));
        __syncthreads();
        // (no second barrier: the next tile goes to the other buffer, and this one is written again only behind the next
        // tile's barrier, which every wave passes after these reads)
        const uint32_t valid = (uint32_t)min((uint64_t)PROFILE_TILE, ce - t0);
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q) {
            const uint32_t c = tid + 256 * q;
            if (c >= N) continue;
            for (uint32_t w = 0; w < 4 && 64 * w < valid; ++w) {
                const uint32_t nv = min(64u, valid - 64 * w);
                profile_walk_word(tile[w * NC + c], nv, (uint32_t)(t0 - c0) + 64 * w, k1, s[q]);
            }
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) {
        const uint32_t c = tid + 256 * q;
        if (c >= N) continue;
        // (a column outside `select` was cleared at the transpose: its partial is zeros)
        uint4 *out = partial + ((uint64_t)blockIdx.x * N + c) * 2;
        out[0] = make_uint4(s[q].hits, s[q].runs, s[q].longest, s[q].first);
        out[1] = make_uint4(s[q].end, s[q].gapsum, s[q].head, s[q].open_p);
    }
    if (lane == 0) lrows[wave] = make_uint2(nall, nnone);
    __syncthreads();
    if (tid == 0) {
        uint2 sum = lrows[0];
        for (uint32_t v = 1; v < 4; ++v) sum.x += lrows[v].x, sum.y += lrows[v].y;
        allnone[blockIdx.x] = sum;
    }
}

hipError_t launch_presence_profile(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, const uint64_t *base,
                                   const uint64_t *ends, const uint2 *chunks, uint32_t nchunks, const uint32_t *select, uint32_t k,
                                   uint4 *partial, uint2 *allnone) {
    if (nchunks == 0) return hipSuccess;
    if (ngenomes < 1 || ngenomes > PROFILE_MAX_GENOMES || k < 1) return hipErrorInvalidValue;
    if (!rows || !base || !ends || !chunks || !select || !partial || !allnone) return hipErrorInvalidValue;
    const uint32_t NC = (ngenomes + 63) & ~63u;
    const size_t lds = (size_t)2 * 4 * NC * 8 + 4 * sizeof(uint2);
#define PG_PROFILE_LAUNCH(MAXW, NQ)                                                                                          \
    hipLaunchKernelGGL((k_presence_profile<MAXW, NQ>), dim3(nchunks), dim3(256), lds, st, ngenomes, rows, base, ends, chunks, \
                       select, k - 1, partial, allnone)
    if (ngenomes <= 128)
        PG_PROFILE_LAUNCH(4, 1);
    else if (ngenomes <= 256)
        PG_PROFILE_LAUNCH(0, 1);
    else
        PG_PROFILE_LAUNCH(0, 2);
#undef PG_PROFILE_LAUNCH
    return hipGetLastError();
}

}  // namespace pg
