// pg_gaps.hip — absence runs of a finished bitmap's rows ON THE GPU (gfx950): per genome g, the maximal runs of consecutive
// sampled rows WITHOUT g's bit — where, and how, genome g differs from the anchor.  (Index.query_bitmap followed by a per-column
// np.diff of the padded absence vector; row r of bitmap.1 is the k-mer at anchor bases [r, r + k), so one substituted base
// in g clears k consecutive rows of g's column, an insertion k - 1, a deletion of d bases k - 1 + d: panagram_amd/gaps.py.)
// Every row is read ONCE and all N columns are followed at the same time.
//
// A window is a range [s, e) of SAMPLED rows of one contig, as in pg_find.hip: sampled row j is row j * stride of the contig's
// rows, and no row outside a window is read.  The host cuts every window into chunks of GAPS_CHUNK consecutive sampled rows;
// chunk = {window, first sampled row}.  grid = chunks (of all windows), 256 threads: a block takes its chunk tile by tile (256
// sampled rows, one per lane) in order.
//   transpose  a lane loads its row (pg_rowread.h; the bits at and past N never count, and the columns outside `select` are
//              cleared here, so a word of unselected columns costs one ballot); the ballot of bit c over the wave IS the 64-row
//              word of column c (pairs_ballot_word, pg_pairblocks.h).  The four waves leave their words in LDS: tile[wave][c],
//              two buffers, so one barrier per tile.  The absence word of column c = ~word & (the rows of the tile that exist).
//   walk       thread c owns column c for the whole chunk (N > 256: c + 256 too), its state in registers: the length of the
//              run open at the previous word's end, whether a present row has been seen, the absent rows.  Per tile it walks
//              the four words in order; the runs inside a word come off with ctz of the word and of its complement.
//   closed     a run with a present row on both sides INSIDE the chunk adds 1 to its spectrum bin min(rows, maxlen) — an
//              integer atomic, so the result does not depend on order — and, when selected for emission (min_len <= rows, and
//              rows <= max_len unless max_len is 0), 1 to its window's count and one record {window, genome, first sampled row,
//              rows}.  The records of a chunk are collected in LDS (GAPS_LDS_RECS of them, an LDS atomic each) and go out at the
//              chunk's end behind ONE add to the global cursor; a chunk with more takes the cursor once per further record.
//              (One add per record: 783 k records of 8 genomes over 100 M rows kept the one cursor word busy for 8.7 ms, the
//              rate at which one word takes atomics, around a kernel of 0.6 ms.)  Records at or past cap are dropped, the
//              cursor counts on.  The caller sorts the records: their keys are unique.
//   The rule for the spectrum's atomics: N * (maxlen + 1) <= GAPS_LDS_BINS (6144 bins, 24 KiB) — the chunk's whole table
//              [N][maxlen + 1] is kept in LDS, zeroed at the chunk's start, and its non-zero bins are added to HBM at the
//              chunk's end (8 genomes at maxlen 84: 680 bins; 64 genomes: 5440).  Beyond — 512 genomes, or maxlen 4096 — the
//              table would crowd out the tiles (at 512 genomes they take 32 KiB, the records 4: 60 KiB in all), and closed
//              runs add to HBM directly.
//   edges      no block waits for another or looks back: a chunk writes {head, tail} per genome — the absent rows from its
//              first row on and up to its last row, both the chunk's rows when no row of it is present.
// The stitch step is HOST code over the downloaded edges (pg_gaps_host.h): per (window, genome) it walks the window's chunks in
// order and joins tail, whole-absent chunks and head into runs.  The edges are 8 bytes per chunk and genome — 1.5 MB for 8
// genomes over 100 M rows — against the rows' 100 MB read by the kernel; a second kernel would save that download and cost a
// launch, a scan over a chain of unknown length per column, and a second emitter.  On the host the step is thirty lines that a
// stand-alone program checks under the host sanitizers (tools/gaps_stitch_check.cpp).
// A sampled row number fits 32 bits: a contig's rows are counted in 32 bits (AnchorDesc::nkmers).  So do the spectrum's
// counters: a window holds fewer closed runs than rows.
// N <= 128 (k_absence_runs<4, 1, .>): a lane loads its row's words once, into registers, before the ballots; beyond, up to
// GAPS_MAX_GENOMES, word by word (k_absence_runs<0, 1, .> up to 256 columns, <0, 2, .> two columns per thread).
#include "pg_kernels.h"
#include "pg_rowread.h"
#include "pg_pairblocks.h"

namespace pg {

constexpr uint32_t GAPS_TILE = 256;  // sampled rows per tile: one 64-row word per wave
constexpr uint32_t GAPS_LDS_RECS = 255;  // records a chunk collects in LDS: with their 16-byte header 4 KiB
static_assert(GAPS_CHUNK % GAPS_TILE == 0, "a chunk is a whole number of tiles");

struct GapColumn {
    uint32_t open;    // rows of the run open at the end of the rows walked so far
    uint32_t head;    // absent rows before the chunk's first present row (once seen)
    uint32_t absent;  // absent rows so far
    bool seen;        // a present row has been walked
};

// one 64-row absence word `a` of a column (nv rows exist, the bits at and past nv are 0; bit 0 is sampled row row0):
// closed(rows, exclusive end) for every run that a present row of this chunk bounds on both sides
template <class F>
__device__ __forceinline__ void gaps_walk_word(uint64_t a, uint32_t nv, uint32_t row0, GapColumn &s, F &&closed) {
    s.absent += (uint32_t)__popcll(a);
    uint32_t p = 0;
    while (p < nv) {
        const uint64_t inv = ~(a >> p);
        const uint32_t z = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;  // absent rows from p on (z <= nv - p: the bits past nv are 0)
        s.open += z;
        p += z;
        if (p >= nv) break;  // the run stays open at the word's end
        // row p is present
        if (!s.seen) {
            s.head = s.open;
            s.seen = true;
        } else if (s.open) {
            closed(s.open, row0 + p);
        }
        s.open = 0;
        const uint64_t rest = a >> p;  // (bit 0 clear) on to the next absent row, if the word has one
        p = rest ? p + (uint32_t)__builtin_ctzll(rest) : nv;
    }
}

template <uint32_t MAXW, uint32_t NQ, bool LDSH>
__global__ __launch_bounds__(256) void k_absence_runs(uint32_t N, const uint8_t *__restrict__ rows, uint32_t stride,
                                                      const uint64_t *__restrict__ base, const uint64_t *__restrict__ ends,
                                                      const uint2 *__restrict__ chunks, const uint32_t *__restrict__ select,
                                                      uint32_t maxlen, uint32_t min_len, uint32_t max_len,
                                                      uint32_t *__restrict__ hist, unsigned long long *__restrict__ absent,
                                                      uint2 *__restrict__ edges, unsigned long long *__restrict__ nsel,
                                                      unsigned long long *__restrict__ cursor, uint64_t cap,
                                                      uint4 *__restrict__ recs) {
    // [2 buffers][4 waves][NC] column words, {records collected, -, the cursor's base (64 bits)}, [GAPS_LDS_RECS] records, then
    // (LDSH) [N][maxlen + 1] bins
    extern __shared__ __align__(16) uint64_t gsm[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    const uint32_t NC = (N + 63) & ~63u, nb = maxlen + 1;
    uint32_t *lcount = reinterpret_cast<uint32_t *>(gsm + (size_t)2 * 4 * NC);
    uint64_t *lbase = gsm + (size_t)2 * 4 * NC + 1;
    uint4 *lrecs = reinterpret_cast<uint4 *>(gsm + (size_t)2 * 4 * NC + 2);
    uint32_t *lh = reinterpret_cast<uint32_t *>(lrecs + GAPS_LDS_RECS);
    // (both first added to behind the first tile's barrier)
    if (tid == 0) *lcount = 0;
    if (LDSH)
        for (uint32_t i = tid; i < N * nb; i += 256) lh[i] = 0;
    const uint2 ck = chunks[blockIdx.x];
    const uint32_t win = ck.x;
    const uint8_t *crow = rows + base[win];
    const uint64_t c0 = ck.y, ce = min(c0 + (uint64_t)GAPS_CHUNK, ends[win]);  // this chunk: sampled rows [c0, ce), c0 < ce
    GapColumn s[NQ];
    bool mine[NQ];
    uint32_t nselected = 0;
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) {
        const uint32_t c = tid + 256 * q;
        mine[q] = c < N && ((select[c >> 5] >> (c & 31)) & 1u);
        s[q] = GapColumn{0u, 0u, 0u, false};
    }
    uint32_t sw[MAXW ? MAXW : 1];
#pragma unroll
    for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) sw[d] = MAXW && d < ndw ? select[d] & valid_bits(N, d) : 0u;
    uint32_t buf = 0;
    for (uint64_t t0 = c0; t0 < ce; t0 += GAPS_TILE, buf ^= 1) {
        const uint64_t j = t0 + tid;
        const bool act = j < ce;
        const uint8_t *p = crow + j * stride * nbytes;
        uint64_t *tile = gsm + (size_t)buf * 4 * NC;
        uint64_t *mycols = tile + wave * NC;
        if (MAXW) {
            uint32_t w[MAXW ? MAXW : 1];
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) w[d] = act && d < ndw ? row_word(p, d, nbytes) & sw[d] : 0u;
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
                for (uint32_t d = 2 * q; d < min(2 * q + 2, ndw); ++d)
                    word = pairs_ballot_word(act ? row_word(p, d, nbytes) & select[d] & valid_bits(N, d) : 0u, d, N, lane, word);
                mycols[64 * q + lane] = word;
            }
        }
        __syncthreads();
        // (no second barrier: the next tile goes to the other buffer, and this one is written again only behind the next
        // tile's barrier, which every wave passes after these reads)
        const uint32_t valid = (uint32_t)min((uint64_t)GAPS_TILE, ce - t0);
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q) {
            if (!mine[q]) continue;
            const uint32_t c = tid + 256 * q;
            auto closed = [&](uint32_t len, uint32_t end) {
                const uint32_t bin = min(len, maxlen);
                if (LDSH)
                    atomicAdd(&lh[c * nb + bin], 1u);
                else
                    atomicAdd(&hist[((uint64_t)win * N + c) * nb + bin], 1u);
                if (len >= min_len && (max_len == 0 || len <= max_len)) {
                    ++nselected;
                    if (cap) {
                        const uint4 rec = make_uint4(win, c, end - len, len);
                        const uint32_t slot = atomicAdd(lcount, 1u);
                        if (slot < GAPS_LDS_RECS) {
                            lrecs[slot] = rec;
                        } else {
                            const unsigned long long at = atomicAdd(cursor, 1ull);
                            if (at < cap) recs[at] = rec;
                        }
                    }
                }
            };
            for (uint32_t w = 0; w < 4 && 64 * w < valid; ++w) {
                const uint32_t nv = min(64u, valid - 64 * w);
                const uint64_t exist = nv == 64 ? ~0ull : (1ull << nv) - 1ull;
                gaps_walk_word(~tile[w * NC + c] & exist, nv, (uint32_t)t0 + 64 * w, s[q], closed);
            }
        }
    }
    const uint32_t nrows = (uint32_t)(ce - c0);
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) {
        if (!mine[q]) continue;
        const uint32_t c = tid + 256 * q;
        // (no present row: open has counted every row of the chunk)
        edges[(uint64_t)blockIdx.x * N + c] = s[q].seen ? make_uint2(s[q].head, s[q].open) : make_uint2(nrows, nrows);
        if (s[q].absent) atomicAdd(&absent[(uint64_t)win * N + c], (unsigned long long)s[q].absent);
    }
    if (nselected) atomicAdd(&nsel[win], (unsigned long long)nselected);
    if (LDSH || cap) __syncthreads();  // (cap is the same in every thread)
    if (LDSH) {
        for (uint32_t i = tid; i < N * nb; i += 256) {
            const uint32_t v = lh[i];
            if (v) atomicAdd(&hist[(uint64_t)win * N * nb + i], v);
        }
    }
    if (cap) {
        const uint32_t kept = min(*lcount, GAPS_LDS_RECS);
        if (tid == 0 && kept) *lbase = atomicAdd(cursor, (unsigned long long)kept);
        __syncthreads();
        if (kept) {
            const uint64_t at = *lbase;
            for (uint32_t i = tid; i < kept; i += 256)
                if (at + i < cap) recs[at + i] = lrecs[i];
        }
    }
}

hipError_t launch_absence_runs(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, const uint64_t *base,
                               const uint64_t *ends, const uint2 *chunks, uint32_t nchunks, const uint32_t *select,
                               uint32_t maxlen, uint32_t min_len, uint32_t max_len, uint32_t *hist, unsigned long long *absent,
                               uint2 *edges, unsigned long long *nsel, unsigned long long *cursor, uint64_t cap, uint4 *recs) {
    if (nchunks == 0) return hipSuccess;
    if (ngenomes < 1 || ngenomes > GAPS_MAX_GENOMES || maxlen < 1 || maxlen > GAPS_MAX_MAXLEN || min_len < 1)
        return hipErrorInvalidValue;
    if (!hist || !absent || !edges || !nsel || !cursor || (cap && !recs)) return hipErrorInvalidValue;
    const uint32_t NC = (ngenomes + 63) & ~63u;
    const bool ldsh = (uint64_t)ngenomes * (maxlen + 1) <= GAPS_LDS_BINS;
    const size_t lds = (size_t)2 * 4 * NC * 8 + 16 + (size_t)GAPS_LDS_RECS * 16 + (ldsh ? (size_t)ngenomes * (maxlen + 1) * 4 : 0);
#define PG_GAPS_LAUNCH(MAXW, NQ, LDSH)                                                                                          \
    hipLaunchKernelGGL((k_absence_runs<MAXW, NQ, LDSH>), dim3(nchunks), dim3(256), lds, st, ngenomes, rows, stride, base, ends, \
                       chunks, select, maxlen, min_len, max_len, hist, absent, edges, nsel, cursor, cap, recs)
    if (ngenomes <= 128) {
        if (ldsh)
            PG_GAPS_LAUNCH(4, 1, true);
        else
            PG_GAPS_LAUNCH(4, 1, false);
    } else if (ngenomes <= 256) {
        if (ldsh)
            PG_GAPS_LAUNCH(0, 1, true);
        else
            PG_GAPS_LAUNCH(0, 1, false);
    } else {
        if (ldsh)
            PG_GAPS_LAUNCH(0, 2, true);
        else
            PG_GAPS_LAUNCH(0, 2, false);
    }
#undef PG_GAPS_LAUNCH
    return hipGetLastError();
}

}  // namespace pg
