// pg_place.hip — WHICH of the indexed genomes does an unassembled sample resemble along an anchor (gfx950)?  The sample's reads have
// been counted into one plane of a count table of the anchor's k-mers (pg_copies.hip); the anchor's finished bitmap rows say which
// genomes hold each of those k-mers.  This unit joins the two per row and reduces per window and genome, and nothing per position
// leaves the GPU.
//
// Definitions (tests/place_ref.py is the same in numpy).  For a window w = rows [s, e) of contig c of a rows result, and the
// anchor's sequence set A:
//   row correspondence  row r is the k-mer at bases [r, r + k) of contig c of A (the host refuses a contig whose row count is not
//                       len - k + 1, and a k that is not the count table's).
//   validity            row r is valid when that window of A holds no non-ACGT base.
//   sample column       s(r) = 1 when plane[slot(key(r))] >= min_count; a key the table does not hold reads 0, as in
//                       k_copy_profile.
//   valid[w]    the valid rows                      held[w]     the valid rows with s(r) = 1
//   col[w][g]   the valid rows with bit g set       both[w][g]  the valid rows with bit g set and s(r) = 1
//   The bits at and past N never count.
//
// Windows and chunks as in pg_profile.hip: the host cuts a window into chunks of PLACE_CHUNK consecutive rows (chunk = {window,
// first row}), grid = chunks (of all windows), 256 threads; a block takes its chunk tile by tile (256 rows, one per lane).
//   lookup     a lane resolves its position's validity (window_valid), key and slot (copy_key, copy_lookup: pg_keytable_dev.h) and
//              reads the plane's counter: the ballot of valid & s over the wave IS the 64-row sample word.
//   transpose  as k_presence_profile: the lane loads its row (pg_rowread.h; an invalid row reads as zeros), the ballot of bit c is
//              the 64-row word of column c (pairs_ballot_word), the four waves leave their words — and their sample words — in
//              LDS, two buffers, one barrier per tile.
//   count      thread c owns column c for the whole chunk (N > 256: c + 256 too) and adds popcount(word) and popcount(word &
//              sample word) of the four waves' words.
//   partial    {col, both} per (chunk, genome), {valid, held} per chunk, all 32-bit (at most PLACE_CHUNK each): 8-byte stores.
// No atomic, no block waits for another, every write to HBM is a vector store; the host sums a window's chunks in 64 bits.
// N <= 128 (k_sample_agree<4, 1>): a lane loads its row's words once, into registers, before the ballots; beyond, up to
// PROFILE_MAX_GENOMES, word by word (<0, 1> up to 256 columns, <0, 2> two columns per thread).
#include "pg_kernels.h"
#include "pg_keytable_dev.h"
#include "pg_rowread.h"
#include "pg_pairblocks.h"

namespace pg {

constexpr uint32_t PLACE_TILE = 256;  // rows per tile: one 64-row word per wave
static_assert(PLACE_CHUNK % PLACE_TILE == 0, "a chunk is a whole number of tiles");

template <uint32_t MAXW, uint32_t NQ>
__global__ __launch_bounds__(256) void k_sample_agree(uint32_t N, int k, const uint8_t *__restrict__ rows, const uint64_t *__restrict__ base,
                                                      const uint64_t *__restrict__ ends, const uint2 *__restrict__ chunks,
                                                      const uint32_t *__restrict__ wcontig, const SeqDesc *__restrict__ sd,
                                                      const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                      const unsigned long long *__restrict__ keys, uint64_t nslots, uint32_t max_probe,
                                                      const uint32_t *__restrict__ plane, uint32_t min_count,
                                                      uint2 *__restrict__ partial, uint2 *__restrict__ vh) {
    // [2 buffers][4 waves][NC] column words, then [2 buffers][4 waves] sample words, then [4 waves] {valid, held}
    extern __shared__ __align__(16) uint64_t lds_[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    const uint32_t NC = (N + 63) & ~63u;
    uint64_t *samp = lds_ + (size_t)2 * 4 * NC;
    uint2 *lsum = reinterpret_cast<uint2 *>(samp + 8);
    const uint2 ck = chunks[blockIdx.x];
    const uint32_t win = ck.x;
    const uint8_t *crow = rows + base[win];
    const uint64_t c0 = ck.y, ce = min(c0 + (uint64_t)PLACE_CHUNK, ends[win]);  // this chunk: rows [c0, ce), c0 < ce
    const ContigView v = contig_view(sd, wcontig[win], seqw_all, nmw_all, has_n, k);
    const uint64_t smask = nslots - 1;
    uint32_t col[NQ], both[NQ];
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) col[q] = both[q] = 0;
    uint32_t nvalid = 0, nheld = 0;  // (wave-uniform)
    uint32_t buf = 0;
    for (uint64_t t0 = c0; t0 < ce; t0 += PLACE_TILE, buf ^= 1) {
        const uint64_t j = t0 + tid;
        const bool valid = j < ce && window_valid(v, j, k);
        bool s = false;
        if (valid) {
            const uint32_t slot = copy_lookup(keys, smask, max_probe, copy_key(v.seqw, j, k));
            s = slot != SLOT_ABSENT && plane[slot] >= min_count;
        }
        const uint64_t sword = __ballot(s);
        nvalid += (uint32_t)__popcll(__ballot(valid));
        nheld += (uint32_t)__popcll(sword);
        const uint8_t *p = crow + j * nbytes;
        uint64_t *tile = lds_ + (size_t)buf * 4 * NC;
        uint64_t *mycols = tile + wave * NC;
        if (MAXW) {
            uint32_t w[MAXW ? MAXW : 1];
#pragma unroll
            for (uint32_t dd = 0; dd < (MAXW ? MAXW : 1); ++dd) w[dd] = valid && dd < ndw ? row_word(p, dd, nbytes) & valid_bits(N, dd) : 0u;
            uint64_t word = 0;
#pragma unroll
            for (uint32_t dd = 0; dd < (MAXW ? MAXW : 1); ++dd) {
                if (dd < ndw) word = pairs_ballot_word(w[dd], dd, N, lane, word);
                if ((dd & 1) && 32 * (dd - 1) < NC) {
                    mycols[32 * (dd - 1) + lane] = word;
                    word = 0;
                }
            }
        } else {
            for (uint32_t q = 0; 64 * q < NC; ++q) {
                uint64_t word = 0;
                for (uint32_t dd = 2 * q; dd < min(2 * q + 2, ndw); ++dd) {
                    const uint32_t w = valid ? row_word(p, dd, nbytes) & valid_bits(N, dd) : 0u;
                    word = pairs_ballot_word(w, dd, N, lane, word);
                }
                mycols[64 * q + lane] = word;
            }
        }
        if (lane == 0) samp[buf * 4 + wave] = sword;
        __syncthreads();
        // (no second barrier: the next tile goes to the other buffer, and this one is written again only behind the next
        // tile's barrier, which every wave passes after these reads)
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q) {
            const uint32_t c = tid + 256 * q;
            if (c >= N) continue;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {  // (a wave past the chunk's end left zeros)
                const uint64_t word = tile[w * NC + c];
                col[q] += (uint32_t)__popcll(word);
                both[q] += (uint32_t)__popcll(word & samp[buf * 4 + w]);
            }
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) {
        const uint32_t c = tid + 256 * q;
        if (c < N) partial[(uint64_t)blockIdx.x * N + c] = make_uint2(col[q], both[q]);
    }
    if (lane == 0) lsum[wave] = make_uint2(nvalid, nheld);
    __syncthreads();
    if (tid == 0) {
        uint2 sum = lsum[0];
        for (uint32_t v = 1; v < 4; ++v) sum.x += lsum[v].x, sum.y += lsum[v].y;
        vh[blockIdx.x] = sum;
    }
}

hipError_t launch_sample_agree(hipStream_t st, uint32_t ngenomes, int k, const uint8_t *rows, const uint64_t *base, const uint64_t *ends,
                               const uint2 *chunks, uint32_t nchunks, const uint32_t *wcontig, const SeqDesc *sd, const uint64_t *seqw,
                               const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys, uint64_t nslots,
                               uint32_t max_probe, const uint32_t *plane, uint32_t min_count, uint2 *partial, uint2 *vh) {
    if (nchunks == 0) return hipSuccess;
    if (ngenomes < 1 || ngenomes > PROFILE_MAX_GENOMES || k < 1 || k > 32 || min_count < 1) return hipErrorInvalidValue;
    if (nslots == 0 || (nslots & (nslots - 1)) || nslots > COPIES_MAX_SLOTS) return hipErrorInvalidValue;
    if (!rows || !base || !ends || !chunks || !wcontig || !sd || !seqw || !nmw || !has_n || !keys || !plane || !partial || !vh)
        return hipErrorInvalidValue;
    const uint32_t NC = (ngenomes + 63) & ~63u;
    const size_t lds = (size_t)2 * 4 * NC * 8 + 8 * 8 + 4 * sizeof(uint2);
#define PG_PLACE_LAUNCH(MAXW, NQ)                                                                                                   \
    hipLaunchKernelGGL((k_sample_agree<MAXW, NQ>), dim3(nchunks), dim3(256), lds, st, ngenomes, k, rows, base, ends, chunks, wcontig, \
                       sd, seqw, nmw, has_n, keys, nslots, max_probe, plane, min_count, partial, vh)
    if (ngenomes <= 128)
        PG_PLACE_LAUNCH(4, 1);
    else if (ngenomes <= 256)
        PG_PLACE_LAUNCH(0, 1);
    else
        PG_PLACE_LAUNCH(0, 2);
#undef PG_PLACE_LAUNCH
    return hipGetLastError();
}

}  // namespace pg
