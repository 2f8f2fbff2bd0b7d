// pg_pairs.hip — pair counts of a finished bitmap's rows ON THE GPU (gfx950): C[a][b] = rows of a window holding both genome
// a's and genome b's bit, the one integer matrix the viewer's tree of the genomes over a region needs (panagram/view.py:
// 751-764: create_tree runs linkage(bitmap.T, "ward", "euclidean"); diag(C) are the column sums, C[a][a] + C[b][b] - 2 C[a][b]
// the squared Euclidean distance of two 0/1 columns).
//
// A window is a range [s, e) of SAMPLED rows of one contig, as in pg_bins.hip: sampled row j is row j * stride of the contig's
// rows (bitmap.1 or the low-resolution bitmap, as inflated into a result).  Only the first N bits of a row count: the bits
// past N in its last byte are masked off.
//
// grid = (windows, pieces, slices), 256 threads: piece p of a window takes its 256-row tiles p, p + pieces, ...
//   transpose  a wave takes 64 sampled rows of the tile, one per lane; the ballot of bit c over the wave IS the 64-row word
//              of column c.  Lane c % 64 keeps it, and after every 64 columns the wave stores one word per lane:
//              tile[wave][c] in LDS, 4 words per column and tile, columns past N zero.
//   pairs      the N x N matrix is cut into 4 x 4 blocks, and only the blocks on and above the diagonal are computed.  A thread
//              owns blocks t, t + 256, t + 512 of its slice (PAIRS_ROUNDS = 3: the 528 blocks of N = 128 are one slice) with
//              their 16 counters each in registers across all tiles of the piece: per tile and word it reads its 4 + 4
//              column words (two 16-byte LDS reads each side) and adds popcount(col_a & col_b) for the 16 pairs.
//              Wider rows have more blocks than 3 x 256: slice z of the grid takes blocks [768 z, 768 (z + 1)) and repeats
//              the transpose for itself.  Two tile buffers, so one barrier per tile.
//   flush      one 64-bit global atomic add per non-zero pair of the thread's blocks: the entries on and above the diagonal
//              (and the few below it inside the diagonal blocks).  The caller mirrors them into the lower triangle.
// A thread's counter is 32 bits wide: it never exceeds the sampled rows its block visits, which are rows of ONE contig,
// and a contig's rows are counted in 32 bits (AnchorDesc::nkmers) — so it stays below 2^32; the sums across blocks are
// 64-bit atomics.
// N <= 128 (k_pair_counts<4>): a lane loads its row's words once, into registers, before the ballots; beyond, up to
// PAIRS_MAX_GENOMES (k_pair_counts<0>), word by word.
#include "pg_kernels.h"
#include "pg_rowread.h"
#include "pg_pairblocks.h"

namespace pg {

template <uint32_t MAXW>
__global__ __launch_bounds__(256) void k_pair_counts(uint32_t N, const uint8_t *__restrict__ rows, uint32_t stride,
                                                     const uint64_t *__restrict__ base, const uint64_t *__restrict__ starts,
                                                     const uint64_t *__restrict__ ends, unsigned long long *__restrict__ pairs_out) {
    extern __shared__ __align__(16) uint64_t psm[];  // [2 buffers][4 waves][NC] column words
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    const uint32_t NC = (N + 63) & ~63u;
    // this thread's blocks: number t of the blocks on and above the diagonal, row by row -> (block row, block column)
    PairBlocks<> pb;  // (pg_pairblocks.h, shared with k_table_pair_counts)
    pb.init(tid, blockIdx.z, N);
    const uint8_t *crow = rows + base[blockIdx.x];
    const uint64_t s = starts[blockIdx.x], e = ends[blockIdx.x];
    uint32_t buf = 0;
    for (uint64_t g0 = s + (uint64_t)PAIRS_TILE * blockIdx.y; g0 < e; g0 += (uint64_t)PAIRS_TILE * gridDim.y, buf ^= 1) {
        const uint64_t j = g0 + tid;
        const bool act = j < e;
        const uint8_t *p = crow + j * stride * nbytes;
        uint64_t *tile = psm + (size_t)buf * 4 * NC;
        uint64_t *mycols = tile + wave * NC;
        if (MAXW) {
            uint32_t w[MAXW ? MAXW : 1];
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d)
                w[d] = act && d < ndw ? row_word(p, d, nbytes) & valid_bits(N, d) : 0u;
            uint64_t mine = 0;
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
                if (d < ndw) mine = pairs_ballot_word(w[d], d, N, lane, mine);
                if ((d & 1) && 32 * (d - 1) < NC) {
                    mycols[32 * (d - 1) + lane] = mine;
                    mine = 0;
                }
            }
        } else {
            for (uint32_t q = 0; 64 * q < NC; ++q) {
                uint64_t mine = 0;
                for (uint32_t d = 2 * q; d < min(2 * q + 2, ndw); ++d)
                    mine = pairs_ballot_word(act ? row_word(p, d, nbytes) & valid_bits(N, d) : 0u, d, N, lane, mine);
                mycols[64 * q + lane] = mine;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < PAIRS_ROUNDS; ++r) {
            if (!pb.have[r]) continue;
#pragma unroll
            for (uint32_t wv = 0; wv < 4; ++wv) pb.add(r, tile + wv * NC);
        }
        // (no second barrier: the next tile goes to the other buffer, and this one is written again only behind the next
        // tile's barrier, which every wave passes after these reads)
    }
    pb.flush(pairs_out + (uint64_t)blockIdx.x * N * N, N);
}

hipError_t launch_pair_counts(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, uint32_t nwin,
                              uint32_t pieces, const uint64_t *base, const uint64_t *starts, const uint64_t *ends,
                              unsigned long long *pairs) {
    if (nwin == 0) return hipSuccess;
    if (ngenomes < 1 || ngenomes > PAIRS_MAX_GENOMES) return hipErrorInvalidValue;
    const uint32_t NC = (ngenomes + 63) & ~63u, NB = (ngenomes + 3) / 4, nblk = NB * (NB + 1) / 2;
    const uint32_t slices = (nblk + PAIRS_ROUNDS * 256 - 1) / (PAIRS_ROUNDS * 256);
    const size_t lds = (size_t)2 * 4 * NC * 8;
    if (ngenomes <= 128)
        hipLaunchKernelGGL(k_pair_counts<4>, dim3(nwin, pieces, slices), dim3(256), lds, st, ngenomes, rows, stride, base, starts,
                           ends, pairs);
    else
        hipLaunchKernelGGL(k_pair_counts<0>, dim3(nwin, pieces, slices), dim3(256), lds, st, ngenomes, rows, stride, base, starts,
                           ends, pairs);
    return hipGetLastError();
}

}  // namespace pg
