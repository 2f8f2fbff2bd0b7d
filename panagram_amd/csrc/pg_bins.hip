// pg_bins.hip — masked per-bin column sums of a finished bitmap ON THE GPU (gfx950): the binning step of the
// introgression caller (panagram/introgressions/call_introgressions.py: bitmap_to_bins).
//
// A bin is a range [s, e) of SAMPLED rows of one contig: sampled row j is row j * stride of the contig's rows (bitmap.1 or
// the low-resolution bitmap, as inflated into a result).  Per row, in this order:
//   keep mask    a row with none of the `keep` bits set gets them ORed in (--rmu: reference + outgroup accessions)
//   omit fixed   with `omit_fixed`, a row whose N bits are then all set is dropped (--rmf)
// and per bin the kernel emits the per-genome column sums of the rows left, cs[bin][N], and their number, kept[bin].
// Only the first N bits of a row count: the bits past N in its last byte are masked off.
//
// grid = (bins, pieces), 256 threads: piece p of a bin takes its 256-row groups p, p + pieces, ...; a wave 64 sampled
// rows at a time, one per lane.  A row word's 32 bits are 32 ballots; their popcounts (wave-uniform) are gathered into
// lane b's register for bit b, then ONE ds_add per word and 64 rows lands them in the wave's own LDS counters (no LDS
// atomic per row or per bit).  The block flushes its four waves' counters once, as 64-bit global atomics.
// A wave's counter never exceeds the rows it visits, at most a quarter of the bin plus 64 — below 2^32 for any contig (a
// contig's rows are counted in 32 bits) — and the block sums its waves in 64 bits.
#include "pg_kernels.h"
#include "pg_rowread.h"

namespace pg {

// word d (ng of its bits) of the wave's 64 rows -> the wave's counters wc[32 d ..]
__device__ __forceinline__ void bins_count_word(uint32_t w, uint32_t d, uint32_t N, uint32_t *wc, uint32_t lane) {
    if (__ballot(w != 0) == 0) return;  // (wave-uniform: nothing to count)
    const uint32_t ng = min(32u, N - 32 * d);
    uint32_t mine = 0;  // lane b: the count of bit b over the 64 rows
    // (unrolled by 8, not 32: the full unroll keeps 32 ballot masks live and spills SGPRs into VGPR lanes)
#pragma unroll 8
    for (uint32_t b = 0; b < 32; ++b) {
        if (b < ng) {
            const uint32_t c = (uint32_t)__popcll(__ballot((w >> b) & 1u));
            mine += lane == b ? c : 0u;
        }
    }
    if (lane < ng && mine) atomicAdd(&wc[32 * d + lane], mine);
}

// MAXW = 4: rows of up to 16 bytes (N <= 128), the row's words held in registers between the two passes; MAXW = 0: any
// width, the words read again for the second pass (from the cache).  WHOLE: rows of whole words, read by aligned loads; the
// kernel of all other rows has no test for them (N = 8 and 16 run as they did before there was one: profiles/intros_rate.txt)
template <uint32_t MAXW, bool WHOLE>
__global__ __launch_bounds__(256) void k_bin_colsums(uint32_t N, const uint8_t *__restrict__ rows, uint32_t stride,
                                                     const uint64_t *__restrict__ base, const uint64_t *__restrict__ starts,
                                                     const uint64_t *__restrict__ ends, const uint32_t *__restrict__ keep,
                                                     uint32_t omit_fixed, unsigned long long *__restrict__ cs_out,
                                                     unsigned long long *__restrict__ kept_out) {
    extern __shared__ uint32_t bsm[];  // [4 waves][N] counters, then [4] kept rows
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < 4 * N + 4; i += 256) bsm[i] = 0;
    __syncthreads();
    uint32_t *wc = bsm + wave * N;
    const uint32_t nbytes = (N + 7) / 8, ndw = (N + 31) / 32;
    const uint8_t *crow = rows + base[blockIdx.x];
    const uint64_t s = starts[blockIdx.x], e = ends[blockIdx.x];
    uint32_t kept = 0;
    uint32_t kw[MAXW ? MAXW : 1];
#pragma unroll
    for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) kw[d] = MAXW && d < ndw ? keep[d] : 0u;
    for (uint64_t g0 = s + 256ull * blockIdx.y; g0 < e; g0 += 256ull * gridDim.y) {
        const uint64_t j = g0 + tid;
        const bool act = j < e;
        const uint8_t *p = crow + j * stride * nbytes;
        // pass 1: any keep bit? all N bits set as the row stands / with the keep bits ORed in?
        uint32_t anyk = 0;
        bool full_raw = true, full_kept = true;
        uint32_t w[MAXW ? MAXW : 1];
        if (MAXW) {
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
                w[d] = 0;
                if (d < ndw) {
                    const uint32_t vm = valid_bits(N, d);
                    w[d] = act ? row_word<WHOLE>(p, d, nbytes) & vm : 0u;
                    anyk |= w[d] & kw[d];
                    full_raw &= w[d] == vm;
                    full_kept &= (w[d] | kw[d]) == vm;
                }
            }
        } else {
            for (uint32_t d = 0; d < ndw; ++d) {
                const uint32_t vm = valid_bits(N, d), k = keep[d];
                const uint32_t x = act ? row_word<WHOLE>(p, d, nbytes) & vm : 0u;
                anyk |= x & k;
                full_raw &= x == vm;
                full_kept &= (x | k) == vm;
            }
        }
        const bool take = act && !(omit_fixed && (anyk ? full_raw : full_kept));
        kept += (uint32_t)__popcll(__ballot(take));
        // pass 2: the row as transformed, column by column
        if (MAXW) {
#pragma unroll
            for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d)
                if (d < ndw) bins_count_word(take ? (anyk ? w[d] : w[d] | kw[d]) : 0u, d, N, wc, lane);
        } else {
            for (uint32_t d = 0; d < ndw; ++d) {
                const uint32_t k = keep[d];
                const uint32_t x = take ? row_word<WHOLE>(p, d, nbytes) & valid_bits(N, d) : 0u;
                bins_count_word(take ? (anyk ? x : x | k) : 0u, d, N, wc, lane);
            }
        }
    }
    if (lane == 0) bsm[4 * N + wave] = kept;
    __syncthreads();
    for (uint32_t i = tid; i < N; i += 256) {
        const unsigned long long c = (unsigned long long)bsm[i] + bsm[N + i] + bsm[2 * N + i] + bsm[3 * N + i];
        if (c) atomicAdd(&cs_out[(uint64_t)blockIdx.x * N + i], c);
    }
    if (tid == 0) {
        const unsigned long long k = (unsigned long long)bsm[4 * N] + bsm[4 * N + 1] + bsm[4 * N + 2] + bsm[4 * N + 3];
        if (k) atomicAdd(&kept_out[blockIdx.x], k);
    }
}

hipError_t launch_bin_colsums(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, uint32_t nbins,
                              uint32_t pieces, const uint64_t *base, const uint64_t *starts, const uint64_t *ends,
                              const uint32_t *keep, uint32_t omit_fixed, unsigned long long *cs, unsigned long long *kept) {
    if (nbins == 0) return hipSuccess;
    const size_t lds = (4 * (size_t)ngenomes + 4) * 4;
    const bool whole = (ngenomes + 7) / 8 % 4 == 0;
#define PG_BINS_LAUNCH(MAXW, WHOLE)                                                                                              \
    hipLaunchKernelGGL((k_bin_colsums<MAXW, WHOLE>), dim3(nbins, pieces), dim3(256), lds, st, ngenomes, rows, stride, base, starts, \
                       ends, keep, omit_fixed, cs, kept)
    if (ngenomes <= 128) {
        if (whole)
            PG_BINS_LAUNCH(4, true);
        else
            PG_BINS_LAUNCH(4, false);
    } else {
        if (whole)
            PG_BINS_LAUNCH(0, true);
        else
            PG_BINS_LAUNCH(0, false);
    }
#undef PG_BINS_LAUNCH
    return hipGetLastError();
}

}  // namespace pg
