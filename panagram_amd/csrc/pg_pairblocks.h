// pg_pairblocks.h — what the two pair-count kernels share (k_pair_counts over bitmap rows in pg_pairs.hip, k_table_pair_counts
// over the pan table's slots in pg_tablestats.hip): the ballot transpose of a wave's 64 mask words into column words, and the
// per-thread 4 x 4 blocks of the upper triangle that add popcounts of column-word pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pg {

constexpr uint32_t PAIRS_TILE = 256;  // sampled rows / table slots per tile: one 64-row word per wave
constexpr uint32_t PAIRS_ROUNDS = 3;  // 4 x 4 blocks per thread and slice

// word d of the wave's 64 rows: the column word of bit b goes to lane b (d even) / 32 + b (d odd)
__device__ __forceinline__ uint64_t pairs_ballot_word(uint32_t w, uint32_t d, uint32_t N, uint32_t lane, uint64_t mine) {
    if (__ballot(w != 0) == 0) return mine;  // (wave-uniform: no bit in these 32 columns)
    const uint32_t ng = min(32u, N - 32 * d), l0 = 32 * (d & 1);
    // (unrolled by 8, not 32: the full unroll keeps 32 ballot masks live and spills SGPRs into VGPR lanes)
#pragma unroll 8
    for (uint32_t b = 0; b < 32; ++b) {
        if (b < ng) {
            const uint64_t m = __ballot((w >> b) & 1u);
            mine = lane == l0 + b ? m : mine;
        }
    }
    return mine;
}

// A thread's blocks of one slice: blocks t, t + 256, t + 512 of the slice's 768 (ROUNDS = 3), t numbering the 4 x 4 blocks on and above the
// diagonal row by row, with their 16 counters each in registers.  A counter is 32 bits wide: the caller keeps the rows (slots)
// one thread block visits below 2^32.  ROUNDS = 1 is for a kernel that knows its blocks fit one round: 16 counters instead
// of 48.
template <uint32_t ROUNDS = PAIRS_ROUNDS>
struct PairBlocks {
    uint32_t ca[ROUNDS], cb[ROUNDS];
    bool have[ROUNDS];
    uint32_t acc[ROUNDS][16];

    // (threads: how many share the slice's blocks — the 256 of a thread block, or the 64 of a wave that keeps its own counters)
    __device__ __forceinline__ void init(uint32_t tid, uint32_t slice, uint32_t N, uint32_t threads = 256) {
        const uint32_t NB = (N + 3) / 4, nblk = NB * (NB + 1) / 2;
#pragma unroll
        for (uint32_t r = 0; r < ROUNDS; ++r) {
            const uint32_t t = (slice * ROUNDS + r) * threads + tid;
            have[r] = t < nblk;
            uint32_t a = 0, rem = have[r] ? t : 0;
            while (rem >= NB - a) {
                rem -= NB - a;
                ++a;
            }
            ca[r] = 4 * a;
            cb[r] = 4 * (a + rem);
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) acc[r][i] = 0;
        }
    }
    // one wave's column words (cols[c] = the 64-row word of column c) into block r: two 16-byte LDS reads each side
    __device__ __forceinline__ void add(uint32_t r, const uint64_t *cols) {
        const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(cols + ca[r]);
        const ulonglong2 *pb = reinterpret_cast<const ulonglong2 *>(cols + cb[r]);
        const ulonglong2 a01 = pa[0], a23 = pa[1], b01 = pb[0], b23 = pb[1];
        const uint64_t A[4] = {a01.x, a01.y, a23.x, a23.y}, B[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) acc[r][4 * i + k] += (uint32_t)__popcll(A[i] & B[k]);
    }
    // one 64-bit global atomic add per non-zero pair: the entries on and above the diagonal (and the few below it inside the
    // diagonal blocks).  The caller mirrors them into the lower triangle.
    __device__ __forceinline__ void flush(unsigned long long *out, uint32_t N) const {
#pragma unroll
        for (uint32_t r = 0; r < ROUNDS; ++r) {
            if (!have[r]) continue;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t a = ca[r] + i, b = cb[r] + k, c = acc[r][4 * i + k];
                    if (a < N && b < N && c) atomicAdd(&out[(uint64_t)a * N + b], (unsigned long long)c);
                }
        }
    }
};

}  // namespace pg
