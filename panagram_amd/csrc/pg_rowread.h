// pg_rowread.h — how the window-query kernels (pg_bins.hip, pg_pairs.hip, pg_find.hip, pg_patterns.hip) read one finished bitmap
// row of nbytes = ceil(N / 8) bytes at p: never a byte outside the row.
//
// Alignment, once for all of them: a contig's rows start on 16 bytes, and sampled row j is j * stride * nbytes bytes further
// on.  With nbytes % 4 == 0 that is a multiple of 4, so every word of every sampled row is an aligned 32-bit load (with
// nbytes % 8 == 0 its first 8 bytes an aligned 64-bit one); rows of any other width are read byte by byte.
#pragma once
#include <cstdint>

namespace pg {

// bytes [4d, min(4d + 4, nbytes)) of a row as a little-endian word.  ALIGNED = false: the byte loop whatever the width, for a
// kernel that is built apart for rows that are no whole words (k_bin_colsums, where the test below cost those rows 0.4 %)
template <bool ALIGNED = true>
__device__ __forceinline__ uint32_t row_word(const uint8_t *__restrict__ p, uint32_t d, uint32_t nbytes) {
    if (ALIGNED && (nbytes & 3u) == 0) return *reinterpret_cast<const uint32_t *>(p + 4 * d);
    const uint32_t nb = min(4u, nbytes - 4 * d);
    uint32_t v = 0;
    for (uint32_t b = 0; b < nb; ++b) v |= (uint32_t)p[4 * d + b] << (8 * b);
    return v;
}

// bytes [0, min(8, nbytes)) of a row, zero-extended
__device__ __forceinline__ uint64_t row_low(const uint8_t *__restrict__ p, uint32_t nbytes) {
    if ((nbytes & 7u) == 0) return *reinterpret_cast<const uint64_t *>(p);
    if ((nbytes & 3u) == 0) {
        const uint64_t lo = *reinterpret_cast<const uint32_t *>(p);
        return nbytes > 4 ? lo | (uint64_t)*reinterpret_cast<const uint32_t *>(p + 4) << 32 : lo;
    }
    const uint32_t nb = min(8u, nbytes);
    uint64_t v = 0;
    for (uint32_t b = 0; b < nb; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// the bits of row word d that are genomes: the bits at and past N in a row's last byte are masked off with this
__device__ __forceinline__ uint32_t valid_bits(uint32_t N, uint32_t d) {
    const uint32_t ng = N - 32 * d;
    return ng >= 32 ? 0xFFFFFFFFu : (1u << ng) - 1u;
}

}  // namespace pg
