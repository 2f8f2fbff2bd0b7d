// pg_copies_host.h — the host half of the copy-number profile (pg_copies.hip): the sum of a target contig's chunk partials into
// its histograms.  Plain C++ without a GPU call, as pg_profile_host.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pg {

// Contig t's chunks are [first[t], first[t + 1]), partial[(chunk * nplanes + g) * bins + c] and valid_partial[chunk] as
// k_copy_profile leaves them (32-bit, at most a chunk's positions each).  The sums are taken in 64 bits:
// hist_out[(t * nplanes + g) * bins + c] and valid_out[t]; zeros for a contig without a chunk.
inline void copies_stitch(uint32_t ncontigs, const uint64_t *first, uint32_t nplanes, uint32_t bins, const uint32_t *partial,
                          const uint32_t *valid_partial, uint64_t *hist_out, uint64_t *valid_out) {
    const size_t row = (size_t)nplanes * bins;
    for (uint32_t t = 0; t < ncontigs; ++t) {
        uint64_t *h = hist_out + (size_t)t * row;
        for (size_t j = 0; j < row; ++j) h[j] = 0;
        uint64_t valid = 0;
        for (uint64_t c = first[t]; c < first[t + 1]; ++c) {
            const uint32_t *p = partial + (size_t)c * row;
            for (size_t j = 0; j < row; ++j) h[j] += p[j];
            valid += valid_partial[c];
        }
        valid_out[t] = valid;
    }
}

}  // namespace pg
