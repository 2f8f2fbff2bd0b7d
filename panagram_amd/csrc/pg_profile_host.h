// pg_profile_host.h — the host half of the presence profile (pg_profile.hip): the stitch of a window's chunk partials into its
// six fields.  Plain C++ without a GPU call, so that a stand-alone program can hold it to a loop over the rows under the host
// sanitizers (tools/profile_stitch_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace pg {

struct ProfilePartial {  // (two uint4 of k_presence_profile) of one chunk and genome, row numbers relative to the chunk
    uint32_t hits;       // set rows
    uint32_t runs;       // maximal runs of set rows
    uint32_t longest;    // rows of the longest
    uint32_t first, end;  // the first set row, one past the last; 0, 0 without one
    uint32_t gapsum;     // sum of min(k - 1, L) over the runs of L absent rows between two set rows of the chunk
    uint32_t head, tail;  // set rows from the chunk's first row on / up to its last row (both the chunk's rows when all are set)
};
struct ProfileRows {  // (a uint2 of k_presence_profile) of one chunk
    uint32_t all, none;  // rows with every selected genome's bit / with none
};

constexpr uint32_t PROFILE_FIELDS = 6;  // hits, runs, longest, first, end, covered

// Window i's chunks are [first[i], first[i + 1]), in order, chunk_rows rows each but the last; parts[chunk * N + g].
// Per (window, selected genome g) the chunks are folded in order: counts add; a gap between two set rows that a chunk edge
// cuts — the absent rows behind the last set row so far, whole-absent chunks and the next chunk's absent head — is clipped to
// k - 1 ONCE, as a whole; a run of set rows that ends at a chunk's last row and goes on at the next one's first is one run,
// and its rows, over any number of all-present chunks, compete for `longest`.  covered = hits + the clipped gaps + (k - 1 when
// hits > 0): the bases of the window's n + k - 1 that lie in a held k-mer.
// profile_out[(i * N + g) * 6 + {0..5}] = hits, runs, longest, first, end, covered (window-relative; the caller keeps n + k - 1
// below 2^32), zeros for a genome outside `select` and for an empty window; rows_out[i * 2 + {0, 1}] = the sums of the chunks'
// {all, none}.
inline void profile_stitch(uint32_t N, uint32_t nwin, const uint64_t *starts, const uint64_t *ends, const uint64_t *first,
                           uint32_t chunk_rows, const ProfilePartial *parts, const ProfileRows *rows, const uint32_t *select,
                           uint32_t k, uint32_t *profile_out, uint32_t *rows_out) {
    const uint64_t k1 = k - 1;
    for (uint32_t i = 0; i < nwin; ++i) {
        uint64_t all = 0, none = 0;
        for (uint64_t c = first[i]; c < first[i + 1]; ++c) all += rows[c].all, none += rows[c].none;
        rows_out[(size_t)i * 2] = (uint32_t)all;
        rows_out[(size_t)i * 2 + 1] = (uint32_t)none;
        for (uint32_t g = 0; g < N; ++g) {
            uint32_t *out = profile_out + ((size_t)i * N + g) * PROFILE_FIELDS;
            std::fill(out, out + PROFILE_FIELDS, 0u);
            if (!((select[g >> 5] >> (g & 31)) & 1u)) continue;
            uint64_t hits = 0, runs = 0, longest = 0, wfirst = 0, wend = 0, gapsum = 0;
            uint64_t open_p = 0;  // set rows up to the last row folded so far
            uint64_t open_a = 0;  // absent rows behind the last set row (every row so far without one)
            uint64_t off = 0;     // rows folded so far
            for (uint64_t c = first[i]; c < first[i + 1]; ++c) {
                const uint64_t c0 = starts[i] + (c - first[i]) * chunk_rows, n = std::min<uint64_t>(chunk_rows, ends[i] - c0);
                const ProfilePartial &p = parts[c * N + g];
                if (p.hits == 0) {  // no set row in this chunk
                    open_a += n;
                    open_p = 0;
                    off += n;
                    continue;
                }
                if (hits == 0) {
                    wfirst = off + p.first;
                    runs = p.runs;
                    open_p = 0;
                } else if (open_a + p.first) {  // a gap between two set rows, closed here
                    gapsum += std::min<uint64_t>(k1, open_a + p.first);
                    runs += p.runs;
                    open_p = 0;
                } else {  // the run open at the last chunk's end goes on
                    runs += p.runs - 1;
                    longest = std::max(longest, open_p + p.head);
                }
                hits += p.hits;
                longest = std::max<uint64_t>(longest, p.longest);
                gapsum += p.gapsum;
                wend = off + p.end;
                open_p = p.hits == n ? open_p + n : p.tail;
                open_a = n - p.end;
                off += n;
            }
            out[0] = (uint32_t)hits;
            out[1] = (uint32_t)runs;
            out[2] = (uint32_t)longest;
            out[3] = (uint32_t)wfirst;
            out[4] = (uint32_t)wend;
            out[5] = (uint32_t)(hits ? hits + gapsum + k1 : 0);
        }
    }
}

}  // namespace pg
