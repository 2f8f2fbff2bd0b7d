// pg_gaps_host.h — the host half of the absence runs (pg_gaps.hip): the stitch step over the chunks' edges and the order of
// the emitted records.  Plain C++ without a GPU call, so that a stand-alone program can hold it to a loop over the rows under
// the host sanitizers (tools/gaps_stitch_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pg {

struct GapEdge {  // (a uint2 of k_absence_runs) of one chunk and genome
    uint32_t head, tail;  // absent rows from the chunk's first row on / up to its last row; both the chunk's rows when none is present
};
struct GapRun {  // (a uint4 of k_absence_runs) one closed run
    uint32_t win, genome, start, rows;  // first sampled row, sampled rows
};

inline bool gaps_selected(uint32_t rows, uint32_t min_len, uint32_t max_len) {
    return rows >= min_len && (max_len == 0 || rows <= max_len);
}

// Window i's chunks are [first[i], first[i + 1]), in order, chunk_rows sampled rows each but the last; edges[chunk * N + g].
// Per (window, selected genome g): a chunk's tail, the chunks behind it without a present row and the head of the first one
// with a present row are ONE run, closed when a present row of the window lies before it: hist[(i * N + g) * (maxlen + 1) +
// min(rows, maxlen)] gets 1, and a run selected for emission goes to `emit` and counts in nruns[i].  The runs that touch the
// window's edges stay open: edge_out[(i * N + g) * 2 + {0, 1}] = the absent rows from the window's first row on / up to its
// last row, both the window's rows when none is present (0 for an empty window).
inline void gaps_stitch(uint32_t N, uint32_t nwin, const uint64_t *starts, const uint64_t *ends, const uint64_t *first,
                        uint32_t chunk_rows, const GapEdge *edges, const uint32_t *select, uint32_t maxlen, uint32_t min_len,
                        uint32_t max_len, uint64_t *hist, uint64_t *edge_out, uint64_t *nruns, std::vector<GapRun> &emit) {
    for (uint32_t i = 0; i < nwin; ++i)
        for (uint32_t g = 0; g < N; ++g) {
            if (!((select[g >> 5] >> (g & 31)) & 1u)) continue;
            uint64_t open = 0, edge_head = 0;
            bool seen = false;
            for (uint64_t c = first[i]; c < first[i + 1]; ++c) {
                const uint64_t c0 = starts[i] + (c - first[i]) * chunk_rows, n = std::min<uint64_t>(chunk_rows, ends[i] - c0);
                const GapEdge &ed = edges[c * N + g];
                if (ed.head >= n) {  // no present row in this chunk
                    open += n;
                    continue;
                }
                const uint64_t rows = open + ed.head;
                if (!seen) {
                    edge_head = rows;
                } else if (rows) {
                    hist[((uint64_t)i * N + g) * (maxlen + 1) + std::min<uint64_t>(rows, maxlen)] += 1;
                    if (gaps_selected((uint32_t)rows, min_len, max_len)) {
                        emit.push_back(GapRun{i, g, (uint32_t)(c0 - open), (uint32_t)rows});
                        nruns[i] += 1;
                    }
                }
                seen = true;
                open = ed.tail;
            }
            edge_out[((uint64_t)i * N + g) * 2] = seen ? edge_head : open;
            edge_out[((uint64_t)i * N + g) * 2 + 1] = open;
        }
}

// by (window, genome, first sampled row): the keys are unique, so the order is the same whatever order the records came in.
// From radix_from records on a stable radix sort, least significant digit first (11 bits a pass: start, genome, window; a pass
// whose digit is the same in every record only counts): the 783 k candidates of 8 genomes over 100 M rows are four scatter
// passes over 12.5 MB, and an emitting call's time is this sort and the copies around it, not the kernel.
inline void gaps_sort(std::vector<GapRun> &runs, size_t radix_from = 4096) {
    if (runs.size() < radix_from) {
        std::sort(runs.begin(), runs.end(), [](const GapRun &a, const GapRun &b) {
            if (a.win != b.win) return a.win < b.win;
            if (a.genome != b.genome) return a.genome < b.genome;
            return a.start < b.start;
        });
        return;
    }
    std::vector<GapRun> other(runs.size());
    std::vector<size_t> at(2049);
    uint32_t GapRun::*const fields[3] = {&GapRun::start, &GapRun::genome, &GapRun::win};
    for (uint32_t GapRun::*f : fields)
        for (uint32_t shift = 0; shift < 32; shift += 11) {
            std::fill(at.begin(), at.end(), 0);
            for (const GapRun &r : runs) ++at[((r.*f >> shift) & 2047u) + 1];
            if (*std::max_element(at.begin(), at.end()) == runs.size()) continue;  // (one digit for all)
            for (size_t d = 0; d < 2048; ++d) at[d + 1] += at[d];
            for (const GapRun &r : runs) other[at[(r.*f >> shift) & 2047u]++] = r;
            runs.swap(other);
        }
}

}  // namespace pg
