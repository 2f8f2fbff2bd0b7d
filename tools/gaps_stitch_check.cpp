// gaps_stitch_check.cpp — the host half of the absence runs (panagram_amd/csrc/pg_gaps_host.h: gaps_stitch, gaps_sort) held to a
// loop over the rows, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o gaps_stitch_check tools/gaps_stitch_check.cpp
//   ./gaps_stitch_check        (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
// Random absence columns — dense ones, ones with runs longer than several chunks, columns absent or present throughout — are
// cut into windows and chunks of a few rows.  What k_absence_runs leaves per chunk (head, tail, the runs closed inside the
// chunk) is computed by a loop; gaps_stitch's spectrum, edges, counts and records, merged with the chunks' own and sorted, must
// equal those of a loop over the whole window.
#include "../panagram_amd/csrc/pg_gaps_host.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace pg;

struct Found {
    std::vector<GapRun> runs;  // closed runs, selected or not
    uint64_t head = 0, tail = 0;
};

// the closed runs and the two open ones of rows [s, e) of column `a` (1 = absent)
static Found walk(const std::vector<uint8_t> &a, uint64_t s, uint64_t e, uint32_t win, uint32_t g) {
    Found f;
    uint64_t len = 0;
    bool seen = false;
    for (uint64_t j = s; j < e; ++j) {
        if (a[j]) {
            ++len;
            continue;
        }
        if (len && seen) f.runs.push_back(GapRun{win, g, (uint32_t)(j - len), (uint32_t)len});
        if (len && !seen) f.head = len;
        seen = true;
        len = 0;
    }
    f.tail = len;
    if (!seen) f.head = len;
    return f;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    std::mt19937_64 rng(7);
    uint64_t cases = 0, joined = 0;
    for (uint32_t round = 0; round < 300; ++round) {
        const uint32_t N = 1 + rng() % 70, chunk = 1 + rng() % 9, nrows = rng() % 200, nwin = 1 + rng() % 5;
        const uint32_t maxlen = 1 + rng() % 12, min_len = 1 + rng() % 4, max_len = rng() % 3 ? 0 : min_len + rng() % 20;
        std::vector<std::vector<uint8_t>> col(N, std::vector<uint8_t>(nrows));
        std::vector<uint32_t> select((N + 31) / 32, 0);
        for (uint32_t g = 0; g < N; ++g) {
            const uint32_t kind = rng() % 5;
            uint8_t v = 0;
            for (uint32_t j = 0; j < nrows; ++j) {
                if (kind == 0) v = rng() & 1;                        // dense
                if (kind == 1 && rng() % (3 * chunk) == 0) v = !v;   // runs of several chunks
                if (kind == 2) v = 1;                                // absent throughout
                if (kind == 3) v = 0;                                // present throughout
                if (kind == 4) v = rng() % 8 != 0;                   // mostly absent
                col[g][j] = v;
            }
            if (rng() % 6) select[g >> 5] |= 1u << (g & 31);
        }
        std::vector<uint64_t> starts(nwin), ends(nwin), first(nwin + 1, 0);
        std::vector<GapEdge> edges;
        std::vector<uint64_t> hist((size_t)nwin * N * (maxlen + 1), 0), edge_out((size_t)nwin * N * 2, 0), nruns(nwin, 0);
        std::vector<GapRun> records, want;
        std::vector<uint64_t> want_hist(hist.size(), 0), want_nruns(nwin, 0);
        for (uint32_t i = 0; i < nwin; ++i) {
            starts[i] = nrows ? rng() % (nrows + 1) : 0;
            ends[i] = starts[i] + (nrows > starts[i] ? rng() % (nrows - starts[i] + 1) : 0);
            if (i == 0) starts[i] = 0, ends[i] = nrows;
            for (uint64_t c0 = starts[i]; c0 < ends[i]; c0 += chunk) {  // what the kernel leaves for this chunk
                const uint64_t ce = std::min<uint64_t>(c0 + chunk, ends[i]);
                for (uint32_t g = 0; g < N; ++g) {
                    const bool sel = (select[g >> 5] >> (g & 31)) & 1u;
                    const Found f = walk(col[g], c0, ce, i, g);
                    edges.push_back(sel ? GapEdge{(uint32_t)f.head, (uint32_t)f.tail} : GapEdge{0xDEADBEEFu, 0xDEADBEEFu});
                    if (!sel) continue;
                    for (const GapRun &r : f.runs) {
                        hist[((size_t)i * N + g) * (maxlen + 1) + std::min(r.rows, maxlen)] += 1;
                        if (gaps_selected(r.rows, min_len, max_len)) records.push_back(r), nruns[i] += 1;
                    }
                }
            }
            first[i + 1] = edges.size() / N;
            for (uint32_t g = 0; g < N; ++g) {  // the whole window by the loop
                if (!((select[g >> 5] >> (g & 31)) & 1u)) continue;
                const Found f = walk(col[g], starts[i], ends[i], i, g);
                for (const GapRun &r : f.runs) {
                    want_hist[((size_t)i * N + g) * (maxlen + 1) + std::min(r.rows, maxlen)] += 1;
                    if (gaps_selected(r.rows, min_len, max_len)) want.push_back(r), want_nruns[i] += 1;
                }
                edge_out[((size_t)i * N + g) * 2] = edge_out[((size_t)i * N + g) * 2 + 1] = ~0ull;  // (the stitch must write both)
            }
        }
        const size_t in_chunks = records.size();
        std::shuffle(records.begin(), records.end(), rng);  // (the kernel's cursor hands out places in any order)
        gaps_stitch(N, nwin, starts.data(), ends.data(), first.data(), chunk, edges.data(), select.data(), maxlen, min_len, max_len,
                    hist.data(), edge_out.data(), nruns.data(), records);
        joined += records.size() - in_chunks;
        gaps_sort(records, round % 2 ? 4096 : 2);  // (every other round: the radix passes whatever the number of records)
        CHECK(hist == want_hist);
        CHECK(nruns == want_nruns);
        CHECK(records.size() == want.size());
        for (size_t r = 0; r < want.size(); ++r)  // (the loop went window by window, genome by genome, row by row: sorted)
            CHECK(records[r].win == want[r].win && records[r].genome == want[r].genome && records[r].start == want[r].start &&
                  records[r].rows == want[r].rows);
        for (uint32_t i = 0; i < nwin; ++i)
            for (uint32_t g = 0; g < N; ++g) {
                const bool sel = (select[g >> 5] >> (g & 31)) & 1u;
                const Found f = walk(col[g], starts[i], ends[i], i, g);
                CHECK(edge_out[((size_t)i * N + g) * 2] == (sel ? f.head : 0));
                CHECK(edge_out[((size_t)i * N + g) * 2 + 1] == (sel ? f.tail : 0));
            }
        ++cases;
    }
    // the radix passes at a size that takes them by itself, with digits above the lowest in every field: against the comparison sort
    std::vector<GapRun> big(50000);
    for (size_t i = 0; i < big.size(); ++i) big[i] = GapRun{(uint32_t)(rng() % 3000), (uint32_t)(rng() % 512), (uint32_t)i * 85899u, (uint32_t)rng()};
    std::shuffle(big.begin(), big.end(), rng);
    std::vector<GapRun> by_radix = big;
    gaps_sort(by_radix);
    gaps_sort(big, big.size() + 1);
    for (size_t i = 0; i < big.size(); ++i)
        CHECK(big[i].win == by_radix[i].win && big[i].genome == by_radix[i].genome && big[i].start == by_radix[i].start && big[i].rows == by_radix[i].rows);
    std::printf("ok: %llu cases, %llu runs joined across chunks\n", (unsigned long long)cases, (unsigned long long)joined);
    return joined > 1000 ? 0 : 1;
}
