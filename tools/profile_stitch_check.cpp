// profile_stitch_check.cpp — the host half of the presence profile (panagram_amd/csrc/pg_profile_host.h: profile_stitch) held to a
// loop over the whole vector, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o profile_stitch_check tools/profile_stitch_check.cpp
//   ./profile_stitch_check     (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
// Presence columns — random dense and sparse ones, ones with runs and gaps longer than several chunks, columns set or clear
// throughout, and crafted ones (gaps of k - 2, k - 1 and k rows, a single set row, the longest run at either end) — are cut into
// chunks of 4, 5 and 64 rows.  The window starts at every offset 0 .. chunk - 1 of the vector, so that a chunk edge falls on
// every position of it.  What k_presence_profile leaves per chunk is computed by a loop over the chunk's rows; profile_stitch's
// six fields must equal those of a loop over the whole window, whose `covered` comes from marking bases, not from the identity.
#include "../panagram_amd/csrc/pg_profile_host.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace pg;

// what the kernel leaves for rows [s, e) of column `p` (1 = set), by the definitions
static ProfilePartial chunk_partial(const std::vector<uint8_t> &p, uint64_t s, uint64_t e, uint32_t k) {
    ProfilePartial r{0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t run = 0, gap = 0;
    bool seen = false;
    for (uint64_t j = s; j < e; ++j) {
        if (p[j]) {
            if (run == 0) {
                ++r.runs;
                if (seen) r.gapsum += (uint32_t)std::min<uint64_t>(k - 1, gap);
                if (!seen) r.first = (uint32_t)(j - s);
            }
            seen = true;
            ++r.hits;
            ++run;
            gap = 0;
            r.longest = std::max(r.longest, (uint32_t)run);
            r.end = (uint32_t)(j - s + 1);
        } else {
            run = 0;
            ++gap;
        }
    }
    r.tail = (uint32_t)run;
    for (uint64_t j = s; j < e && p[j]; ++j) ++r.head;
    return r;
}

// the six fields of rows [s, e) by the definitions: covered by marking the bases [j, j + k) of every set row
static void whole(const std::vector<uint8_t> &p, uint64_t s, uint64_t e, uint32_t k, uint32_t out[6]) {
    const uint64_t n = e - s;
    std::vector<uint8_t> base(n + k, 0);
    uint32_t hits = 0, runs = 0, longest = 0, first = 0, end = 0, run = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (!p[s + j]) {
            run = 0;
            continue;
        }
        if (!hits) first = (uint32_t)j;
        ++hits;
        if (run++ == 0) ++runs;
        longest = std::max(longest, run);
        end = (uint32_t)j + 1;
        for (uint32_t b = 0; b < k; ++b) base[j + b] = 1;
    }
    uint32_t covered = 0;
    for (uint8_t b : base) covered += b;
    const uint32_t f[6] = {hits, runs, longest, first, end, covered};
    std::copy(f, f + 6, out);
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static uint64_t cases = 0, joined = 0;

// N columns of nrows rows, k, one chunk size: windows [s, nrows) for s = 0 .. chunk - 1, an empty one and a random one
static int check(const std::vector<std::vector<uint8_t>> &col, uint32_t nrows, uint32_t k, uint32_t chunk, std::mt19937_64 &rng) {
    const uint32_t N = (uint32_t)col.size();
    std::vector<uint32_t> select((N + 31) / 32, 0);
    for (uint32_t g = 0; g < N; ++g)
        if (g == 0 || rng() % 6) select[g >> 5] |= 1u << (g & 31);
    std::vector<uint64_t> starts, ends;
    for (uint32_t s = 0; s < chunk && s <= nrows; ++s) starts.push_back(s), ends.push_back(nrows);
    starts.push_back(nrows / 2), ends.push_back(nrows / 2);  // empty
    const uint64_t a = nrows ? rng() % nrows : 0;
    starts.push_back(a), ends.push_back(a + (nrows ? rng() % (nrows - a + 1) : 0));
    const uint32_t nwin = (uint32_t)starts.size();
    std::vector<uint64_t> first(nwin + 1, 0);
    std::vector<ProfilePartial> parts;
    std::vector<ProfileRows> rows;
    std::vector<uint32_t> want_rows(2 * (size_t)nwin, 0);
    for (uint32_t i = 0; i < nwin; ++i) {
        for (uint64_t c0 = starts[i]; c0 < ends[i]; c0 += chunk) {
            const uint64_t ce = std::min<uint64_t>(c0 + chunk, ends[i]);
            for (uint32_t g = 0; g < N; ++g) {
                const bool sel = (select[g >> 5] >> (g & 31)) & 1u;
                // (the kernel writes zeros for a column outside the selection; the stitch must not read them)
                parts.push_back(sel ? chunk_partial(col[g], c0, ce, k)
                                    : ProfilePartial{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu});
            }
            ProfileRows pr{0, 0};
            for (uint64_t j = c0; j < ce; ++j) {
                bool every = true, any = false;
                for (uint32_t g = 0; g < N; ++g)
                    if ((select[g >> 5] >> (g & 31)) & 1u) every = every && col[g][j], any = any || col[g][j];
                pr.all += every, pr.none += !any;
            }
            rows.push_back(pr);
            want_rows[2 * (size_t)i] += pr.all, want_rows[2 * (size_t)i + 1] += pr.none;
        }
        first[i + 1] = rows.size();
        if (first[i + 1] - first[i] > 1) ++joined;
    }
    std::vector<uint32_t> got((size_t)nwin * N * 6, 0xABABABABu), got_rows(2 * (size_t)nwin, 0xABABABABu);
    profile_stitch(N, nwin, starts.data(), ends.data(), first.data(), chunk, parts.data(), rows.data(), select.data(), k, got.data(),
                   got_rows.data());
    CHECK(got_rows == want_rows);
    for (uint32_t i = 0; i < nwin; ++i)
        for (uint32_t g = 0; g < N; ++g) {
            uint32_t want[6] = {0, 0, 0, 0, 0, 0};
            if ((select[g >> 5] >> (g & 31)) & 1u) whole(col[g], starts[i], ends[i], k, want);
            for (uint32_t f = 0; f < 6; ++f)
                if (got[((size_t)i * N + g) * 6 + f] != want[f]) {
                    std::fprintf(stderr, "rows [%llu, %llu) chunk %u k %u genome %u field %u: %u, want %u\n",
                                 (unsigned long long)starts[i], (unsigned long long)ends[i], chunk, k, g, f,
                                 got[((size_t)i * N + g) * 6 + f], want[f]);
                    return 1;
                }
        }
    ++cases;
    return 0;
}

int main() {
    std::mt19937_64 rng(11);
    const uint32_t chunks[3] = {4, 5, 64};
    // random columns
    for (uint32_t round = 0; round < 240; ++round) {
        const uint32_t chunk = chunks[round % 3], N = 1 + rng() % 40, nrows = rng() % (chunk == 64 ? 400 : 60), k = 1 + rng() % 32;
        std::vector<std::vector<uint8_t>> col(N, std::vector<uint8_t>(nrows));
        for (uint32_t g = 0; g < N; ++g) {
            const uint32_t kind = rng() % 6;
            uint8_t v = rng() & 1;
            for (uint32_t j = 0; j < nrows; ++j) {
                if (kind == 0) v = rng() & 1;                       // dense
                if (kind == 1 && rng() % (3 * chunk) == 0) v = !v;  // runs and gaps of several chunks
                if (kind == 2) v = 1;                               // set throughout
                if (kind == 3) v = 0;                               // clear throughout
                if (kind == 4) v = rng() % 8 != 0;                  // mostly set
                if (kind == 5) v = rng() % 8 == 0;                  // mostly clear
                col[g][j] = v;
            }
        }
        if (check(col, nrows, k, chunk, rng)) return 1;
    }
    // crafted columns: per k and chunk size, gaps of k - 2, k - 1, k and k + 1 rows between two runs at every position; a single set
    // row at every position; the longest run at the start and at the end
    for (uint32_t chunk : chunks)
        for (uint32_t k : {1u, 2u, 3u, 5u, 21u, 32u}) {
            const uint32_t nrows = 3 * chunk + k + 3;
            std::vector<std::vector<uint8_t>> col;
            for (uint32_t gap = k >= 2 ? k - 2 : 0; gap <= k + 1; ++gap)
                for (uint32_t at = 1; at + gap + 1 <= nrows; ++at) {  // rows [at, at + gap) clear, all others set
                    std::vector<uint8_t> v(nrows, 1);
                    std::fill(v.begin() + at, v.begin() + at + gap, 0);
                    col.push_back(v);
                    if (at % 3 == 0) {  // two single set rows around the gap
                        std::vector<uint8_t> u(nrows, 0);
                        u[at - 1] = u[at + gap] = 1;
                        col.push_back(u);
                    }
                }
            for (uint32_t at = 0; at < nrows; ++at) {
                std::vector<uint8_t> v(nrows, 0);
                v[at] = 1;
                col.push_back(v);
            }
            for (uint32_t len = 1; len < nrows; len += 1 + len / 4) {
                std::vector<uint8_t> v(nrows, 0), u(nrows, 0);
                for (uint32_t j = 0; j < nrows; ++j) v[j] = j < len || (j > len && j % 2), u[nrows - 1 - j] = v[j];
                col.push_back(v);
                col.push_back(u);
            }
            if (check(col, nrows, k, chunk, rng)) return 1;
        }
    std::printf("ok: %llu cases, %llu windows of more than one chunk\n", (unsigned long long)cases, (unsigned long long)joined);
    return joined > 500 ? 0 : 1;
}
