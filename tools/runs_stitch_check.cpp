// runs_stitch_check.cpp — the host scan between the two passes of the run kernels (panagram_amd/csrc/pg_runs_host.h: runs_stitch)
// held to a brute-force loop, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o runs_stitch_check tools/runs_stitch_check.cpp
//   ./runs_stitch_check        (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
// Seeded groups of marked / unmarked positions — groups of no position (no chunk), of one chunk, of many — are cut into chunks of a
// few positions.  What a count pass leaves per chunk {tally a, starts, ends, tally b} is computed by a loop with one halo position;
// runs_stitch's offsets then drive a loop that writes what an emit pass writes, chunk by chunk in any order, and the runs that
// come out must equal those of one loop over the whole group.  Crafted beside them: a run that starts in one chunk and ends three
// chunks later, and a group whose starts and ends differ, which must come back as ~0 with the group's number.
#include "../panagram_amd/csrc/pg_runs_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

using namespace pg;

struct Count4 {
    uint32_t x, y, z, w;  // tally a, starts, ends, tally b
};
struct Offs2 {
    uint64_t x, y;
};
struct Run {
    uint32_t group;
    uint64_t start, end;
    bool operator==(const Run &o) const { return group == o.group && start == o.start && end == o.end; }
};
struct Group {
    std::vector<uint8_t> marked, other;  // per position: in a run; counted by tally b
};

// chunk [c0, ce) of a group as a run kernel walks it.  offs == nullptr: the count pass; otherwise the emit pass into starts / ends
static Count4 chunk_pass(const Group &g, uint64_t c0, uint64_t ce, const Offs2 *offs, std::vector<uint64_t> &starts, std::vector<uint64_t> &ends) {
    Count4 c{0, 0, 0, 0};
    uint8_t prev = c0 > 0 ? g.marked[c0 - 1] : 0;  // (the halo)
    const auto put = [&](std::vector<uint64_t> &dst, uint64_t at, uint64_t v) {
        if (at >= dst.size()) std::abort();  // (an offset past the runs: the stitch counted wrong)
        dst[at] = v;
    };
    for (uint64_t j = c0; j < ce; ++j) {
        const uint8_t cur = g.marked[j];
        if (cur && !prev) {
            if (offs) put(starts, offs->x + c.y, j);
            c.y += 1;
        }
        if (prev && !cur) {
            if (offs) put(ends, offs->y + c.z, j);
            c.z += 1;
        }
        c.x += cur;
        c.w += g.other[j];
        prev = cur;
    }
    if (ce == g.marked.size() && prev) {  // a run that reaches the group's end is closed there
        if (offs) put(ends, offs->y + c.z, ce);
        c.z += 1;
    }
    return c;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct Piece {
    uint32_t group;
    uint64_t c0, ce;
};

// the groups cut into chunks of `chunk` positions, both passes with the stitch between them, against one loop per group
static int check(const std::vector<Group> &groups, uint64_t chunk, std::mt19937_64 &rng, uint64_t *across) {
    const uint32_t ngroups = (uint32_t)groups.size();
    std::vector<uint64_t> first(ngroups + 1, 0), none;
    std::vector<Piece> pieces;
    std::vector<Count4> counts;
    for (uint32_t g = 0; g < ngroups; ++g) {
        first[g] = pieces.size();
        for (uint64_t c0 = 0; c0 < groups[g].marked.size(); c0 += chunk) {
            pieces.push_back(Piece{g, c0, std::min<uint64_t>(c0 + chunk, groups[g].marked.size())});
            counts.push_back(chunk_pass(groups[g], c0, pieces.back().ce, nullptr, none, none));
        }
    }
    first[ngroups] = pieces.size();
    std::vector<Offs2> offs(pieces.size());
    std::vector<uint64_t> nruns(ngroups, ~0ull), tally(ngroups, ~0ull);
    uint64_t sums[2] = {~0ull, ~0ull}, bad[3] = {0, 0, 0};
    const uint64_t total = runs_stitch(ngroups, first.data(), counts.data(), offs.data(), nruns.data(), tally.data(), sums, bad);
    CHECK(total != ~0ull);
    // the emit pass, the chunks in any order
    std::vector<uint64_t> starts(total, ~0ull), ends(total, ~0ull);
    std::vector<size_t> order(pieces.size());
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);
    for (size_t i : order) chunk_pass(groups[pieces[i].group], pieces[i].c0, pieces[i].ce, &offs[i], starts, ends);
    // one loop over every group
    std::vector<Run> want;
    uint64_t want_a = 0, want_b = 0;
    for (uint32_t g = 0; g < ngroups; ++g) {
        const size_t before = want.size();
        const std::vector<uint8_t> &m = groups[g].marked;
        uint64_t a = 0;
        for (uint64_t j = 0; j < m.size(); ++j) {
            if (m[j] && (j == 0 || !m[j - 1])) want.push_back(Run{g, j, 0});
            if (m[j] && (j + 1 == m.size() || !m[j + 1])) want.back().end = j + 1;
            a += m[j];
            want_b += groups[g].other[j];
        }
        CHECK(nruns[g] == want.size() - before);
        CHECK(tally[g] == a);
        want_a += a;
    }
    CHECK(total == want.size());
    CHECK(sums[0] == want_a && sums[1] == want_b);
    uint64_t at = 0;
    for (uint32_t g = 0; g < ngroups; ++g)
        for (uint64_t i = 0; i < nruns[g]; ++i, ++at) {
            CHECK((Run{g, starts[at], ends[at]}) == want[at]);
            *across += ends[at] / chunk >= starts[at] / chunk + 3;
        }
    return 0;
}

int main() {
    std::mt19937_64 rng(7);
    uint64_t cases = 0, across = 0, empty_groups = 0;
    // crafted: chunks of 4 positions; group 0 has no position, group 1 a run over positions [2, 15) — it starts in chunk 0 and ends
    // three chunks later, in chunk 3 — and one that reaches the group's end; group 2 has no position either
    {
        std::vector<Group> groups(3);
        groups[1].marked.assign(22, 0);
        groups[1].other.assign(22, 1);
        for (uint64_t j = 2; j < 15; ++j) groups[1].marked[j] = 1;
        groups[1].marked[20] = groups[1].marked[21] = 1;
        uint64_t far = 0;
        if (check(groups, 4, rng, &far)) return 1;
        CHECK(far == 1);
        ++cases;
    }
    // crafted: a group whose starts and ends differ (counts that no kernel leaves) is named, whatever stands behind it
    {
        const std::vector<uint64_t> first = {0, 2, 2, 4, 5};
        const std::vector<Count4> counts = {{3, 1, 0, 0}, {2, 0, 1, 0}, {4, 2, 1, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}};
        std::vector<Offs2> offs(counts.size());
        std::vector<uint64_t> nruns(4, 0);
        uint64_t sums[2] = {0, 0}, bad[3] = {~0ull, 0, 0};
        CHECK(runs_stitch(4, first.data(), counts.data(), offs.data(), nruns.data(), nullptr, sums, bad) == ~0ull);
        CHECK(bad[0] == 2 && bad[1] == 3 && bad[2] == 2);
        CHECK(nruns[0] == 1 && nruns[1] == 0);
        ++cases;
    }
    for (uint32_t round = 0; round < 400; ++round) {
        const uint32_t ngroups = 1 + rng() % 6;
        const uint64_t chunk = 1 + rng() % 9;
        std::vector<Group> groups(ngroups);
        for (Group &g : groups) {
            const uint64_t n = rng() % 4 == 0 ? 0 : rng() % 150;
            empty_groups += n == 0;
            const uint32_t keep = 1 + rng() % 12;  // (long runs and short ones)
            uint8_t cur = rng() & 1;
            for (uint64_t j = 0; j < n; ++j) {
                if (rng() % keep == 0) cur ^= 1;
                g.marked.push_back(cur);
                g.other.push_back(rng() & 1);
            }
        }
        if (check(groups, chunk, rng, &across)) return 1;
        ++cases;
    }
    std::printf("ok: %llu cases, %llu runs ending three chunks or more behind their start, %llu groups without a chunk\n",
                (unsigned long long)cases, (unsigned long long)across, (unsigned long long)empty_groups);
    return across > 200 && empty_groups > 100 ? 0 : 1;
}
