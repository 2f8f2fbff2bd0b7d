// planes_check.cpp — the integer part of the column sums' counter planes (panagram_amd/csrc/pg_planes.h: add4, settle, the
// transposition into byte counters) held to a plain count, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o planes_check tools/planes_check.cpp
//   ./planes_check        (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
// One word.  Rows go in in blocks of four, odd4 / odd8 derived from the running count as the kernels derive them; after 4, 8, ...,
// 252 rows a COPY of the planes is settled and transposed and all 32 column counts are compared with a plain count (so every
// state of the held-back carries is flushed once), and the planes themselves after the last block.  Pseudo-random rows of several
// densities; all-ones rows, which take every plane to its ceiling at 252; and the same again on the planes a flush has left
// behind, which must start clean.
#include "../panagram_amd/csrc/pg_planes.h"

#include <cstdio>
#include <random>

using namespace pg;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// one word's storage, as the kernels declare it (there: three arrays over the words)
struct Store {
    uint32_t p[8], pf, pe;
    Planes view() { return Planes(p, pf, pe); }
};

// what a flush does to the planes, but for the exchange or the LDS adds: settle, transpose, zero
static void flush(Store &S, uint32_t rows, uint32_t got[32]) {
    Planes P = S.view();
    P.settle(Planes::odd4(rows), Planes::odd8(rows));
    for (int q = 0; q < 8; ++q) {
        const uint32_t v = P.bytes(q);
        for (int b = 0; b < 4; ++b) got[8 * b + q] = (v >> (8 * b)) & 255u;  // byte b counts bit 8 b + q
    }
    P.zero_planes();
}

// `blocks` blocks of four rows from next() into P (which must be clean), checked after every block
template <class F>
static int feed(Store &S, uint32_t blocks, F &&next, uint64_t &checks) {
    Planes P = S.view();
    uint32_t want[32] = {0}, rows = 0;
    for (uint32_t blk = 0; blk < blocks; ++blk) {
        uint32_t r[4];
        for (int j = 0; j < 4; ++j) {
            r[j] = next();
            for (int g = 0; g < 32; ++g) want[g] += (r[j] >> g) & 1u;
        }
        P.add4(r[0], r[1], r[2], r[3], Planes::odd4(rows), Planes::odd8(rows));
        rows += 4;
        CHECK(rows <= PLANES_CEIL);
        Store copy = S;
        uint32_t got[32];
        flush(copy, rows, got);
        for (int g = 0; g < 32; ++g) CHECK(got[g] == want[g]);
        ++checks;
    }
    uint32_t got[32];
    flush(S, rows, got);  // ... and the planes themselves: the next feed starts from what this leaves
    for (int g = 0; g < 32; ++g) CHECK(got[g] == want[g]);
    for (int q = 0; q < 8; ++q) CHECK(S.p[q] == 0);
    return 0;
}

int main() {
    static_assert(PLANES_FLUSH % 16 == 0 && PLANES_FLUSH + 15 <= PLANES_CEIL, "a flush between whole 16-row blocks, one more block fits");
    std::mt19937 rng(11);
    uint64_t checks = 0, feeds = 0;
    Store P;
    P.view().clear();
    const uint32_t blocks = 252 / 4;  // the most four-row blocks eight planes hold
    for (uint32_t round = 0; round < 40; ++round) {
        // (after the first round every feed runs on planes that a flush has left behind, held-back carries and all)
        const uint32_t dens = round % 4;  // all bits at random; sparse; dense; one column always set
        auto rnd = [&]() -> uint32_t {
            const uint32_t a = rng(), b = rng();
            return dens == 0 ? a : dens == 1 ? (a & b) : dens == 2 ? (a | b) : (a | 0x80000001u);
        };
        if (feed(P, round % 5 == 4 ? 1 + rng() % blocks : blocks, rnd, checks)) return 1;
        ++feeds;
        if (round % 8 == 3) {  // all-ones rows: every column counts 4, 8, ..., 252
            if (feed(P, blocks, []() -> uint32_t { return 0xFFFFFFFFu; }, checks)) return 1;
            ++feeds;
        }
    }
    {  // the kernels' threshold: PLANES_FLUSH rows of all ones on fresh planes, no carry held back at the flush
        Store Q;
        Q.view().clear();
        if (feed(Q, PLANES_FLUSH / 4, []() -> uint32_t { return 0xFFFFFFFFu; }, checks)) return 1;
        CHECK(!Planes::odd4(PLANES_FLUSH) && !Planes::odd8(PLANES_FLUSH));
        ++feeds;
    }
    std::printf("ok: %llu feeds, %llu flushes compared with a plain count\n", (unsigned long long)feeds, (unsigned long long)checks);
    return checks > 2000 ? 0 : 1;
}
