// select_segments_check.cpp — the host half of the column selection (panagram_amd/csrc/pg_select_host.h: select_segments,
// select_needed_words) held to a loop over the bits, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o select_segments_check tools/select_segments_check.cpp
//   ./select_segments_check    (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
// Random rows of 1..200 genomes and random ordered selections of them — columns dropped, kept runs, permutations — go through the
// segments the way k_rows_select applies them (two neighbouring 32-bit source words shifted, masked and ORed into one destination
// word); the result must equal a loop that moves one bit at a time, every segment must stay inside one destination word and
// two source words, and no segment may read a word select_needed_words does not name.
#include "../panagram_amd/csrc/pg_select_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

using namespace pg;

static void fail(const char *what, uint32_t n_old, uint32_t n_new) {
    std::fprintf(stderr, "MISMATCH: %s (%u -> %u genomes)\n", what, n_old, n_new);
    std::exit(1);
}

int main() {
    std::mt19937 rng(12345);
    unsigned cases = 0, nsegs = 0;
    for (uint32_t n_old = 1; n_old <= 200; ++n_old)
        for (int kind = 0; kind < 6; ++kind) {
            std::vector<uint32_t> all(n_old), sel;
            std::iota(all.begin(), all.end(), 0u);
            if (kind == 0) {  // one column dropped
                const uint32_t d = rng() % n_old;
                for (uint32_t g : all)
                    if (g != d || n_old == 1) sel.push_back(g);
            } else if (kind == 1) {  // random columns dropped, order kept
                for (uint32_t g : all)
                    if (rng() % 4) sel.push_back(g);
                if (sel.empty()) sel.push_back(n_old - 1);
            } else if (kind == 2) {  // reversal
                sel.assign(all.rbegin(), all.rend());
            } else if (kind == 3) {  // the identity
                sel = all;
            } else {  // a shuffle, cut short
                std::shuffle(all.begin(), all.end(), rng);
                sel.assign(all.begin(), all.begin() + 1 + rng() % n_old);
            }
            const uint32_t n_new = (uint32_t)sel.size(), ws = (n_old + 31) / 32, wd = (n_new + 31) / 32;
            const std::vector<SelSeg> segs = select_segments(sel.data(), n_new);
            const uint32_t need = select_needed_words(segs);
            std::vector<uint32_t> src(ws + 1), want(wd, 0u), got(wd, 0u);
            for (uint32_t &w : src) w = (uint32_t)rng();  // (stale bits past n_old included; src[ws] is what lies behind the row)
            for (uint32_t j = 0; j < n_new; ++j) want[j / 32] |= ((src[sel[j] / 32] >> (sel[j] % 32)) & 1u) << (j % 32);
            uint32_t covered = 0, last_dw = 0;
            for (const SelSeg &g : segs) {
                const uint32_t sw = g.words & 0xFFFFu, dw = g.words >> 16, sh = g.shifts & 0xFFu, dsh = (g.shifts >> 8) & 0xFFu, two = (g.shifts >> 16) & 1u;
                const uint32_t len = (uint32_t)__builtin_popcount(g.mask);
                if (g.mask != (len >= 32 ? 0xFFFFFFFFu : (1u << len) - 1u) || len == 0) fail("a mask that is no run of low bits", n_old, n_new);
                if (dsh + len > 32 || dw >= wd || dw < last_dw) fail("a segment leaves its destination word, or the order", n_old, n_new);
                if (two != (sh + len > 32 ? 1u : 0u) || sw + two >= ws) fail("a segment reads past the source row's words", n_old, n_new);
                if (sw < 32 && !((need >> sw) & 1u)) fail("a word read that is not named", n_old, n_new);
                if (two && sw + 1 < 32 && !((need >> (sw + 1)) & 1u)) fail("a second word read that is not named", n_old, n_new);
                const uint32_t lo = src[sw], hi = two ? src[sw + 1] : 0u;
                got[dw] |= ((uint32_t)((((unsigned long long)hi << 32) | lo) >> sh) & g.mask) << dsh;
                covered += len;
                last_dw = dw;
            }
            if (covered != n_new) fail("the segments do not cover the destination's bits once", n_old, n_new);
            if (got != want) fail("the segments' result differs from the bit loop", n_old, n_new);
            ++cases;
            nsegs += (unsigned)segs.size();
        }
    // the counts the kernel's header promises
    {
        std::vector<uint32_t> sel;
        for (uint32_t g = 0; g < 9; ++g)
            if (g != 4) sel.push_back(g);
        if (select_segments(sel.data(), 8).size() != 2) fail("dropping one of nine columns: two segments", 9, 8);
        std::vector<uint32_t> rev(16);
        for (uint32_t j = 0; j < 16; ++j) rev[j] = 15 - j;
        if (select_segments(rev.data(), 16).size() != 16) fail("a full reversal: one segment per column", 16, 16);
    }
    std::printf("ok: %u selections, %u segments\n", cases, nsegs);
    return 0;
}
