// genotype_stitch_check.cpp — the host half of the allele kernels (panagram_amd/csrc/pg_genotype_host.h: allele_windows, allele_cut,
// allele_stitch) held to loops over single windows, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o genotype_stitch_check tools/genotype_stitch_check.cpp
//   ./genotype_stitch_check            (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
//   ./genotype_stitch_check CASES      (tests/test_genotype_cpu.py: one line "L k s l" per range in CASES; prints per range
//                                       "p0 p1 pieces windows inf seen depth", the sums of the partials below, for the numpy model)
// Every window of a range is marked by the definition — does it overlap bases [s, s + l), or hold both neighbours of the junction —
// and the pieces must cover exactly the marked windows, each once, in order, at most ALLELE_PIECE windows each.  The partial of
// piece j of range i is made up from (i, j, n) alone: windows = n, inf = (7 j + i) % (n + 1), seen = inf / 2, depth = 2^33 + j inf —
// sums over a long range need their 64 bits — and allele_stitch's sums, taken over the piece list in slices of 1, 3 and all pieces,
// must equal the sums of a plain loop.
#include "../panagram_amd/csrc/pg_genotype_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pg;

struct Range {
    uint64_t L, k, s, l;
};

static AllelePartial made_up(uint64_t i, uint64_t j, uint64_t n) {
    const uint64_t inf = (7 * j + i) % (n + 1), seen = inf / 2;
    return AllelePartial{n | inf << 16 | seen << 32, ((uint64_t)1 << 33) + j * inf};
}

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

// the sums of every range, by slices of `slice` pieces (0: all at once)
static void run(const std::vector<Range> &rs, uint64_t slice, std::vector<uint64_t> out[4], std::vector<uint64_t> &p0s,
                std::vector<uint64_t> &p1s, std::vector<uint64_t> &first) {
    std::vector<AllelePiece> pieces;
    std::vector<AllelePartial> partial;
    first.assign(rs.size() + 1, 0);
    p0s.resize(rs.size());
    p1s.resize(rs.size());
    for (size_t i = 0; i < rs.size(); ++i) {
        const Range &r = rs[i];
        uint64_t p0, p1;
        allele_windows(r.L, (uint32_t)r.k, r.s, r.l, &p0, &p1);
        p0s[i] = p0;
        p1s[i] = p1;
        // the definition, window by window
        const uint64_t nk = r.L >= r.k ? r.L - r.k + 1 : 0;
        std::vector<uint8_t> mark(nk, 0), got(nk, 0);
        for (uint64_t p = 0; p < nk; ++p)
            mark[p] = r.l ? (p < r.s + r.l && p + r.k > r.s) : (r.s >= 1 && p <= r.s - 1 && p + r.k > r.s);
        first[i] = pieces.size();
        allele_cut((uint32_t)i, p0, p1, pieces);
        CHECK(pieces.size() - first[i] == allele_piece_count(p1 - p0));
        uint64_t at = p0;
        for (size_t j = first[i]; j < pieces.size(); ++j) {
            const AllelePiece &pc = pieces[j];
            CHECK(pc.contig == i && pc.p0 == at && pc.n >= 1 && pc.n <= ALLELE_PIECE && pc.p0 + pc.n <= nk);
            CHECK(j + 1 == pieces.size() || pc.n == ALLELE_PIECE);
            for (uint64_t p = pc.p0; p < pc.p0 + pc.n; ++p) ++got[p];
            at += pc.n;
            partial.push_back(made_up(i, j - first[i], pc.n));
        }
        CHECK(at == p1);
        for (uint64_t p = 0; p < nk; ++p) CHECK(got[p] == mark[p]);
    }
    first[rs.size()] = pieces.size();
    for (int f = 0; f < 4; ++f) out[f].assign(rs.size(), 0);
    const uint64_t per = slice ? slice : (pieces.empty() ? 1 : pieces.size());
    for (uint64_t c0 = 0; c0 < pieces.size(); c0 += per) {
        const uint64_t m = pieces.size() - c0 < per ? pieces.size() - c0 : per;
        allele_stitch(rs.size(), first.data(), partial.data() + c0, c0, m, out[0].data(), out[1].data(), out[2].data(), out[3].data());
    }
    // a plain loop
    for (size_t i = 0; i < rs.size(); ++i) {
        uint64_t w = 0, inf = 0, seen = 0, depth = 0;
        for (uint64_t j = 0; j < first[i + 1] - first[i]; ++j) {
            const uint64_t n = j + 1 == first[i + 1] - first[i] ? (p1s[i] - p0s[i]) - j * ALLELE_PIECE : ALLELE_PIECE;
            const AllelePartial p = made_up(i, j, n);
            w += n;
            inf += (p.counts >> 16) & 0xFFFF;
            seen += p.counts >> 32;
            depth += p.depth;
        }
        CHECK(w == out[0][i] && inf == out[1][i] && seen == out[2][i] && depth == out[3][i] && w == p1s[i] - p0s[i]);
    }
}

int main(int argc, char **argv) {
    std::vector<Range> rs;
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "r");
        CHECK(f);
        Range r;
        while (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &r.L, &r.k, &r.s, &r.l) == 4) rs.push_back(r);
        std::fclose(f);
    } else {
        for (uint64_t k : {1, 2, 6, 21, 32})
            for (uint64_t L : {0, 1, 5, 20, 21, 31, 32, 33, 63, 64, 65, 100, 300})
                for (uint64_t s = 0; s <= L; ++s)
                    for (uint64_t l : {0, 1, 2, 20, 63, 64, 65, 130, 300})
                        if (s + l <= L) rs.push_back(Range{L, k, s, l});
        rs.push_back(Range{70000, 21, 0, 70000});   // 1 094 pieces: the depth needs 64 bits
        rs.push_back(Range{70000, 21, 100, 65536});  // 1 025 pieces
    }
    std::vector<uint64_t> out[4], alt[4], p0, p1, first;
    run(rs, 0, out, p0, p1, first);
    for (uint64_t slice : {1, 3}) {
        if (argc > 1 || rs.size() > 3000) {  // (slices of one piece over the whole built-in list would take minutes)
            std::vector<Range> some(rs.end() - (rs.size() < 300 ? rs.size() : 300), rs.end());
            std::vector<uint64_t> whole[4], q0, q1, qf;
            run(some, 0, whole, q0, q1, qf);
            run(some, slice, alt, q0, q1, qf);
            for (int f = 0; f < 4; ++f) CHECK(alt[f] == whole[f]);
        } else {
            std::vector<uint64_t> q0, q1, qf;
            run(rs, slice, alt, q0, q1, qf);
            for (int f = 0; f < 4; ++f) CHECK(alt[f] == out[f]);
        }
    }
    if (argc > 1)
        for (size_t i = 0; i < rs.size(); ++i)
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p0[i], p1[i],
                        first[i + 1] - first[i], out[0][i], out[1][i], out[2][i], out[3][i]);
    else
        std::printf("ok: %zu ranges, %" PRIu64 " pieces\n", rs.size(), first[rs.size()]);
    return 0;
}
