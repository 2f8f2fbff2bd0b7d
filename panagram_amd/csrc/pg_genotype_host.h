// pg_genotype_host.h — the host half of the allele kernels (pg_genotype.hip; the definitions are there): the window interval of an
// allele range, its cut into pieces of at most ALLELE_PIECE windows — one wave's work — and the sum of a range's piece partials.
// Plain C++ without a GPU call, as pg_copies_host.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pg {

constexpr uint32_t ALLELE_PIECE = 64;  // windows per piece: one per lane of a wave

// windows [p0, p0 + n) of contig `contig`, 1 <= n <= ALLELE_PIECE, all below the contig's len - k + 1
struct AllelePiece {
    uint32_t contig, n;
    uint64_t p0;
};
// what k_allele_support leaves per piece: counts = windows | inf << 16 | seen << 32 (each at most ALLELE_PIECE), depth = the sum of
// the sample's counters over the informative windows
struct AllelePartial {
    uint64_t counts, depth;
};

// the allele windows of bases [s, s + l) of a contig of len bases, s + l <= len: positions [*p0, *p1), p0 == p1 when there is none
inline void allele_windows(uint64_t len, uint32_t k, uint64_t s, uint64_t l, uint64_t *p0, uint64_t *p1) {
    const uint64_t nk = len >= k ? len - k + 1 : 0;
    const uint64_t lo = s + 1 > k ? s + 1 - k : 0, hi = s + l < nk ? s + l : nk;
    *p0 = lo;
    *p1 = hi > lo ? hi : lo;
}

// how many pieces a range of nwin windows takes
inline uint64_t allele_piece_count(uint64_t nwin) { return (nwin + ALLELE_PIECE - 1) / ALLELE_PIECE; }

// the pieces of windows [p0, p1) of `contig` appended to `out`, in position order
inline void allele_cut(uint32_t contig, uint64_t p0, uint64_t p1, std::vector<AllelePiece> &out) {
    for (uint64_t p = p0; p < p1; p += ALLELE_PIECE) {
        const uint64_t n = p1 - p < ALLELE_PIECE ? p1 - p : ALLELE_PIECE;
        out.push_back(AllelePiece{contig, (uint32_t)n, p});
    }
}

// Range i's pieces are [first[i], first[i + 1]) of partial[]; the sums are taken in 64 bits and ADDED to the four outputs of range
// i (a caller that launches the piece list in slices passes each slice's pieces: `base` = the number of the first piece of
// partial[], pieces outside [base, base + count) are skipped).
inline void allele_stitch(uint64_t nranges, const uint64_t *first, const AllelePartial *partial, uint64_t base, uint64_t count,
                          uint64_t *windows, uint64_t *inf, uint64_t *seen, uint64_t *depth) {
    for (uint64_t i = 0; i < nranges; ++i) {
        const uint64_t a = first[i] > base ? first[i] : base, b = first[i + 1] < base + count ? first[i + 1] : base + count;
        for (uint64_t c = a; c < b; ++c) {
            const AllelePartial &p = partial[c - base];
            windows[i] += p.counts & 0xFFFFu;
            inf[i] += (p.counts >> 16) & 0xFFFFu;
            seen[i] += (p.counts >> 32) & 0xFFFFu;
            depth[i] += p.depth;
        }
    }
}

}  // namespace pg
