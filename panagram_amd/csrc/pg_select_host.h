// pg_select_host.h — the host half of the column selection (k_rows_select*, pg_rows.hip): an ordered selection of source
// columns compiled into the few shift-and-mask steps the kernel runs per row.  Plain C++ without a GPU call, so that a
// stand-alone program can hold it to a loop over the bits under the host sanitizers (tools/select_segments_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace pg {

// One segment: a maximal run of consecutive source bits that go to consecutive destination bits, cut where the destination's
// 32-bit word ends.  It has at most 32 bits, so it reads source word sw and, where it runs past that word's end (two), sw + 1,
// and writes destination word dw:  dst[dw] |= (((src[sw + 1] : src[sw]) >> sh) & mask) << dsh.
struct SelSeg {
    uint32_t mask;    // the low `len` bits
    uint32_t words;   // sw | dw << 16
    uint32_t shifts;  // sh | dsh << 8 | two << 16
};
constexpr uint32_t SELECT_MAX_GENOMES = 32u << 16;  // (word numbers of 16 bits)

// destination bit j = source bit sel[j]; the segments come out in the order of their destination bits, so those of one
// destination word are neighbours.  (Dropping one column: two segments and the cuts at word ends; a full reversal: nsel.)
inline std::vector<SelSeg> select_segments(const uint32_t *sel, uint32_t nsel) {
    std::vector<SelSeg> out;
    for (uint32_t j = 0; j < nsel;) {
        uint32_t len = 1;
        while (j + len < nsel && (j + len) % 32 != 0 && sel[j + len] == sel[j] + len) ++len;
        const uint32_t sh = sel[j] % 32, two = sh + len > 32 ? 1u : 0u;
        out.push_back({len >= 32 ? 0xFFFFFFFFu : (1u << len) - 1u, (sel[j] / 32) | ((j / 32) << 16), sh | ((j % 32) << 8) | (two << 16)});
        j += len;
    }
    return out;
}

// bit d: some segment reads source word d (d < 32: the widths the kernel keeps a row's words in registers for)
inline uint32_t select_needed_words(const std::vector<SelSeg> &segs) {
    uint32_t need = 0;
    for (const SelSeg &g : segs) {
        const uint32_t sw = g.words & 0xFFFFu;
        if (sw < 32) need |= 1u << sw;
        if (((g.shifts >> 16) & 1u) && sw + 1 < 32) need |= 1u << (sw + 1);
    }
    return need;
}

}  // namespace pg
