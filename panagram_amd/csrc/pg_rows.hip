// pg_rows.hip — everything that reads FINISHED bitmap.1 rows on gfx950 (CDNA4, wave64): the statistics pass and its side paths.
//
// Replaces (reference, kjenike/panagram): the popcount / 1-in-100 / histogram part of KMCdb::write_bits' scatter loop
// (cpp/anchor.cpp:156-189), Genome.bin_bitsum and the column sums of the anchoring loop (index.py:1048-1051,1169-1183), its
// gene windows (index.py:1055-1063) and the lowres_step rows (index.py:101-106).  The genome-sharded exchange has no
// counterpart there.
//
//   k_epilogue_* streaming statistics from the finished bitmap.1 rows: bitmap.100 (1-in-100
//                rows), per-bin popcount histogram, per-contig column sums — persistent
//                workgroups, register accumulators.  They share the histogram window (HistWindow), the prologue
//                (epi_prologue) and, but for one-byte rows, the column sums' counter planes (pg_planes.h).
//   k_epilogue_b1  one-byte rows (up to 8 genomes): 32 rows per thread over 8 full tiles, bit-sliced.
//   k_epilogue_n   rows of 2..8 bytes, one instantiation per width: 16 consecutive rows per thread over 4 full tiles.
//   k_epilogue_w   rows of 9..16 bytes (65..128 genomes): three or four words per row.
//   k_epilogue_chunks  rows wider than 16 bytes (more than 128 genomes): a lane owns one
//                16-byte chunk of the rows it visits, one launch reads every row once.
//   k_window_stats, k_cols_extract / k_cols_merge: side paths (gene / bin windows; the
//                genome-sharded exchange).
//   k_rows_append*  finished rows of N genomes + column blocks of m more -> rows of N + m genomes in one pass (`add`).
//   k_rows_select*  finished rows of N genomes -> rows of an ordered selection of their columns in one pass (`subset`).
//   k_lowres, k_tile_reduce: the low-resolution bitmap for steps other than 100; the per-tile counters of a fused k_probe launch
//                (FuseArgs, pg_kernels.h) into the bins and column sums.
#include "pg_kernels.h"
#include "pg_planes.h"
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <type_traits>

#include <algorithm>

namespace pg {

// ---------------------------------------------------------------------------
// statistics from finished rows: bitmap.100, per-bin popcount histogram, column sums.
// A workgroup (256 threads) walks a CONTIGUOUS range of tiles (PT consecutive positions per
// thread and tile); histogram counters stay in LDS until the bin changes and column sums until
// the end, so that global atomics on the few shared counters stay rare.
// (also the second half of the genome-sharded mode: rows combined over xGMI first)
// ---------------------------------------------------------------------------
// A workgroup keeps the histograms of EPI_MAXB consecutive bins in LDS at a time (rows relative to
// cur_row0): contigs of a few kb .. Mb have bins of nkmers/100 positions, far shorter than a tile.
// The window is 16..128 bins wide, as many as about 12 KB of LDS hold at N + 1 counters per bin (chosen by the launcher,
// handed over in bits 8..15 of `flags`): with 16 bins a contig of a few kb — bins of 50 rows, a tile spans 11 of them —
// flushed its window to global memory after nearly every tile (4 x 100 Mb in 20 000 contigs: 1.45 ms for 4 x 10^8 rows).
constexpr uint32_t EPI_MAXB = 16;  // (the least)
__host__ __device__ __forceinline__ uint32_t epi_maxb_for(uint32_t ngenomes) {
    const uint32_t b = 3072u / (ngenomes + 1u);
    return b < EPI_MAXB ? EPI_MAXB : (b > 128u ? 128u : b);
}
__host__ __device__ __forceinline__ uint32_t epi_minbin(uint32_t maxb) { return ((uint32_t)PROBE_TILE + maxb - 3u) / (maxb - 2u); }  // a tile then spans <= maxb bins
// column sums: one ballot + popcount per genome bit, accumulated in LDS by lane 0
__device__ __forceinline__ void colsum_word(uint32_t wv, uint32_t d, uint32_t N, uint32_t *cs, int lane) {
    const uint32_t ng = min(32u, N - 32 * d);
    for (uint32_t bit = 0; bit < ng; ++bit) {
        const unsigned long long bal = __ballot((wv >> bit) & 1u);
        if (lane == 0 && bal) atomicAdd(&cs[32 * d + bit], (uint32_t)__popcll(bal));
    }
}
// wave-aggregated histogram of (bin, popcount): LDS for the first EPI_MAXB bins from bin0, global beyond
__device__ __forceinline__ void hist_position(bool active, uint32_t pos, uint32_t popc, uint32_t N, uint32_t binlen,
                                              uint32_t bin0, uint32_t bin0_start, uint32_t rel_base, uint32_t *hist,
                                              uint32_t *bins, uint64_t bin_off, int lane, uint32_t maxb) {
    if (popc > N) popc = N;  // junk bits beyond ngenomes: the reference indexes out of bounds here
    const uint32_t dpos = pos - bin0_start;
    const uint32_t rel = (binlen >= (uint32_t)PROBE_TILE) ? (dpos >= binlen ? 1u : 0u) : dpos / binlen;
    const uint32_t hk = rel * (N + 1) + popc;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lk = __shfl(hk, leader);
        const unsigned long long mk = __ballot(active && hk == lk) & todo;
        if (lane == leader) {
            const uint32_t cnt = (uint32_t)__popcll(mk);
            if (rel_base + rel < maxb) atomicAdd(&hist[rel_base * (N + 1) + hk], cnt);
            else atomicAdd(&bins[(bin_off + bin0 + rel) * (uint64_t)(N + 1) + popc], cnt);
        }
        todo &= ~mk;
    }
}

// Every lane adds its own value to the LDS counter p (one ds_add per lane).  With an address the compiler sees as uniform,
// its atomic optimizer sums the lanes first in a SCALAR loop over the active lanes (s_ff1 / v_readlane / s_add ..., seven
// scalar instructions per lane and a dependent chain through all 64): k_epilogue_b1's end-of-bin and end-of-range
// reductions (9 + 8 counters) came to most of the pass's SQ_INSTS_SALU, and their chains were most of its fixed cost
// (profiles/r7_stats_fixed_cost.md).  The zero comes out of inline assembly, so that the address stays per lane; the LDS
// works the same-address lanes off one after the other, about 64 cycles per instruction.
__device__ __forceinline__ void lds_add_lanes(uint32_t *p, uint32_t v) {
    uint32_t z;
    asm("v_mov_b32 %0, 0" : "=v"(z));
    atomicAdd(p + z, v);
}

// four consecutive rows of NB bytes = NB aligned 32-bit words (a thread's first row starts at a
// multiple of 4 rows): load the words (all in flight together), cut the rows out with static shifts
template <int NB>
__device__ __forceinline__ void load_row_words(const uint8_t *g4, uint32_t raw[8]) {
#pragma unroll
    for (int i = 0; i < NB; ++i) raw[i] = reinterpret_cast<const uint32_t *>(g4)[i];
}
template <int NB>
__device__ __forceinline__ void cut4_rows(const uint32_t raw[8], uint32_t w0[4], uint32_t w1[4]) {
    uint32_t w[NB + 1];
#pragma unroll
    for (int i = 0; i < NB; ++i) w[i] = raw[i];
    w[NB] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        constexpr uint64_t keep = NB >= 8 ? ~0ull : ((1ull << (8 * (NB & 7))) - 1);
        const int off = j * NB, idx = off >> 2, sh = 8 * (off & 3);
        uint64_t v = (uint64_t)w[idx] >> sh;
        if (idx + 1 <= NB) v |= (uint64_t)w[idx + 1] << (32 - sh);
        if (sh && idx + 2 <= NB) v |= (uint64_t)w[idx + 2] << (64 - sh);
        v &= keep;
        w0[j] = (uint32_t)v;
        w1[j] = (uint32_t)(v >> 32);
    }
}
#ifndef PG_EPI_MIN_TILES
#define PG_EPI_MIN_TILES 128
#endif
constexpr int EPI_THREADS = PROBE_TILE / 4;

static_assert(EPI_THREADS >= 64 && EPI_THREADS % 64 == 0, "PROBE_TILE must be a multiple of 256");

struct __attribute__((packed)) U32 { uint32_t v; };             // (unaligned 4- and 16-byte accesses)
struct __attribute__((packed)) U128 { uint32_t x, y, z, w; };

__device__ __forceinline__ void flush_hist(uint32_t N, uint32_t *hist, uint32_t *bins, uint64_t bin_row0, int tid, uint32_t maxb) {
    for (uint32_t i = tid; i < maxb * (N + 1); i += EPI_THREADS) {
        const uint32_t hv = hist[i];
        if (hv) {
            const uint32_t rel = i / (N + 1), pc2 = i - rel * (N + 1);
            atomicAdd(&bins[(bin_row0 + rel) * (uint64_t)(N + 1) + pc2], hv);
            hist[i] = 0;
        }
    }
}

// The histogram window of a workgroup: the LDS counters `hist` stand for the MAXB bins rows from cur_row0 on (~0: none yet).
// All of its state is block-uniform; every member is called by the whole workgroup.
//
// The group paths of rows of 2..16 bytes add ONE to an LDS counter per row, and the lanes of a wave mostly ask for the
// same few counters (the popcount classes near N): the LDS works a wave's atomic off one lane per cycle and address —
// 0.9-1.0 ps per row whatever the row width, twice what 2-byte rows need otherwise.  While the groups lie inside one
// or two long bins (any contig of more than 200 kb) the window is therefore used as EPI_REPL copies of those two bin
// rows, lane l adding to copy l % EPI_REPL (copy c at c * repl_stride, an odd stride: the copies of one class sit in
// different banks); `unreplicate` folds the copies into the window's ordinary form — rows 0 and 1 — before anything
// else reads or flushes it.  (The chunk kernel keeps the plain window: the copies lose 3-6 % where only every second or third
// lane adds, profiles/r4e_ab_stats_hist_copies_wide.txt.)
constexpr uint32_t EPI_REPL = 8;  // (16 copies: no further gain, profiles/r3_ab_stats_hist_copies.txt)
struct HistWindow {
    uint32_t *hist, *bins;
    uint32_t N, MAXB, MINBIN;  // MINBIN: bins at least this long let a tile span <= MAXB of them
    int tid;
    uint64_t cur_row0;  // bins row the counters currently stand for
    bool repl;          // the window holds copies
    __device__ __forceinline__ uint32_t repl_stride() const { return (2u * (N + 1u)) | 1u; }
    // the copies must fit the window: the last one would run into the column counters behind it otherwise (8 copies need
    // 16 (N + 1) + 8 words: MAXB >= 17 — epi_maxb_for gives >= 23 for N <= 128)
    __device__ __forceinline__ bool copies_fit() const { return EPI_REPL * repl_stride() <= MAXB * (N + 1u); }
    __device__ __forceinline__ void flush() {
        __syncthreads();
        flush_hist(N, hist, bins, cur_row0, tid, MAXB);
        __syncthreads();
    }
    __device__ __forceinline__ void unreplicate() {
        if (!repl) return;
        __syncthreads();
        for (uint32_t i = tid; i < 2u * (N + 1u); i += EPI_THREADS) {
            uint32_t v = hist[i];
#pragma unroll
            for (uint32_t cpy = 1; cpy < EPI_REPL; ++cpy) {
                v += hist[cpy * repl_stride() + i];
                hist[cpy * repl_stride() + i] = 0;
            }
            hist[i] = v;
        }
        __syncthreads();
        repl = false;
    }
    // Seat the bins rows row0 .. row0 + last_rel (a tile's, or a one-byte group's) in the window in its ordinary form: may
    // they add to it as it stands?  If not it is flushed and moved to row0.  exact: the caller's per-thread accumulators stand
    // for the window's FIRST row, so row0 must be it; an unwindowed tile (bins shorter than MINBIN) likewise uses row 0 only.
    // before_flush: what the caller has to put into the window first (the one-byte kernel's register accumulators).
    // Returns row0's place in the window.
    template <class F>
    __device__ __forceinline__ uint32_t seat_tile(uint64_t row0, uint32_t last_rel, bool windowed, bool exact, F &&before_flush) {
        const bool fits = cur_row0 != ~0ull && (exact || !windowed ? row0 == cur_row0
                                                : (row0 >= cur_row0 && row0 + last_rel < cur_row0 + MAXB));
        if (!fits) {
            if (cur_row0 != ~0ull) {
                before_flush();
                flush();
            }
            cur_row0 = row0;
        }
        return (uint32_t)(row0 - cur_row0);
    }
    __device__ __forceinline__ uint32_t seat_tile(uint64_t row0, uint32_t last_rel, bool windowed) {
        return seat_tile(row0, last_rel, windowed, false, [] {});
    }
    // Seat the nbg bins rows of a group of rows of 2..16 bytes: as copies while the group lies inside one or two bins.
    // Returns whether the window holds copies now.
    __device__ __forceinline__ bool seat_group(uint64_t row0g, uint32_t nbg) {
        const bool want_repl = nbg <= 2u && copies_fit();
        if (want_repl) {
            if (!(repl && row0g >= cur_row0 && row0g + nbg <= cur_row0 + 2u)) {
                if (cur_row0 != ~0ull) {
                    unreplicate();
                    flush();
                }
                cur_row0 = row0g;
                repl = true;
            }
        } else {
            unreplicate();
            if (cur_row0 == ~0ull || row0g < cur_row0 || row0g + nbg > cur_row0 + MAXB) {
                if (cur_row0 != ~0ull) flush();
                cur_row0 = row0g;
            }
        }
        return want_repl;
    }
    // the counters of bins row row0g + rel0 after seat_group: the lane's copy of them, or the only one
    __device__ __forceinline__ uint32_t *group_row(uint64_t row0g, uint32_t rel0, bool copies, int lane) const {
        return hist + ((uint32_t)(row0g - cur_row0) + rel0) * (N + 1) + (copies ? ((uint32_t)lane % EPI_REPL) * repl_stride() : 0u);
    }
    template <class F>
    __device__ __forceinline__ void finish(F &&before_flush) {  // the end of the workgroup's range
        unreplicate();
        before_flush();
        __syncthreads();
        if (cur_row0 != ~0ull) flush_hist(N, hist, bins, cur_row0, tid, MAXB);
    }
    __device__ __forceinline__ void finish() { finish([] {}); }
};

// The tiles a statistics workgroup takes: a contiguous range, cut in units of `gt` tiles (the group paths' granule).
// ranges == NULL: the launch covers tiles [0, ntiles), split evenly over the grid.  Otherwise (a CHUNK of a run whose
// probe launches are interleaved with their statistics passes, pg_api.hip: anchor_run): the launch covers the tile ranges
// ranges[0 .. gridDim.x / wpr) — what one slice of the co-schedule touches of every genome — with wpr workgroups each.
struct EpiRange {
    uint32_t begin, end;
};
__device__ __forceinline__ EpiRange epi_range(uint32_t gt, uint32_t ntiles, const uint2 *ranges, uint32_t wpr) {
    uint32_t lo = 0, hi = ntiles, j = blockIdx.x, n = gridDim.x;
    if (ranges) {
        const uint2 rg = ranges[blockIdx.x / wpr];
        lo = rg.x;
        hi = rg.y;
        j = blockIdx.x % wpr;
        n = wpr;
    }
    const uint32_t ngroups = (hi - lo + gt - 1) / gt;
    EpiRange e;
    e.begin = lo + gt * (uint32_t)((uint64_t)ngroups * j / n);
    e.end = min(hi, lo + gt * (uint32_t)((uint64_t)ngroups * (j + 1) / n));
    return e;
}

// What every statistics kernel starts from: the LDS carved into the histogram window and `ncs` column counters behind it, both
// zeroed; the launch's flags; an empty contig descriptor; the workgroup's tile range in units of `gt` tiles.
struct EpiStart {
    HistWindow win;
    uint32_t *cs;
    bool want_cs, want100;  // column sums asked for; bitmap.100 written here (flags bit 1: k_lowres takes the low-resolution rows, step != 100)
    uint32_t t_begin, t_end;
    AnchorDesc a;
};
__device__ __forceinline__ EpiStart epi_prologue(uint4 *smem, uint32_t N, uint32_t ncs, uint32_t flags, uint32_t *bins, uint32_t gt,
                                                 uint32_t ntiles, const uint2 *ranges, uint32_t wpr) {
    EpiStart s;
    const int tid = threadIdx.x;
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
    const uint32_t MAXB = max(EPI_MAXB, (flags >> 8) & 0xFFu);  // bins in the LDS window (launcher's choice)
    s.cs = hist + ((MAXB * (N + 1) + 3) & ~3u);
    for (uint32_t i = tid; i < MAXB * (N + 1); i += EPI_THREADS) hist[i] = 0;
    for (uint32_t i = tid; i < ncs; i += EPI_THREADS) s.cs[i] = 0;
    __syncthreads();
    s.win.hist = hist;
    s.win.bins = bins;
    s.win.N = N;
    s.win.MAXB = MAXB;
    s.win.MINBIN = epi_minbin(MAXB);
    s.win.tid = tid;
    s.win.cur_row0 = ~0ull;
    s.win.repl = false;
    s.want_cs = (flags & 1u) != 0;
    s.want100 = (flags & 2u) == 0;
    const EpiRange er = epi_range(gt, ntiles, ranges, wpr);
    s.t_begin = er.begin;
    s.t_end = er.end;
    s.a.out_off = s.a.out100_off = s.a.bin_off = 0;
    s.a.nkmers = s.a.binlen = s.a.tile0 = s.a.nbins = 0;
    return s;
}

// column sums are kept per contig (colsums[contig][N]): the workgroup's N plain LDS counters are emptied whenever its tile
// range moves on to another contig (block-uniform, rare)
__device__ __forceinline__ void flush_colsums(uint32_t N, uint32_t *cs, unsigned long long *colsums, uint32_t contig, int tid) {
    __syncthreads();
    for (uint32_t i = tid; i < N; i += EPI_THREADS) {
        const uint32_t v = cs[i];
        if (v) {
            atomicAdd(&colsums[(uint64_t)contig * N + i], (unsigned long long)v);
            cs[i] = 0;
        }
    }
    __syncthreads();
}

// The low-resolution copy takes every 100th row: among a thread's n <= 100 consecutive rows from pos0 there is at most one,
// row `r100` of the copy, `first` rows behind pos0 — it is one of the thread's if first < n.
struct Hit100 {
    uint32_t r100, first;
};
__device__ __forceinline__ Hit100 hit100(uint32_t pos0) {
    Hit100 h;
    h.r100 = (pos0 + 99u) / 100u;
    h.first = h.r100 * 100u - pos0;
    return h;
}

// one row of NBT bytes copied to the low-resolution bitmap: one unaligned 16-byte read (it may reach into the rows that follow, or
// into the 16 bytes of slack every row buffer carries), whole words and the tail's bytes written
template <int NBT>
__device__ __forceinline__ void copy_row_w(const uint8_t *pr, uint8_t *o) {
    const U128 t = *reinterpret_cast<const U128 *>(pr);
    const uint32_t xw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int w = 0; w < NBT / 4; ++w) reinterpret_cast<U32 *>(o + 4 * w)->v = xw[w];
#pragma unroll
    for (int bb = 0; bb < NBT % 4; ++bb) o[4 * (NBT / 4) + bb] = (uint8_t)(xw[(NBT / 4) & 3] >> (8 * bb));
}

// A tile whose bins are shorter than MINBIN — it may span more bins than the window holds (rows of 1..8 bytes): byte loads, the
// histogram wave-aggregated into the window or, beyond it, global memory; one ballot per genome for the column sums.
template <int NBT, int PT>
__device__ __forceinline__ void epi_tile_unwindowed(const HistWindow &win, uint32_t N, const AnchorDesc &a, const uint8_t *g, uint32_t p0,
                                                    uint32_t npos, uint32_t tile_start, uint32_t bin0, uint32_t bin0_start,
                                                    uint32_t rel_base, bool want100, bool want_cs, uint8_t *out100, uint32_t *cs, int lane) {
    constexpr uint32_t nbytes = NBT;
    const uint32_t ndbs_all = (N + 31) / 32;
#pragma unroll
    for (int jj = 0; jj < PT; ++jj) {
        const uint32_t pl = p0 + jj;
        const bool active = pl < npos;
        const uint32_t pos = tile_start + pl;
        uint32_t popc = 0;
        const bool is100 = want100 && active && (pos % 100u == 0);
        for (uint32_t d = 0; d < ndbs_all; ++d) {
            const uint32_t nb = min(4u, nbytes - 4 * d);
            uint32_t wv = 0;
            if (active)
                for (uint32_t bb = 0; bb < nb; ++bb) wv |= (uint32_t)g[(uint64_t)pl * nbytes + 4 * d + bb] << (8 * bb);
            popc += __popc(wv);
            if (is100) {
                uint8_t *o100 = out100 + a.out100_off + (uint64_t)(pos / 100u) * nbytes + 4 * d;
                for (uint32_t bb = 0; bb < nb; ++bb) o100[bb] = (uint8_t)(wv >> (8 * bb));
            }
            if (want_cs) colsum_word(wv, d, N, cs, lane);
        }
        hist_position(active, pos, popc, N, a.binlen, bin0, bin0_start, rel_base, win.hist, win.bins, a.bin_off, lane, win.MAXB);
    }
}

// (k_epilogue_b1's bit-sliced planes) row j = 4 * word + byte of a thread sits at bit 8 * byte + word of every plane: the rows below j
__device__ __forceinline__ uint32_t b1_rows_below(uint32_t j) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t rb = 0; rb < 4; ++rb) {
        const uint32_t nw = j > rb ? min(8u, (j - rb + 3u) >> 2) : 0u;  // words whose byte rb is below row j
        m |= ((1u << nw) - 1u) << (8u * rb);
    }
    return m;
}

// ---------------------------------------------------------------------------
// One-byte rows (N <= 8): persistent workgroups, register accumulators.
// GROUP PATH: 8 full tiles of one contig inside one bin = 32 one-byte rows per thread in two
// 16-byte loads, worked on BIT-SLICED: a three-stage butterfly between the 8 words regroups their 256 bits so
// that word g holds bit g of all 32 rows (same row, same bit position in every word: 4 instructions per word
// pair and stage); an 8-input sorting network on those planes (19 compare-exchanges = AND / OR pairs) turns
// them into thresholds "row has more than i bits"; popcounts of the planes are the column sums, popcounts of
// the thresholds the cumulative histogram.  3.2 instructions per row, where one-hot adds per row took 13.
// Two kinds of group: (1) all 4096 rows inside ONE bin — thresholds and rows counted in registers, reduced when the
// bin changes; (2) several bins (contigs of a few kb .. Mb have bins of nkmers / 100 rows): bins of at least 32
// rows, so that a thread's 32 rows meet at most one bin boundary, and all of the group's bins inside the LDS window —
// the thread splits its threshold popcounts at the boundary (a mask over the planes' bit positions) and adds the
// classes of its one or two bins to the window with up to 9 LDS atomics each, where the per-tile path does one per row.
// A group need not be whole: a contig's last tiles (and a workgroup's last ones) form a group of fewer rows — a thread
// then holds nv < 32 valid rows (possibly none) and masks the planes with the same kind of position mask.
// STREAK: whole one-bin groups known to follow the current one inside its bin, contig and tile range.  This
// pass is bound by its SCALAR instructions — a SIMD issues at most one per four cycles, and the block-uniform bookkeeping of
// a group (two tile_contig look-ups, six divisions by the bin length at 11 instructions each, the window checks) came to
// 330 of them against 195 vector instructions (100 dummy s_add per group: +0.07 ms on 8 x 10^8 rows, 100 dummy VALU: +0.04;
// profiles/r4e_stats_scalar_bound.txt).  Worked out ONCE when a group turns out whole and inside one bin; the groups of
// the streak then take nothing of that: same contig, same bin row, no window check, the next group's prefetch certain.
// (held to the registers of 7 waves per SIMD — 72 VGPRs and 20 bytes of scratch on a cold path instead of 79,
// 96 SGPRs instead of 106: 6 -> 7 workgroups per CU, the pass 0.362 -> 0.353 ms on 8 x 10^8 rows, 0.616 -> 0.588 on
// 1.6 x 10^9; 8 waves (64 VGPRs, 40 bytes of scratch) are slower, 0.392; profiles/r4b_ab_epilogue_waves.txt)
// ---------------------------------------------------------------------------
#ifndef PG_EPI_WAVES0
#define PG_EPI_WAVES0 7
#endif
#ifndef PG_EPI_SGPRS0
#define PG_EPI_SGPRS0 96
#endif
__global__ __launch_bounds__(EPI_THREADS, PG_EPI_WAVES0)
__attribute__((amdgpu_num_sgpr(PG_EPI_SGPRS0))) void k_epilogue_b1(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                             const uint32_t *__restrict__ tile_contig, uint32_t ntiles,
                                                             const uint8_t *__restrict__ out1, uint8_t *__restrict__ out100,
                                                             uint32_t *__restrict__ bins,
                                                             unsigned long long *__restrict__ colsums, uint32_t flags,
                                                             const uint2 *__restrict__ ranges, uint32_t wpr) {
    extern __shared__ uint4 smem[];
    constexpr int PT = 4;  // rows per thread and tile: EPI_THREADS = PROBE_TILE / 4 threads per workgroup
    const int tid = threadIdx.x, lane = tid & 63;
    // contiguous tile ranges, cut in units of the group path's 8 tiles (32 rows per thread)
    EpiStart st = epi_prologue(smem, N, N, flags, bins, 8u, ntiles, ranges, wpr);
    HistWindow &win = st.win;
    uint32_t *const hist = win.hist, *const cs = st.cs;
    const uint32_t MAXB = win.MAXB, MINBIN = win.MINBIN;
    const bool want_cs = st.want_cs, want100 = st.want100;
    const uint32_t t_begin = st.t_begin, t_end = st.t_end;
    uint32_t cur_c = ~0u;
    AnchorDesc a = st.a;
    const uint32_t p0 = tid * PT;
    // per-thread accumulators, reduced over the workgroup only when the bin
    // changes / at the end: 9 popcount classes as 7-bit fields of one u64 (spilled to the u32 counters
    // below every 31 tiles), 8 column counters
    unsigned long long hacc = 0;
    // ... and of the group path: thr[i] = rows seen with MORE than i bits set (the histogram classes are their
    // differences), grows = rows seen
    uint32_t thr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, grows = 0;
    uint32_t cacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t since_spill = 0;
    uint32_t next_packed = 0;  // software prefetch of the next tile's rows
    bool next_valid = false;
    auto spill = [&]() {  // the per-tile path's classes (7-bit fields of hacc) join the thresholds: thr[i] += rows of class > i
        uint32_t run = 0;
#pragma unroll
        for (int v = 8; v >= 1; --v) {
            run += (uint32_t)(hacc >> (7 * v)) & 127u;
            thr[v - 1] += run;
        }
        grows += run + ((uint32_t)hacc & 127u);
        hacc = 0;
        since_spill = 0;
    };
    auto reduce_hist = [&]() {  // per-thread thresholds -> classes -> LDS histogram (bin-relative row 0)
        spill();
        uint32_t hc[9];
        hc[0] = grows - thr[0];
#pragma unroll
        for (int v = 1; v < 8; ++v) hc[v] = thr[v - 1] - thr[v];
        hc[8] = thr[7];
#pragma unroll
        for (int v = 8; v >= 1; --v)  // (junk bits beyond ngenomes count as class N, as on the per-tile path)
            if ((uint32_t)v > N) {
                hc[v - 1] += hc[v];
                hc[v] = 0;
            }
        grows = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) thr[v] = 0;
#pragma unroll
        for (int v = 0; v < 9; ++v)
            if ((uint32_t)v <= N && hc[v]) lds_add_lanes(&hist[v], hc[v]);
    };
    auto contig_done = [&](uint32_t contig) {  // the register column counters join the LDS ones, those leave for the contig's sums
#pragma unroll
        for (int gb = 0; gb < 8; ++gb) {
            if ((uint32_t)gb < N && cacc[gb]) lds_add_lanes(&cs[gb], cacc[gb]);
            cacc[gb] = 0;
        }
        flush_colsums(N, cs, colsums, contig, tid);
    };
    uint4 gq_next = make_uint4(0, 0, 0, 0), gq_next2 = make_uint4(0, 0, 0, 0);  // group path: prefetched rows of the next group
    bool gq_valid = false;
    // the streak (see above the kernel): whole one-bin groups known to follow, and what the group before worked out of the next one
    uint32_t streak = 0, nk_ba = 0, nk_bz = 0;
    int nk_kind = 0;
    for (uint32_t tile = t_begin; tile < t_end; ++tile) {
        uint32_t c = cur_c;
        if (!(streak || gq_valid)) {  // (a group the one before has announced lies in its contig)
            c = tile_contig[tile];
            if (c != cur_c) {  // block-uniform; consecutive tiles nearly always share their contig
                if (want_cs && cur_c != ~0u) contig_done(cur_c);
                a = ad[c];
                cur_c = c;
            }
        }
        // ---- group path (see above the kernel) ----
        {
            const uint32_t ts = (tile - a.tile0) * PROBE_TILE;
            const uint32_t span = 8u * PROBE_TILE;
            // rows of this contig from ts on that belong to this workgroup's tile range, at most a whole group's
            auto rows_at = [&](uint32_t tl, uint32_t t0) -> uint32_t {  // (block-uniform)
                if (tl >= t_end || tile_contig[tl] != c || t0 >= a.nkmers) return 0u;
                return min(min(span, a.nkmers - t0), (t_end - tl) * (uint32_t)PROBE_TILE);
            };
            // (block-uniform) first and last bin of the rows [t0, t0 + rows) and the kind of group they make — 1: one bin, 2: several
            // bins, 0: not a group
            auto group_kind = [&](uint32_t t0, uint32_t rows, uint32_t &ba, uint32_t &bz) -> int {
                if (rows == 0) return 0;
                const uint32_t bl = a.binlen;
                ba = t0 / bl;
                bz = (t0 + rows - 1) / bl;
                if (ba == bz) return 1;
                return (bl >= 32u && bz - ba + 1u <= MAXB) ? 2 : 0;
            };
            const bool fast = streak != 0;  // (block-uniform) a group of a streak: whole, one bin, the bin of the group before
            const bool known = !fast && gq_valid;  // the group before worked this one out (whole; nk_kind, nk_ba .. nk_bz) when it asked for its rows
            uint32_t grows_n = span, ba = nk_ba, bz = nk_bz;
            int kind = fast ? 1 : nk_kind;
            if (fast) {
                --streak;
            } else if (!known) {
                grows_n = rows_at(tile, ts);  // (>= 1: this tile has rows)
                kind = group_kind(ts, grows_n, ba, bz);
            }
            if (kind != 0) {
                uint64_t row0g = win.cur_row0;
                if (!fast) {
                    row0g = a.bin_off + ba;
                    // (a one-bin group's thresholds are counted in registers: they stand for the window's first row)
                    win.seat_tile(row0g, bz - ba, true, kind == 1, reduce_hist);
                    if (kind == 1 && grows_n == span) {
                        // whole groups from ts on that end inside this bin, this contig and this workgroup's range (this one included)
                        const uint64_t bin_end = min((uint64_t)(ba + 1u) * a.binlen, (uint64_t)a.nkmers);
                        streak = min((uint32_t)(bin_end - ts) / span, (t_end - tile) / 8u) - 1u;
                    }
                }
                const uint32_t nv = 32u * tid < grows_n ? min(32u, grows_n - 32u * tid) : 0u;  // this thread's valid rows
                // (a 16-byte load that begins on a valid row ends inside the contig's 16-byte padded region)
                const uint4 *gg = reinterpret_cast<const uint4 *>(out1 + a.out_off + (uint64_t)ts + 32u * tid);
                const uint4 z4 = make_uint4(0, 0, 0, 0);
                const uint4 qa = gq_valid ? gq_next : (nv > 0u ? gg[0] : z4);
                const uint4 qb = gq_valid ? gq_next2 : (nv > 16u ? gg[1] : z4);
                // This group's rows are waited for HERE, before the next group's loads go out.  Left to the compiler the wait sat
                // at the rows' first use — BEHIND the prefetch — and, the paths above having merged, as vmcnt(0): it waited for
                // the prefetch as well, so that a group's load latency and its arithmetic ran one after the other (0.35 ms for
                // 8 x 10^8 rows where a kernel of the same geometry that only loads and counts takes 0.19).
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), nothing else
                // prefetch the next group when this one is whole and a whole group follows right behind
                const uint32_t tiles_here = (grows_n + PROBE_TILE - 1) / PROBE_TILE;
                gq_valid = streak != 0;
                if (!gq_valid && grows_n == span && rows_at(tile + 8, ts + span) == span) {
                    nk_kind = group_kind(ts + span, span, nk_ba, nk_bz);
                    gq_valid = nk_kind != 0;
                }
                if (gq_valid) {
                    gq_next = gg[span / 16u];
                    gq_next2 = gg[span / 16u + 1];
                }
                uint32_t w[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                const uint32_t pos0 = ts + 32u * tid;
                const Hit100 h = hit100(pos0);
                if (want100 && h.first < nv) {
                    uint32_t sel = w[0];
#pragma unroll
                    for (uint32_t i = 1; i < 8; ++i) sel = (h.first >> 2) == i ? w[i] : sel;
                    out100[a.out100_off + h.r100] = (uint8_t)(sel >> (8 * (h.first & 3)));
                }
#pragma unroll
                for (int kb = 0; kb < 3; ++kb) {
                    const uint32_t m0 = kb == 0 ? 0x55555555u : kb == 1 ? 0x33333333u : 0x0F0F0F0Fu;
                    const int sh = 1 << kb;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (i & sh) continue;
                        const uint32_t x = w[i], y = w[i | sh];
                        w[i] = (x & m0) | ((y << sh) & ~m0);       // the pair's bits with bit kb of g clear
                        w[i | sh] = ((x >> sh) & m0) | (y & ~m0);  // ... and set
                    }
                }
                const bool whole = grows_n == span;  // (block-uniform)
                const uint32_t mval = whole ? 0xFFFFFFFFu : b1_rows_below(nv);
                if (!whole) {
#pragma unroll
                    for (int gb = 0; gb < 8; ++gb) w[gb] &= mval;  // rows past the group hold whatever follows in memory
                }
                if (want_cs) {
#pragma unroll
                    for (int gb = 0; gb < 8; ++gb) cacc[gb] += __popc(w[gb]);
                }
                auto cx = [&](int i, int j) __attribute__((always_inline)) {
                    const uint32_t lo = w[i] & w[j], hi = w[i] | w[j];
                    w[i] = lo;
                    w[j] = hi;
                };
                cx(0, 1), cx(2, 3), cx(4, 5), cx(6, 7);
                cx(0, 2), cx(1, 3), cx(4, 6), cx(5, 7);
                cx(1, 2), cx(5, 6), cx(0, 4), cx(3, 7);
                cx(1, 5), cx(2, 6);
                cx(1, 4), cx(3, 6);
                cx(2, 4), cx(3, 5);
                cx(3, 4);
                if (kind == 1) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) thr[i] += __popc(w[7 - i]);  // ascending order: w[7] = any bit set
                    grows += nv;
                } else {
                    // this thread's rows pos0 .. pos0 + nv - 1: bin of the first one (relative to the group's first bin) and
                    // rows until the next bin boundary
                    const uint32_t bl = a.binlen, bin0s = ba * bl, d0 = pos0 - bin0s;  // (ba = ts / bl)
                    const uint32_t rel0 = bl >= span ? (d0 >= bl ? 1u : 0u) : __umulhi(d0, 0xFFFFFFFFu / bl + 1u);  // (d0 < 2^16)
                    const uint32_t jb = min(nv, (rel0 + 1u) * bl - d0);  // valid rows of the first bin
                    const uint32_t mlo = b1_rows_below(jb);
                    uint32_t *h0 = hist + ((uint32_t)(row0g - win.cur_row0) + rel0) * (N + 1);
                    auto add_classes = [&](uint32_t *hb, uint32_t mask, uint32_t rows) __attribute__((always_inline)) {
                        uint32_t cl[9], above = rows;
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const uint32_t t = (uint32_t)__popc(w[7 - i] & mask);  // rows of this bin with more than i bits
                            cl[i] = above - t;
                            above = t;
                        }
                        cl[8] = above;
#pragma unroll
                        for (int v = 8; v >= 1; --v)  // (junk bits beyond ngenomes count as class N)
                            if ((uint32_t)v > N) {
                                cl[v - 1] += cl[v];
                                cl[v] = 0;
                            }
#pragma unroll
                        for (int v = 0; v < 9; ++v)
                            if ((uint32_t)v <= N && cl[v]) atomicAdd(&hb[v], cl[v]);
                    };
                    if (jb) add_classes(h0, mlo, jb);
                    if (jb < nv) add_classes(h0 + (N + 1), mval & ~mlo, nv - jb);
                }
                next_valid = false;
                tile += tiles_here - 1;
                continue;
            }
            gq_valid = false;
        }
        // ---- one tile: 4 one-byte rows per thread in one 32-bit word ----
        const uint32_t tile_start = (tile - a.tile0) * PROBE_TILE;
        const uint32_t npos = min((uint32_t)PROBE_TILE, a.nkmers - tile_start);
        const uint32_t binlen = a.binlen, bin0 = tile_start / binlen, bin0_start = bin0 * binlen;
        const uint64_t row0 = a.bin_off + bin0;
        const bool onebin = (tile_start + npos) <= (bin0_start + binlen);  // block-uniform
        const bool big = binlen >= (uint32_t)PROBE_TILE;                    // a tile spans at most 2 bins
        const bool windowed = binlen >= MINBIN;                             // ... at most MAXB bins
        const uint32_t last_rel = (tile_start + npos - 1 - bin0_start) / binlen;
        // (bin - bin0) of a position for short bins: exact for pos - bin0_start < 2^16 > tile + bin
        const uint32_t binv = big ? 0u : 0xFFFFFFFFu / binlen + 1u;
        // The per-thread accumulators stand for the window's first bin, so a one-bin tile needs row0 == cur_row0.
        const bool reg_tile = big && onebin;
        const uint32_t rel_base = win.seat_tile(row0, last_rel, windowed, reg_tile, reduce_hist);
        auto rel_of = [&](uint32_t pos) -> uint32_t {  // bin of a position of this tile, relative to bin0
            const uint32_t dpos = pos - bin0_start;
            return big ? (dpos >= binlen ? 1u : 0u) : __umulhi(dpos, binv);
        };
        const uint8_t *g = out1 + a.out_off + (uint64_t)tile_start;
        if (windowed) {
            uint32_t packed = 0;
            if (next_valid) packed = next_packed;
            else if (p0 + 3 < npos) packed = *reinterpret_cast<const uint32_t *>(g + p0);
            else
                for (uint32_t j = 0; j < 4; ++j)
                    if (p0 + j < npos) packed |= (uint32_t)g[p0 + j] << (8 * j);
            // prefetch: the next tile of the same contig is a full tile right behind this one
            next_valid = (tile + 1 < t_end) && (npos == (uint32_t)PROBE_TILE) &&
                         (tile_start + 2u * PROBE_TILE <= a.nkmers) && (tile_contig[tile + 1] == c);
            if (next_valid) next_packed = *reinterpret_cast<const uint32_t *>(g + PROBE_TILE + p0);
            const uint32_t nact = p0 < npos ? min(4u, npos - p0) : 0u;
            if (want_cs) {  // bit g of the 4 rows = bits g, g+8, g+16, g+24 of the word
#pragma unroll
                for (int gb = 0; gb < 8; ++gb) cacc[gb] += __popc(packed & (0x01010101u << gb));
            }
            if (reg_tile) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pcj = min((uint32_t)__popc((packed >> (8 * j)) & 0xFFu), N);
                    if ((uint32_t)j < nact) hacc += 1ull << (7 * pcj);
                }
                if (++since_spill == 31) spill();
            } else {  // the tile spans several bins: one LDS counter per (bin, popcount)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((uint32_t)j < nact)
                        atomicAdd(&hist[(rel_base + rel_of(tile_start + p0 + j)) * (N + 1) +
                                        min((uint32_t)__popc((packed >> (8 * j)) & 0xFFu), N)], 1u);
            }
            if (nact) {
                const Hit100 h = hit100(tile_start + p0);
                if (want100 && h.first < nact) out100[a.out100_off + h.r100] = (uint8_t)(packed >> (8 * h.first));
            }
        } else {
            next_valid = false;
            epi_tile_unwindowed<1, PT>(win, N, a, g, p0, npos, tile_start, bin0, bin0_start, rel_base, want100, want_cs, out100, cs, lane);
        }
    }
    if (want_cs && cur_c != ~0u) contig_done(cur_c);
    win.finish(reduce_hist);
}

// ---------------------------------------------------------------------------
// Rows of 2..8 bytes (9..64 genomes), one or two words per row: one instantiation, and one register allocation, per width.
// Column sums in two levels, all in registers until the very end —
//  L1  the counter planes of pg_planes.h, per thread and word;
//  L2  every PLANES_FLUSH rows the planes are transposed into byte counters, and a halving exchange over the wave
//      leaves each total in one lane, which adds it to the workgroup's LDS counters.
// (rows of 2 to 5 bytes: 6 waves per SIMD instead of the 4-5 their 96-106 VGPRs allowed — 12 x 60 Mb 0.578 -> 0.509 ms,
// 20 x 40 Mb 0.647 -> 0.57, 27 x 40 Mb and 40 x 30 Mb 2-6 %; 8-byte rows lose with it, 1.95 -> 2.1-2.3 ms, and stay as they were)
// ---------------------------------------------------------------------------
#ifndef PG_EPI_WAVES1
#define PG_EPI_WAVES1 6
#endif
template <int NBT>  // NBT = bytes per row (2..8)
__global__ __launch_bounds__(EPI_THREADS, (NBT <= 5 ? PG_EPI_WAVES1 : 1))
__attribute__((amdgpu_num_sgpr(PG_EPI_SGPRS0))) void k_epilogue_n(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                            const uint32_t *__restrict__ tile_contig, uint32_t ntiles,
                                                            const uint8_t *__restrict__ out1, uint8_t *__restrict__ out100,
                                                            uint32_t *__restrict__ bins,
                                                            unsigned long long *__restrict__ colsums, uint32_t flags,
                                                            const uint2 *__restrict__ ranges, uint32_t wpr) {
    static_assert(NBT >= 2 && NBT <= 8, "rows of 2..8 bytes");
    extern __shared__ uint4 smem[];
    constexpr int PT = 4;  // rows per thread and tile: EPI_THREADS = PROBE_TILE / 4 threads per workgroup
    constexpr uint32_t nbytes = NBT;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t ndbs = (N + 31) / 32;
    // contiguous tile ranges, cut in units of the group path's 4 tiles (16 rows per thread)
    EpiStart st = epi_prologue(smem, N, N, flags, bins, 4u, ntiles, ranges, wpr);
    HistWindow &win = st.win;
    uint32_t *const hist = win.hist, *const cs = st.cs;
    const uint32_t MAXB = win.MAXB, MINBIN = win.MINBIN;
    const bool want_cs = st.want_cs, want100 = st.want100;
    const uint32_t t_begin = st.t_begin, t_end = st.t_end;
    uint32_t cur_c = ~0u;
    AnchorDesc a = st.a;
    const uint32_t p0 = tid * PT;
    uint4 wp_a = make_uint4(0, 0, 0, 0), wp_b = make_uint4(0, 0, 0, 0);  // software prefetch of the next tile's 4- / 8-byte rows
    bool wp_valid = false;
    // This kernel keeps ITS OWN WORDING of two shared pieces, because its registers and scratch follow the parent's only so
    // (profiles/stats_share_isa.txt): the flush of the planes below (through planes_flush_wave the loop nest of the exchange is
    // compiled inside an always_inline function and comes out with R[] dynamically indexed: 3.7 -> 17.7 thousand VALU), and
    // the unwindowed tile path at the bottom of the tile loop.  The planes are the three arrays Planes is a view of.
    const uint32_t Nw = N;
    uint32_t vp[2][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}}, pf[2] = {0, 0}, pe[2] = {0, 0};
    uint32_t vrows = 0;  // rows in the planes (block-uniform, a multiple of 4): the carries held back follow from it
    auto ripple = [&](uint32_t (&p)[8], uint32_t cw, int q0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q >= q0) {
                const uint32_t n = p[q] & cw;
                p[q] ^= cw;
                cw = n;
            }
    };
    auto vadd4 = [&](int ws, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) __attribute__((always_inline)) {
        Planes(vp[ws], pf[ws], pe[ws]).add4(r0, r1, r2, r3, Planes::odd4(vrows), Planes::odd8(vrows));  // (the caller advances vrows once all words of the four rows are in)
    };
    auto vflush = [&]() {  // L1 -> L2, wave-uniform call sites only
        const bool odd4 = Planes::odd4(vrows), odd8 = Planes::odd8(vrows);  // carries still held back (a flush between whole 16-row blocks)
        for (uint32_t ws = 0; ws < ndbs && ws < 2; ++ws) {
            if (odd4) ripple(vp[ws], pf[ws], 2);
            if (odd8) ripple(vp[ws], pe[ws], 3);
            uint32_t R[16];
#pragma unroll
            for (int q = 0; q < 8; ++q) {  // byte b of v counts genome 32 ws + 8 b + q (up to 255 rows)
                uint32_t v = 0;
#pragma unroll
                for (int pl = 0; pl < 8; ++pl) v |= ((vp[ws][pl] >> q) & 0x01010101u) << pl;
                R[2 * q] = v & 0x00FF00FFu;
                R[2 * q + 1] = (v >> 8) & 0x00FF00FFu;
            }
#pragma unroll
            for (int pl = 0; pl < 8; ++pl) vp[ws][pl] = 0;
#pragma unroll
            for (int half = 8, bit = 32; half >= 1; half >>= 1, bit >>= 1) {
                const bool up = (lane & bit) != 0;
#pragma unroll
                for (int i = 0; i < half; ++i) {
                    const uint32_t send = up ? R[i] : R[i + half];
                    const uint32_t keep = up ? R[i + half] : R[i];
                    R[i] = keep + (uint32_t)__shfl_xor((int)send, bit);
                }
            }
            R[0] += (uint32_t)__shfl_xor((int)R[0], 2);
            R[0] += (uint32_t)__shfl_xor((int)R[0], 1);
            if ((lane & 3) == 0) {  // this lane holds register (lane >> 2): q = idx / 2, odd idx = bytes 1 and 3
                const uint32_t idx = (uint32_t)lane >> 2;
                const uint32_t g0 = 32 * ws + (idx >> 1) + ((idx & 1) ? 8u : 0u);
                if (g0 < Nw && (R[0] & 0xFFFFu)) atomicAdd(&cs[g0], R[0] & 0xFFFFu);
                if (g0 + 16 < Nw && (R[0] >> 16)) atomicAdd(&cs[g0 + 16], R[0] >> 16);
            }
        }
        vrows = 0;
    };
    auto contig_done = [&](uint32_t contig) {  // what the planes hold joins the LDS counters, those leave for the contig's sums
        if (vrows) vflush();
        flush_colsums(N, cs, colsums, contig, tid);
    };
    for (uint32_t tile = t_begin; tile < t_end; ++tile) {
        const uint32_t c = tile_contig[tile];
        if (c != cur_c) {  // block-uniform; consecutive tiles nearly always share their contig
            if (want_cs && cur_c != ~0u) contig_done(cur_c);
            a = ad[c];
            cur_c = c;
        }
        // ---- group path: 4 full tiles of one contig inside one bin = 16 consecutive
        // rows per thread (4 x nbytes aligned words).  The per-tile bookkeeping (bin arithmetic, window
        // check, 1-in-100 search) is paid once per 16 rows instead of once per 4 — it was two thirds of
        // the instructions of this pass — and the histogram index needs no bin lookup ----
        {
            const uint32_t ts = (tile - a.tile0) * PROBE_TILE;
            const uint32_t span = 4u * PROBE_TILE;
            // (the group may span several bins — contigs under 20 Mb have bins of nkmers / 100 rows — as long as a bin holds
            // at least 16 rows, so that a thread's 16 rows meet at most one boundary, and the group's bins fit the LDS window)
            const uint32_t nbg = (ts + span - 1) / a.binlen - ts / a.binlen + 1u;  // bins of the group
            const bool grp_ok = tile + 3 < t_end && tile_contig[tile + 3] == c && ts + span <= a.nkmers &&
                                (nbg == 1u || (a.binlen >= 16u && nbg <= MAXB));
            if (grp_ok) {
                const uint64_t row0g = a.bin_off + ts / a.binlen;
                const bool copies = win.seat_group(row0g, nbg);
                // this thread's 16 rows: bin of the first one (relative to the group's first bin) and rows until the boundary
                uint32_t rel0 = 0, jb = 16;
                if (nbg > 1u) {
                    const uint32_t bl = a.binlen, d0 = ts + 16u * tid - (ts / bl) * bl;
                    rel0 = bl >= span ? (d0 >= bl ? 1u : 0u) : __umulhi(d0, 0xFFFFFFFFu / bl + 1u);  // (d0 < 2^16)
                    jb = min(16u, (rel0 + 1u) * bl - d0);
                }
                uint32_t *hrow = win.group_row(row0g, rel0, copies, lane);
                const uint8_t *gt = out1 + a.out_off + ((uint64_t)ts + 16u * tid) * nbytes;
                auto rows16 = [&]() {
                    uint32_t raw[4][8];
#pragma unroll
                    for (int q = 0; q < 4; ++q) load_row_words<NBT>(gt + q * 4 * NBT, raw[q]);  // all 16 rows in flight
                    // (fewer in flight saves registers but measured slower: 2.6 / 2.74 / 2.78 ms at N=64 for 4 / 2 / 1
                    // groups ahead; requesting the NEXT group's rows as well costs a wave of occupancy: 2.2 vs 1.4 ms at N=27)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t w0[4], w1[4];
                        cut4_rows<NBT>(raw[q], w0, w1);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            atomicAdd(&hrow[((uint32_t)(4 * q + j) >= jb ? N + 1 : 0u) +
                                            min((uint32_t)(__popc(w0[j]) + (NBT > 4 ? __popc(w1[j]) : 0)), N)], 1u);
                        if (want_cs) {
                            vadd4(0, w0[0], w0[1], w0[2], w0[3]);
                            if (NBT > 4) vadd4(1, w1[0], w1[1], w1[2], w1[3]);
                            vrows += PT;
                            if (vrows == PLANES_FLUSH) vflush();
                        }
                    }
                };
                rows16();
                // 1-in-100 rows: the row is read again (a cache hit) rather than selected out of 16 register pairs
                const Hit100 h = hit100(ts + 16u * tid);
                if (want100 && h.first < 16u) {
                    const uint8_t *pr = gt + h.first * nbytes;
                    uint8_t *o100 = out100 + a.out100_off + (uint64_t)h.r100 * nbytes;
                    for (uint32_t bb = 0; bb < nbytes; ++bb) o100[bb] = pr[bb];
                }
                wp_valid = false;
                tile += 3;
                continue;
            }
        }
        // ---- one tile: the thread's four rows ----
        win.unreplicate();  // (the per-tile paths read the window in its ordinary form)
        const uint32_t tile_start = (tile - a.tile0) * PROBE_TILE;
        const uint32_t npos = min((uint32_t)PROBE_TILE, a.nkmers - tile_start);
        const uint32_t binlen = a.binlen, bin0 = tile_start / binlen, bin0_start = bin0 * binlen;
        const uint64_t row0 = a.bin_off + bin0;
        const bool big = binlen >= (uint32_t)PROBE_TILE;  // a tile spans at most 2 bins
        const bool windowed = binlen >= MINBIN;           // ... at most MAXB bins
        const uint32_t last_rel = (tile_start + npos - 1 - bin0_start) / binlen;
        // (bin - bin0) of a position for short bins: exact for pos - bin0_start < 2^16 > tile + bin
        const uint32_t binv = big ? 0u : 0xFFFFFFFFu / binlen + 1u;
        const uint32_t rel_base = win.seat_tile(row0, last_rel, windowed);
        auto rel_of = [&](uint32_t pos) -> uint32_t {  // bin of a position of this tile, relative to bin0
            const uint32_t dpos = pos - bin0_start;
            return big ? (dpos >= binlen ? 1u : 0u) : __umulhi(dpos, binv);
        };
        const uint8_t *g = out1 + a.out_off + (uint64_t)tile_start * nbytes;
        if (windowed) {
            // ---- the row bytes as one or two 32-bit words ----
            uint32_t w0[PT], w1[PT];
            if (npos == (uint32_t)PROBE_TILE) {  // (block-uniform) a full tile
                if constexpr (NBT == 4 || NBT == 8) {
                    // the thread's 4 rows are 16 / 32 aligned bytes.  The next tile's are requested before this
                    // tile is worked on when it is an equally regular one right behind: loads issued only when
                    // their tile starts leave the memory latency exposed (2.2-3.4 TB/s of the 6.3 a plain
                    // streaming read reaches with this geometry)
                    constexpr bool two = NBT == 8;
                    uint4 qa, qb = make_uint4(0, 0, 0, 0);
                    const uint8_t *g4 = g + (uint64_t)p0 * nbytes;
                    if (wp_valid) {
                        qa = wp_a;
                        qb = wp_b;
                    } else {
                        qa = *reinterpret_cast<const uint4 *>(g4);
                        if (two) qb = *reinterpret_cast<const uint4 *>(g4 + 16);
                    }
                    wp_valid = (tile + 1 < t_end) && (tile_start + 2u * PROBE_TILE <= a.nkmers) && (tile_contig[tile + 1] == c);
                    if (wp_valid) {
                        const uint8_t *gn = g4 + (uint64_t)PROBE_TILE * nbytes;
                        wp_a = *reinterpret_cast<const uint4 *>(gn);
                        if (two) wp_b = *reinterpret_cast<const uint4 *>(gn + 16);
                    }
                    if (two) {
                        w0[0] = qa.x; w1[0] = qa.y; w0[1] = qa.z; w1[1] = qa.w;
                        w0[2] = qb.x; w1[2] = qb.y; w0[3] = qb.z; w1[3] = qb.w;
                    } else {
                        w0[0] = qa.x; w0[1] = qa.y; w0[2] = qa.z; w0[3] = qa.w;
                        w1[0] = w1[1] = w1[2] = w1[3] = 0;
                    }
                } else {  // other widths: nbytes aligned words, rows cut out with static shifts
                    wp_valid = false;
                    uint32_t raw[8];
                    load_row_words<NBT>(g + (uint64_t)p0 * nbytes, raw);
                    cut4_rows<NBT>(raw, w0, w1);
                }
            } else {  // a contig's last tile: byte loads
                wp_valid = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint64_t r = 0;
                    if (p0 + j < npos)
                        for (uint32_t bb = 0; bb < nbytes; ++bb) r |= (uint64_t)g[(uint64_t)(p0 + j) * nbytes + bb] << (8 * bb);
                    w0[j] = (uint32_t)r;
                    w1[j] = (uint32_t)(r >> 32);
                }
            }
            const uint32_t nact = p0 < npos ? min(4u, npos - p0) : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((uint32_t)j < nact) {
                    const uint32_t pc = __popc(w0[j]) + __popc(w1[j]);
                    atomicAdd(&hist[(rel_base + rel_of(tile_start + p0 + j)) * (N + 1) + min(pc, N)], 1u);
                }
            }
            if (nact) {
                const Hit100 h = hit100(tile_start + p0);
                const uint32_t jsel = h.first;
                if (want100 && jsel < nact) {
                    const uint32_t a0 = jsel == 0 ? w0[0] : jsel == 1 ? w0[1] : jsel == 2 ? w0[2] : w0[3];
                    const uint32_t a1 = jsel == 0 ? w1[0] : jsel == 1 ? w1[1] : jsel == 2 ? w1[2] : w1[3];
                    uint8_t *o100 = out100 + a.out100_off + (uint64_t)h.r100 * nbytes;
                    if constexpr (NBT == 4) *reinterpret_cast<uint32_t *>(o100) = a0;
                    else if constexpr (NBT == 8) *reinterpret_cast<uint2 *>(o100) = make_uint2(a0, a1);
                    else {
                        const uint64_t r = (uint64_t)a0 | ((uint64_t)a1 << 32);
                        for (uint32_t bb = 0; bb < nbytes; ++bb) o100[bb] = (uint8_t)(r >> (8 * bb));
                    }
                }
            }
            if (want_cs) {  // rows beyond npos are zero: adding them is harmless
                vadd4(0, w0[0], w0[1], w0[2], w0[3]);
                if (ndbs > 1) vadd4(1, w1[0], w1[1], w1[2], w1[3]);
                vrows += PT;
                if (vrows == PLANES_FLUSH) vflush();
            }
        } else {
            // (epi_tile_unwindowed's text: called as a function it costs rows of 6..8 bytes a VGPR and moves the scratch of 3 and 5)
            const uint32_t ndbs_all = (N + 31) / 32;
#pragma unroll
            for (int jj = 0; jj < PT; ++jj) {
                const uint32_t pl = p0 + jj;
                const bool active = pl < npos;
                const uint32_t pos = tile_start + pl;
                uint32_t popc = 0;
                const bool is100 = want100 && active && (pos % 100u == 0);
                for (uint32_t d = 0; d < ndbs_all; ++d) {
                    const uint32_t nb = min(4u, nbytes - 4 * d);
                    uint32_t wv = 0;
                    if (active)
                        for (uint32_t bb = 0; bb < nb; ++bb) wv |= (uint32_t)g[(uint64_t)pl * nbytes + 4 * d + bb] << (8 * bb);
                    popc += __popc(wv);
                    if (is100) {
                        uint8_t *o100 = out100 + a.out100_off + (uint64_t)(pos / 100u) * nbytes + 4 * d;
                        for (uint32_t bb = 0; bb < nb; ++bb) o100[bb] = (uint8_t)(wv >> (8 * bb));
                    }
                    if (want_cs) colsum_word(wv, d, N, cs, lane);
                }
                hist_position(active, pos, popc, N, binlen, bin0, bin0_start, rel_base, hist, bins, a.bin_off, lane, MAXB);
            }
        }
    }
    if (want_cs && cur_c != ~0u) contig_done(cur_c);
    win.finish();
}

// ---------------------------------------------------------------------------
// Rows wider than 16 bytes (more than 128 genomes): the same statistics CHUNK-PARALLEL.  A lane owns one
// 16-byte chunk c of the rows it visits (C = ceil(nbytes / 16) consecutive lanes share a row, 64 / C
// rows per wave and step; one 16-byte load per lane and row, contiguous over the wave, at whatever byte
// alignment the row stride gives), so the per-row work (addressing, tail masking, histogram, the
// 1-in-100 test) is paid once per 16 bytes and every lane carries the vertical counters of FOUR words
// whatever the row width.  (Round 2's first version gave every lane one 32-bit word: 45 VALU
// instructions per word, 2.8 wave-instructions per 16-byte row, issue-bound at 2.7 TB/s.)
//   popcount of a row   4 v_bcnt per lane, C - 1 shuffles to the row's first lane, one LDS atomic
//   bitmap.100          each lane copies its chunk of the 1-in-100 rows
//   column sums         the counter planes of pg_planes.h per word, per-lane LDS adds every PLANES_FLUSH rows, per contig
//                       to global
// EXACT: nbytes == 16 C (N a multiple of 128): aligned loads, no tail mask.
// ---------------------------------------------------------------------------
// (it runs 3-4 waves per SIMD on 104-149 VGPRs; round 4's first attempt to hold it to 5 or 6: 65-128 genomes 2.7-5.5 -> 5.0-13.9 ms,
// profiles/r4b_ab_epilogue_waves.txt)
template <int C_T, bool EXACT>  // chunks per row known at compile time (2..4), or 0: any
// (held to the registers of 5 waves per SIMD — 96 — it still spills in the row loop: 65-128 genomes 2.67-5.23 -> 3.04-5.55 ms,
// profiles/r4e_ab_stats_harley_seal.txt)
#ifndef PG_EPI_WAVESC
#define PG_EPI_WAVESC 1
#endif
__global__ __launch_bounds__(EPI_THREADS, PG_EPI_WAVESC) void k_epilogue_chunks(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                                 const uint32_t *__restrict__ tile_contig, uint32_t ntiles,
                                                                 const uint8_t *__restrict__ out1, uint8_t *__restrict__ out100,
                                                                 uint32_t *__restrict__ bins,
                                                                 unsigned long long *__restrict__ colsums, uint32_t flags,
                                                                 const uint2 *__restrict__ ranges, uint32_t wpr) {
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nbytes = (N + 7) / 8, C = C_T ? (uint32_t)C_T : (nbytes + 15) / 16;
    const uint32_t RPW = 64u / C, RPS = RPW * (EPI_THREADS / 64);  // rows per wave / per workgroup and step
    const uint32_t c = (uint32_t)lane % C, rsub = (uint32_t)wave * RPW + (uint32_t)lane / C;
    const bool lane_on = (uint32_t)lane < RPW * C;
    const uint32_t vb = EXACT ? 16u : min(16u, nbytes - 16u * c);  // bytes of this lane's chunk (the row's last one may be short)
    // column counters in LDS: one copy per 16 rows of a wave's step, so that at most 16 lanes add to a word
    // at a time (and the address is lane-dependent: on a wave-uniform address the compiler's atomic
    // optimizer would sum the lanes' values one by one, 64 rounds per counter)
    const uint32_t K = (RPW + 15u) / 16u, cs_words = 128u * C;
    uint32_t wm[4];                                  // ... as masks of its four words
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t nb = vb > 4u * w ? min(4u, vb - 4u * w) : 0u;
        wm[w] = nb == 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u;
    }
    EpiStart st = epi_prologue(smem, N, K * cs_words, flags, bins, 4u, ntiles, ranges, wpr);
    HistWindow &win = st.win;
    uint32_t *const hist = win.hist, *const cs = st.cs;
    const uint32_t MAXB = win.MAXB, MINBIN = win.MINBIN;
    uint32_t *cs_mine = cs + ((uint32_t)lane / C / 16u) * cs_words + 128u * c;
    const bool want_cs = st.want_cs, want100 = st.want100;
    const uint32_t t_begin = st.t_begin, t_end = st.t_end;
    uint32_t cur_c = ~0u;
    AnchorDesc a = st.a;
    uint32_t vp[4][8], pf[4], pe[4];  // column sums of this lane's four words
#pragma unroll
    for (int w = 0; w < 4; ++w) Planes(vp[w], pf[w], pe[w]).clear();
    uint32_t vrows = 0;  // rows in the planes (block-uniform, a multiple of 4): the carries held back follow from it
    auto vflush = [&]() __attribute__((always_inline)) {  // planes -> the workgroup's LDS counters of this lane's words
        const bool odd4 = Planes::odd4(vrows), odd8 = Planes::odd8(vrows);
#pragma unroll
        for (int w = 0; w < 4; ++w) planes_flush_lanes(Planes(vp[w], pf[w], pe[w]), cs_mine + 32 * w, odd4, odd8);
        vrows = 0;
    };
    auto flush_colsums_k = [&](uint32_t contig) __attribute__((always_inline)) {  // ... and the K copies of those -> the contig's sums
        if (vrows) vflush();
        __syncthreads();
        for (uint32_t i = tid; i < N; i += EPI_THREADS) {
            uint32_t v = 0;
            for (uint32_t kk = 0; kk < K; ++kk) {
                v += cs[kk * cs_words + i];
                cs[kk * cs_words + i] = 0;
            }
            if (v) atomicAdd(&colsums[(uint64_t)contig * N + i], (unsigned long long)v);
        }
        __syncthreads();
    };
    // popcount of a whole row from its lanes' chunks, valid (at least) in the row's first lane
    auto row_popc = [&](uint32_t pc) __attribute__((always_inline)) -> uint32_t {
        if (C_T == 2) return pc + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pc, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
        if (C_T == 4) {
            pc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pc, 0xB1, 0xF, 0xF, false);
            return pc + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pc, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
        }
        uint32_t tot = pc;
        for (uint32_t q = 1; q < C; ++q) tot += (uint32_t)__shfl_down((int)pc, q);
        return tot;
    };
    // The rows are streamed in iterations of 4 steps (4 x RPS rows), the loads of iteration i + 1 issued
    // before iteration i is worked on — also across tiles: 8 x 16 bytes per lane in flight.
    constexpr uint32_t NJ = 4;
    const uint32_t iter_rows = NJ * RPS, IPT = ((uint32_t)PROBE_TILE + iter_rows - 1) / iter_rows;
    const uint32_t nit = t_end > t_begin ? (t_end - t_begin) * IPT : 0u;
    auto issue = [&](uint32_t it, uint4 (&out)[NJ]) {
        const uint32_t tile = t_begin + it / IPT, r0 = (it % IPT) * iter_rows;
        const AnchorDesc A = ad[tile_contig[tile]];  // (uniform: scalar loads)
        const uint32_t ts = (tile - A.tile0) * PROBE_TILE;
        const uint32_t npos = min((uint32_t)PROBE_TILE, A.nkmers - ts);
        const uint8_t *g = out1 + A.out_off + (uint64_t)ts * nbytes + 16u * c;
        // branch-free: every lane always loads 16 bytes from a valid row (a predicated load per row makes
        // the compiler wait for each load in turn); a short last chunk reads into the next row — or, at the
        // very end, into the 16 bytes of slack every row buffer carries
#pragma unroll
        for (uint32_t j = 0; j < NJ; ++j) {
            const uint32_t pl = r0 + j * RPS + rsub;
            const uint8_t *q = g + min(pl, npos - 1u) * nbytes;
            if (EXACT) out[j] = *reinterpret_cast<const uint4 *>(q);
            else {
                const U128 t = *reinterpret_cast<const U128 *>(q);
                out[j] = make_uint4(t.x, t.y, t.z, t.w);
            }
        }
    };
    uint4 v[NJ], vn[NJ];
    if (nit) issue(0, v);
    // per-tile state (block-uniform), set when an iteration starts a tile
    uint32_t tile_start = 0, npos = 0, binlen = 1, bin0 = 0, bin0_start = 0, binv = 0, rel_base = 0;
    bool big = false, windowed = false;
    for (uint32_t it = 0; it <= nit; ++it) {  // (one more round: the last contig's column sums, flushed at ONE site)
        const bool fin = it == nit;
        if (it + 1 < nit) issue(it + 1, vn);
        const uint32_t tile = t_begin + it / IPT, r0 = fin ? 0u : (it % IPT) * iter_rows;
        if (r0 == 0) {
            const uint32_t cg = fin ? ~0u : tile_contig[tile];
            if (cg != cur_c) {
                if (want_cs && cur_c != ~0u) flush_colsums_k(cur_c);
                if (!fin) a = ad[cg];
                cur_c = cg;
            }
            if (fin) break;
            tile_start = (tile - a.tile0) * PROBE_TILE;
            npos = min((uint32_t)PROBE_TILE, a.nkmers - tile_start);
            binlen = a.binlen;
            bin0 = tile_start / binlen;
            bin0_start = bin0 * binlen;
            const uint64_t row0 = a.bin_off + bin0;
            big = binlen >= (uint32_t)PROBE_TILE;
            windowed = binlen >= MINBIN;
            const uint32_t last_rel = (tile_start + npos - 1 - bin0_start) / binlen;
            binv = big ? 0u : 0xFFFFFFFFu / binlen + 1u;
            rel_base = win.seat_tile(row0, last_rel, windowed);
        }
        if (r0 < npos) {  // (block-uniform)
            uint32_t *hrow = hist + rel_base * (N + 1);
            const bool full = EXACT && C_T && (64 % (C_T ? C_T : 1) == 0) && r0 + iter_rows <= npos;  // (block-uniform) no row to mask
#pragma unroll
            for (uint32_t j = 0; j < NJ; ++j) {
                const uint32_t pl = r0 + j * RPS + rsub;
                const bool on = full || (lane_on && pl < npos);
                if (!full) {
                    const uint32_t keep = on ? 0xFFFFFFFFu : 0u;
                    v[j].x &= EXACT ? keep : keep & wm[0];
                    v[j].y &= EXACT ? keep : keep & wm[1];
                    v[j].z &= EXACT ? keep : keep & wm[2];
                    v[j].w &= EXACT ? keep : keep & wm[3];
                }
                const uint32_t tot = row_popc(__popc(v[j].x) + __popc(v[j].y) + __popc(v[j].z) + __popc(v[j].w));
                const uint32_t pos = tile_start + pl;
                if (windowed) {
                    if (on && c == 0) {
                        const uint32_t dpos = pos - bin0_start;
                        const uint32_t rel = big ? (dpos >= binlen ? 1u : 0u) : __umulhi(dpos, binv);
                        atomicAdd(&hrow[rel * (N + 1) + min(tot, N)], 1u);
                    }
                } else {
                    hist_position(on && c == 0, pos, tot, N, binlen, bin0, bin0_start, rel_base, hist, bins, a.bin_off, lane, MAXB);
                }
                if (want100 && on && pos % 100u == 0) {  // 1-in-100 rows: every lane copies its chunk
                    uint8_t *o = out100 + a.out100_off + (uint64_t)(pos / 100u) * nbytes + 16u * c;
                    if (EXACT) *reinterpret_cast<uint4 *>(o) = v[j];
                    else {
                        const uint32_t xw[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                        for (uint32_t w = 0; w < 4; ++w) {
                            if (vb >= 4u * w + 4u) reinterpret_cast<U32 *>(o + 4u * w)->v = xw[w];
                            else if (vb > 4u * w)
                                for (uint32_t bb = 0; bb < vb - 4u * w; ++bb) o[4u * w + bb] = (uint8_t)(xw[w] >> (8 * bb));
                        }
                    }
                }
            }
            if (want_cs) {  // rows beyond npos are zero: adding them is harmless
                const bool odd4 = Planes::odd4(vrows), odd8 = Planes::odd8(vrows);
                Planes(vp[0], pf[0], pe[0]).add4(v[0].x, v[1].x, v[2].x, v[3].x, odd4, odd8);
                Planes(vp[1], pf[1], pe[1]).add4(v[0].y, v[1].y, v[2].y, v[3].y, odd4, odd8);
                Planes(vp[2], pf[2], pe[2]).add4(v[0].z, v[1].z, v[2].z, v[3].z, odd4, odd8);
                Planes(vp[3], pf[3], pe[3]).add4(v[0].w, v[1].w, v[2].w, v[3].w, odd4, odd8);
                vrows += 4;
                if (vrows == PLANES_FLUSH) vflush();
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < NJ; ++j) v[j] = vn[j];
    }
    win.finish();
}

// ---------------------------------------------------------------------------
// Rows of 9..16 bytes (65..128 genomes): k_epilogue_n's scheme at THREE or FOUR words per row.
// k_epilogue_chunks gives every row one lane and one (unaligned) 16-byte load whatever its width — ≈ 38 instructions per
// row and lane, 4.1 ps per row at 9 bytes as at 16: the 65th genome paid for 128 (0.98 -> 2.68 ms for one more row byte).
// Here a thread owns RPT consecutive rows of a group of full tiles (NBT aligned words per four rows, cut into rows with
// static funnel shifts; RPT = 8, a group = two tiles: 16 rows per thread as for the narrower widths cost a wave of occupancy
// and 2-7 %, profiles/r5g_ab_stats_w_rows.txt), the group's bookkeeping (bins, window, the 1-in-100 row) is paid once per group,
// the histogram takes one LDS atomic per row (in 8 copies while the group lies inside one or two long bins), and the
// column sums go through the counter planes of pg_planes.h, one set per word.
// Tiles that form no group — a contig's last ones, contigs of a few tiles, bins shorter than 16 rows — take the same
// four rows per thread one tile at a time.  Reference: the per-bin histogram and rows of cpp/anchor.cpp:150-189,
// index.py:1169-1183; column sums: index.py:1051,1068-1074.
// ---------------------------------------------------------------------------
#ifndef PG_EPI_W_GQ12
#define PG_EPI_W_GQ12 2  // k_epilogue_w, rows of 9..12 bytes: tiles per group (4: 16 consecutive rows per thread, 2: 8)
#endif
#ifndef PG_EPI_W_GQ16
#define PG_EPI_W_GQ16 2  // ... rows of 13..16 bytes
#endif
#ifndef PG_EPI_WAVESW12
#define PG_EPI_WAVESW12 1  // waves per SIMD the instantiations of 9..12-byte rows are held to (1: the compiler's choice)
#endif
#ifndef PG_EPI_WAVESW16
#define PG_EPI_WAVESW16 4  // ... of 13..16-byte rows
#endif
template <int NB>
__device__ __forceinline__ void cut4_rows_w(const uint32_t (&raw)[NB], uint32_t (&w)[(NB + 3) / 4][4]) {
    constexpr int NW = (NB + 3) / 4;
    constexpr uint32_t last_keep = (NB % 4) ? ((1u << (8 * (NB % 4))) - 1u) : 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int off = j * NB, idx = off >> 2, sh = 8 * (off & 3);  // (constants once unrolled)
#pragma unroll
        for (int t = 0; t < NW; ++t) {
            const uint32_t lo = raw[idx + t];  // (idx + NW - 1 <= NB - 1: the row ends inside the four rows' words)
            const uint32_t hi = (idx + t + 1 < NB) ? raw[idx + t + 1] : 0u;
            uint32_t v = sh ? __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh) : lo;
            if (t == NW - 1) v &= last_keep;
            w[t][j] = v;
        }
    }
}
template <int NBT>
__global__ __launch_bounds__(EPI_THREADS, (NBT <= 12 ? PG_EPI_WAVESW12 : PG_EPI_WAVESW16)) void k_epilogue_w(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                                          const uint32_t *__restrict__ tile_contig, uint32_t ntiles,
                                                                          const uint8_t *__restrict__ out1, uint8_t *__restrict__ out100,
                                                                          uint32_t *__restrict__ bins,
                                                                          unsigned long long *__restrict__ colsums, uint32_t flags,
                                                                          const uint2 *__restrict__ ranges, uint32_t wpr) {
    static_assert(NBT >= 9 && NBT <= 16, "rows of 9..16 bytes");
    extern __shared__ uint4 smem[];
    constexpr int PT = 4;             // rows per thread and tile
    constexpr int NW = (NBT + 3) / 4;  // words per row
    constexpr int GQ = (NBT <= 12 ? PG_EPI_W_GQ12 : PG_EPI_W_GQ16);  // tiles per group = blocks of four rows per thread and group
    constexpr uint32_t RPT = 4u * GQ;   // consecutive rows of a group per thread
    constexpr uint32_t nbytes = NBT;
    const int tid = threadIdx.x, lane = tid & 63;
    EpiStart st = epi_prologue(smem, N, N, flags, bins, 4u, ntiles, ranges, wpr);
    HistWindow &win = st.win;
    uint32_t *const hist = win.hist, *const cs = st.cs;
    const uint32_t MAXB = win.MAXB, MINBIN = win.MINBIN;
    const bool want_cs = st.want_cs, want100 = st.want100;
    const uint32_t t_begin = st.t_begin, t_end = st.t_end;
    uint32_t cur_c = ~0u;
    AnchorDesc a = st.a;
    const uint32_t p0 = tid * PT;
    uint32_t vp[NW][8], pf[NW], pe[NW];  // column sums, one set of planes per word
#pragma unroll
    for (int w = 0; w < NW; ++w) Planes(vp[w], pf[w], pe[w]).clear();
    uint32_t vrows = 0;  // rows in the planes (block-uniform, a multiple of 4)
    auto vadd_rows = [&](const uint32_t (&w)[NW][4]) __attribute__((always_inline)) {  // four rows into the planes of every word
        const bool odd4 = Planes::odd4(vrows), odd8 = Planes::odd8(vrows);
#pragma unroll
        for (int t = 0; t < NW; ++t) Planes(vp[t], pf[t], pe[t]).add4(w[t][0], w[t][1], w[t][2], w[t][3], odd4, odd8);
        vrows += PT;
    };
    auto vflush = [&]() __attribute__((always_inline)) {  // planes -> the workgroup's LDS counters: ONE (wave-uniform) call site, at the top of the tile loop
        const bool odd4 = Planes::odd4(vrows), odd8 = Planes::odd8(vrows);
#pragma unroll
        for (int ws = 0; ws < NW; ++ws) planes_flush_wave(Planes(vp[ws], pf[ws], pe[ws]), ws, N, cs, lane, odd4, odd8);
        vrows = 0;
    };
    auto popc_row = [&](const uint32_t (&w)[NW][4], int j) __attribute__((always_inline)) -> uint32_t {
        uint32_t pc = (uint32_t)__popc(w[0][j]);
#pragma unroll
        for (int t = 1; t < NW; ++t) pc += (uint32_t)__popc(w[t][j]);
        return min(pc, N);  // (junk bits beyond ngenomes count as class N)
    };
    for (uint32_t tile = t_begin; tile <= t_end; ++tile) {  // (one more round: the last contig's column sums leave at the one site)
        const bool fin = tile >= t_end;
        const uint32_t c = fin ? ~0u : tile_contig[tile];
        // the planes count to PLANES_CEIL rows and a group brings RPT: emptied here when they could not take another group, and
        // when the range moves on to another contig (column sums are kept per contig)
        if (want_cs && vrows && (vrows + RPT > PLANES_CEIL || c != cur_c)) vflush();
        if (c != cur_c) {  // block-uniform
            if (want_cs && cur_c != ~0u) flush_colsums(N, cs, colsums, cur_c, tid);
            if (!fin) a = ad[c];
            cur_c = c;
        }
        if (fin) break;
        // ---- group path: GQ full tiles of one contig = 4 GQ consecutive rows per thread (GQ = 2: 8 rows) ----
        {
            const uint32_t ts = (tile - a.tile0) * PROBE_TILE;
            const uint32_t span = (uint32_t)GQ * PROBE_TILE;
            const uint32_t nbg = (ts + span - 1) / a.binlen - ts / a.binlen + 1u;  // bins of the group
            const bool grp_ok = tile + (GQ - 1) < t_end && tile_contig[tile + (GQ - 1)] == c && ts + span <= a.nkmers &&
                                (nbg == 1u || (a.binlen >= RPT && nbg <= MAXB));
            if (grp_ok) {
                const uint64_t row0g = a.bin_off + ts / a.binlen;
                const bool copies = win.seat_group(row0g, nbg);
                uint32_t rel0 = 0, jb = RPT;  // bin of the thread's first row (relative to the group's first bin), rows until the boundary
                if (nbg > 1u) {
                    const uint32_t bl = a.binlen, d0 = ts + RPT * tid - (ts / bl) * bl;
                    rel0 = bl >= span ? (d0 >= bl ? 1u : 0u) : __umulhi(d0, 0xFFFFFFFFu / bl + 1u);  // (d0 < 2^16)
                    jb = min(RPT, (rel0 + 1u) * bl - d0);
                }
                uint32_t *hrow = win.group_row(row0g, rel0, copies, lane);
                const uint8_t *gt = out1 + a.out_off + ((uint64_t)ts + RPT * tid) * nbytes;
                uint32_t raw[GQ][NBT];
#pragma unroll
                for (int q = 0; q < GQ; ++q) {  // all of the thread's rows in flight
#pragma unroll
                    for (int i = 0; i < NBT; ++i) raw[q][i] = reinterpret_cast<const uint32_t *>(gt + q * 4 * NBT)[i];
                }
#pragma unroll
                for (int q = 0; q < GQ; ++q) {
                    uint32_t w[NW][4];
                    cut4_rows_w<NBT>(raw[q], w);
#pragma unroll
                    for (int j = 0; j < 4; ++j) atomicAdd(&hrow[((uint32_t)(4 * q + j) >= jb ? N + 1 : 0u) + popc_row(w, j)], 1u);
                    if (want_cs) vadd_rows(w);
                }
                // 1-in-100 rows: the row is read again (a cache hit)
                const Hit100 h = hit100(ts + RPT * tid);
                if (want100 && h.first < RPT) copy_row_w<NBT>(gt + h.first * nbytes, out100 + a.out100_off + (uint64_t)h.r100 * nbytes);
                tile += GQ - 1;
                continue;
            }
        }
        // ---- one tile: the thread's four rows ----
        win.unreplicate();
        const uint32_t tile_start = (tile - a.tile0) * PROBE_TILE;
        const uint32_t npos = min((uint32_t)PROBE_TILE, a.nkmers - tile_start);
        const uint32_t binlen = a.binlen, bin0 = tile_start / binlen, bin0_start = bin0 * binlen;
        const uint64_t row0 = a.bin_off + bin0;
        const bool big = binlen >= (uint32_t)PROBE_TILE;  // a tile spans at most 2 bins
        const bool windowed = binlen >= MINBIN;           // ... at most MAXB bins
        const uint32_t last_rel = (tile_start + npos - 1 - bin0_start) / binlen;
        const uint32_t binv = big ? 0u : 0xFFFFFFFFu / binlen + 1u;
        const uint32_t rel_base = win.seat_tile(row0, last_rel, windowed);
        const uint8_t *g = out1 + a.out_off + (uint64_t)tile_start * nbytes;
        const uint32_t nact = p0 < npos ? min(4u, npos - p0) : 0u;
        uint32_t w[NW][4];
        if (npos == (uint32_t)PROBE_TILE) {  // (block-uniform) a full tile: NBT aligned words
            uint32_t raw[NBT];
#pragma unroll
            for (int i = 0; i < NBT; ++i) raw[i] = reinterpret_cast<const uint32_t *>(g + (uint64_t)p0 * nbytes)[i];
            cut4_rows_w<NBT>(raw, w);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int t = 0; t < NW; ++t) {
                    uint32_t v = 0;
                    if ((uint32_t)j < nact) {
#pragma unroll
                        for (int bb = 0; bb < (NBT - 4 * t < 4 ? NBT - 4 * t : 4); ++bb) v |= (uint32_t)g[(uint64_t)(p0 + j) * nbytes + 4 * t + bb] << (8 * bb);
                    }
                    w[t][j] = v;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pos = tile_start + p0 + j;
            const uint32_t pc = popc_row(w, j);
            if (windowed) {
                if ((uint32_t)j < nact) {
                    const uint32_t dpos = pos - bin0_start;
                    const uint32_t rel = big ? (dpos >= binlen ? 1u : 0u) : __umulhi(dpos, binv);
                    atomicAdd(&hist[(rel_base + rel) * (N + 1) + pc], 1u);
                }
            } else {
                hist_position((uint32_t)j < nact, pos, pc, N, binlen, bin0, bin0_start, rel_base, hist, bins, a.bin_off, lane, MAXB);
            }
        }
        if (nact) {
            const Hit100 h = hit100(tile_start + p0);
            if (want100 && h.first < nact) copy_row_w<NBT>(g + (uint64_t)(p0 + h.first) * nbytes, out100 + a.out100_off + (uint64_t)h.r100 * nbytes);
        }
        if (want_cs) vadd_rows(w);  // (rows beyond npos are zero — a partial tile's words are built that way: adding them is harmless)
    }
    win.finish();
}

// ---------------------------------------------------------------------------
// statistics of arbitrary row windows of a finished bitmap (genes, bins of any length): per window
// the histogram of row popcounts and, optionally, the per-genome column sums.  Not on the hot
// path: LDS atomics for the histogram, one ballot per genome bit and 64 rows for the columns.
// grid = (windows, pieces): piece p of a window takes its 256-row groups p, p + pieces, ...
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window_stats(uint32_t N, const uint8_t *__restrict__ rows, uint64_t nrows,
                                                      const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends,
                                                      unsigned long long *__restrict__ hist_out,
                                                      unsigned long long *__restrict__ cs_out) {
    extern __shared__ uint32_t wsm[];
    uint32_t *hist = wsm, *cs = wsm + (N + 1);
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t i = tid; i < 2 * N + 1; i += 256) wsm[i] = 0;
    __syncthreads();
    const uint32_t nbytes = (N + 7) / 8, ndbs = (N + 31) / 32;
    const uint64_t s = starts[blockIdx.x], e = min(ends[blockIdx.x], nrows);
    if (s < e) {
        for (uint64_t g0 = s + 256ull * blockIdx.y; g0 < e; g0 += 256ull * gridDim.y) {
            const uint64_t r = g0 + tid;
            const bool active = r < e;
            uint32_t popc = 0;
            for (uint32_t d = 0; d < ndbs; ++d) {
                const uint32_t nb = min(4u, nbytes - 4 * d);
                uint32_t wv = 0;
                if (active)
                    for (uint32_t bb = 0; bb < nb; ++bb) wv |= (uint32_t)rows[r * nbytes + 4 * d + bb] << (8 * bb);
                popc += __popc(wv);
                if (cs_out) colsum_word(wv, d, N, cs, lane);
            }
            if (active) atomicAdd(&hist[min(popc, N)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i <= N; i += 256)
        if (hist[i]) atomicAdd(&hist_out[(uint64_t)blockIdx.x * (N + 1) + i], (unsigned long long)hist[i]);
    if (cs_out)
        for (uint32_t i = tid; i < N; i += 256)
            if (cs[i]) atomicAdd(&cs_out[(uint64_t)blockIdx.x * N + i], (unsigned long long)cs[i]);
}

// ---------------------------------------------------------------------------
// genome-sharded exchange (tables too big for one GPU): a rank's partial rows hold only the bits of
// the genomes it owns, so what crosses xGMI is a COMPACT block of bit columns — for every 64
// positions, one u64 per owned genome (bit l = position l) — all-gathered over RCCL and merged back
// into full rows: (n-1)/n row bytes received per position instead of the 2(n-1)/n of an all-reduce.
// Layout: tile t (PROBE_TILE positions) owns TILE_SLOTS = PROBE_TILE / 64 slots of `width` u64 words: word
// (TILE_SLOTS t + s) * width + j = genome g0 + j at positions 64 s .. 64 s + 63 of the tile.
// ---------------------------------------------------------------------------
// One-byte rows (a block of up to 8 genomes — config 5: ONE genome per GPU): a lane takes 16 consecutive positions (one
// aligned 16-byte load, the wave a whole tile) and gathers bit g of 8 row bytes into one byte with a multiply — two bytes per
// genome and lane: bytes 2 (lane % 4), 2 (lane % 4) + 1 of word (slot = lane / 4, genome j), one 16-bit store.  A wave takes
// COLS_TPW tiles, all of their loads in flight together.  (Rounds 2-4: a wave per 512 positions, 8 per lane — 4.7 x 10^7 waves
// of one load and one byte store each for config 5's 2.4 x 10^10 positions: 15 ms per pass at 1.6 TB/s, the launch's waves,
// not its bytes.)
constexpr uint32_t COLS_TPW = 4;  // tiles per wave of the one-byte-row column kernels
static_assert(PROBE_TILE == 1024, "k_cols_extract_b1 / k_cols_merge_b1: a wave's 64 lanes x 16 positions are one tile");
__global__ __launch_bounds__(256) void k_cols_extract_b1(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                         const uint32_t *__restrict__ tile_contig, uint32_t tile_base,
                                                         uint32_t ntiles, const uint8_t *__restrict__ out1, uint32_t g0,
                                                         uint32_t width, uint8_t *__restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * COLS_TPW;
    if (t0 >= ntiles) return;  // wave-uniform
    uint4 v[COLS_TPW];
    uint32_t valid[COLS_TPW];
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        v[k] = make_uint4(0, 0, 0, 0);
        valid[k] = 0;
        if (t0 + k < ntiles) {  // (wave-uniform)
            const uint32_t tile = tile_base + t0 + k;
            const AnchorDesc a = ad[tile_contig[tile]];
            const uint32_t p0 = (tile - a.tile0) * PROBE_TILE + 16 * lane;
            if (p0 < a.nkmers) {  // (rows are padded to 16 bytes per contig: the aligned 16-byte load stays inside)
                v[k] = *reinterpret_cast<const uint4 *>(out1 + a.out_off + p0);
                valid[k] = min(16u, a.nkmers - p0);
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        if (t0 + k >= ntiles) break;  // (wave-uniform)
        uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {  // bytes of positions past the contig's end hold whatever follows: cleared
            const uint32_t nv = valid[k] > 4 * i ? min(4u, valid[k] - 4 * i) : 0u;
            w[i] &= nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
        }
        uint8_t *o = dst + ((uint64_t)(t0 + k) * TILE_SLOTS + (lane >> 2)) * width * 8 + 2 * (lane & 3);
        for (uint32_t j = 0; j < width; ++j) {
            const uint32_t g = g0 + j;
            uint32_t b = 0;
            if (g < N) {  // bit g of rows 0..3 / 4..7 -> bits 0..3 / 4..7 (0x01020408: the four bits meet in bits 24..27)
                const uint32_t a0 = ((w[0] >> g) & 0x01010101u) * 0x01020408u, a1 = ((w[1] >> g) & 0x01010101u) * 0x01020408u;
                const uint32_t a2 = ((w[2] >> g) & 0x01010101u) * 0x01020408u, a3 = ((w[3] >> g) & 0x01010101u) * 0x01020408u;
                b = ((a0 >> 24) & 0xFu) | ((a1 >> 20) & 0xF0u) | ((a2 >> 16) & 0xF00u) | ((a3 >> 12) & 0xF000u);
            }
            *reinterpret_cast<uint16_t *>(o + 8 * j) = (uint16_t)b;
        }
    }
}

// the reverse for one-byte rows (N <= 8): a lane rebuilds the rows of 16 consecutive positions — its two bytes of each genome's
// word spread over 16 row bytes — and stores (or ORs) them as one aligned 16-byte word; COLS_TPW tiles per wave, their loads
// (the genomes' bytes and, when accumulating, the rows as they are) in flight together
__global__ __launch_bounds__(256) void k_cols_merge_b1(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                       const uint32_t *__restrict__ tile_contig, uint32_t tile_base,
                                                       uint32_t ntiles, uint8_t *__restrict__ out1,
                                                       const uint8_t *__restrict__ src, uint32_t part0, uint32_t nparts,
                                                       uint64_t part_bytes, uint32_t per, uint32_t accumulate) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * COLS_TPW;
    if (t0 >= ntiles) return;  // wave-uniform
    const uint32_t gfirst = part0 * per, gend = min(N, (part0 + nparts) * per);
    uint4 old[COLS_TPW];
    uint4 *rowp[COLS_TPW];
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        old[k] = make_uint4(0, 0, 0, 0);
        rowp[k] = nullptr;
        if (t0 + k < ntiles) {  // (wave-uniform)
            const uint32_t tile = tile_base + t0 + k;
            const AnchorDesc a = ad[tile_contig[tile]];
            const uint32_t p0 = (tile - a.tile0) * PROBE_TILE + 16 * lane;
            if (p0 < a.nkmers) {
                rowp[k] = reinterpret_cast<uint4 *>(out1 + a.out_off + p0);
                if (accumulate) old[k] = *rowp[k];
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        if (t0 + k >= ntiles) break;  // (wave-uniform)
        const uint8_t *in = src + ((uint64_t)(t0 + k) * TILE_SLOTS + (lane >> 2)) * per * 8 + 2 * (lane & 3);
        uint32_t w[4] = {old[k].x, old[k].y, old[k].z, old[k].w};
        for (uint32_t g = gfirst; g < gend; ++g) {
            const uint32_t part = g / per - part0, j = g % per;
            const uint32_t b2 = *reinterpret_cast<const uint16_t *>(in + (uint64_t)part * part_bytes + 8 * j);
            const uint32_t r0 = (b2 & 0xFFu) * 0x01010101u, r1 = (b2 >> 8) * 0x01010101u;  // bit i of a byte -> bit 0 of byte i
            w[0] |= ((((r0 & 0x08040201u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
            w[1] |= ((((r0 & 0x80402010u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
            w[2] |= ((((r1 & 0x08040201u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
            w[3] |= ((((r1 & 0x80402010u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
        }
        if (rowp[k]) *rowp[k] = make_uint4(w[0], w[1], w[2], w[3]);  // (bits of positions past nkmers are zero in the blocks: the padding stays zero)
    }
}

// Wider rows.  A lane owns one position; the wave one slot of 64.  The row bytes are read a 32-bit word at a time (one
// access per 32 genomes: the first version read a byte per genome in a loop that waited for each load in turn — 20 ps
// per row at 32 genomes per block, ten times the probe), a ballot per genome turns the word's bit into the slot's u64,
// kept by lane j and stored coalesced.
__global__ __launch_bounds__(256) void k_cols_extract(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                      const uint32_t *__restrict__ tile_contig, uint32_t tile_base,
                                                      uint32_t ntiles, const uint8_t *__restrict__ out1, uint32_t g0,
                                                      uint32_t width, unsigned long long *__restrict__ dst) {
    struct __attribute__((packed)) U32 { uint32_t v; };
    const int lane = threadIdx.x & 63;
    const uint64_t slot = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // relative to the range's first tile
    if (slot >= (uint64_t)ntiles * TILE_SLOTS) return;  // wave-uniform
    const uint32_t tile = tile_base + (uint32_t)(slot / TILE_SLOTS), sub = (uint32_t)(slot % TILE_SLOTS);
    const AnchorDesc a = ad[tile_contig[tile]];
    const uint32_t nbytes = (N + 7) / 8;
    const uint32_t p = (tile - a.tile0) * PROBE_TILE + sub * 64 + lane;
    const bool active = p < a.nkmers;
    const uint8_t *row = out1 + a.out_off + (uint64_t)p * nbytes;
    const uint32_t gend = min(N, g0 + width);
    for (uint32_t j0 = 0; j0 < width; j0 += 64) {
        unsigned long long mine = 0;
        const uint32_t ga = g0 + j0, gz = min(gend, ga + 64u);  // genomes of this group of (up to) 64 columns
        for (uint32_t wd = ga >> 5; 32u * wd < gz; ++wd) {
            uint32_t v = 0;
            if (active) {  // (the word may reach past the row's last byte: byte loads there)
                if (4u * wd + 4u <= nbytes) v = reinterpret_cast<const U32 *>(row + 4u * wd)->v;
                else
                    for (uint32_t bb = 0; 4u * wd + bb < nbytes; ++bb) v |= (uint32_t)row[4u * wd + bb] << (8u * bb);
            }
            const uint32_t b_lo = max(ga, 32u * wd) - 32u * wd, b_hi = min(gz, 32u * wd + 32u) - 32u * wd;
            for (uint32_t b = b_lo; b < b_hi; ++b) {
                const unsigned long long m = __ballot((v >> b) & 1u);
                if ((uint32_t)lane == 32u * wd + b - ga) mine = m;
            }
        }
        if ((uint32_t)lane < min(64u, width - j0)) dst[slot * width + j0 + lane] = mine;  // (columns past N stay zero)
    }
}

// src = nparts blocks of part_words u64 each (block i = genomes (part0 + i) * per ...); the bits of those genomes are
// set in the rows from the blocks.  accumulate == 0: the rows are written whole (bits of genomes outside the
// blocks become 0); != 0: the blocks' bits are OR-ed into what the rows hold (genome blocks arriving pass by pass).
// The u64 of a genome and slot is the same for the whole wave: lane l FETCHES the one of genome 32 d + l (one coalesced
// access per 32 genomes) and the wave reads them lane by lane — as wave-uniform loads inside the genome loop every one
// of them was waited for in turn (0.4-0.7 ms per call at 64 genomes).
__global__ __launch_bounds__(256) void k_cols_merge(uint32_t N, const AnchorDesc *__restrict__ ad,
                                                    const uint32_t *__restrict__ tile_contig, uint32_t tile_base,
                                                    uint32_t ntiles, uint8_t *__restrict__ out1,
                                                    const unsigned long long *__restrict__ src, uint32_t part0,
                                                    uint32_t nparts, uint64_t part_words, uint32_t per, uint32_t accumulate) {
    const int lane = threadIdx.x & 63;
    const uint64_t slot = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= (uint64_t)ntiles * TILE_SLOTS) return;
    const uint32_t tile = tile_base + (uint32_t)(slot / TILE_SLOTS), sub = (uint32_t)(slot % TILE_SLOTS);
    const AnchorDesc a = ad[tile_contig[tile]];
    const uint32_t nbytes = (N + 7) / 8, ndbs = (N + 31) / 32;
    const uint32_t p = (tile - a.tile0) * PROBE_TILE + sub * 64 + lane;
    uint8_t *row = out1 + a.out_off + (uint64_t)p * nbytes;
    const uint32_t gfirst = part0 * per, gend = min(N, (part0 + nparts) * per);  // genomes the blocks cover
    for (uint32_t d = 0; d < ndbs; ++d) {
        if (accumulate && (32 * d + 32 <= gfirst || 32 * d >= gend)) continue;  // (uniform) word untouched by these blocks
        const uint32_t gl = 32u * d + ((uint32_t)lane & 31u);
        unsigned long long mine = 0;
        if (lane < 32 && gl >= gfirst && gl < gend) mine = src[(uint64_t)(gl / per - part0) * part_words + slot * per + gl % per];
        uint32_t w = 0;
        // bits of this word that the blocks cover (none: the word is written as zeros)
        const bool any = 32u * d < gend && 32u * d + 32u > gfirst;
        const uint32_t b_lo = any ? max(gfirst, 32u * d) - 32u * d : 0u, b_hi = any ? min(gend, 32u * d + 32u) - 32u * d : 0u;
        for (uint32_t b = b_lo; b < b_hi; ++b) {  // (uniform)
            const unsigned long long word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), (int)b) << 32) |
                                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, (int)b);
            w |= (__builtin_amdgcn_inverse_ballot_w64(word) ? 1u : 0u) << b;
        }
        if (p < a.nkmers) {
            const uint32_t n = min(4u, nbytes - 4 * d);
            if (n == 4 && (nbytes & 3u) == 0) {  // (uniform) whole words of rows that start on word boundaries: one access, not four
                uint32_t *rw = reinterpret_cast<uint32_t *>(row + 4 * d);
                if (!accumulate) *rw = w;
                else if (w) *rw |= w;
            } else if (accumulate) {
                for (uint32_t bb = 0; bb < n; ++bb) {
                    const uint8_t add = (uint8_t)(w >> (8 * bb));
                    if (add) row[4 * d + bb] |= add;
                }
            } else {
                for (uint32_t bb = 0; bb < n; ++bb) row[4 * d + bb] = (uint8_t)(w >> (8 * bb));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// append (no reference counterpart: the reference re-runs its whole workflow to add a genome): the finished rows of n_old
// genomes of ONE result plus column blocks of further genomes (the layout above: what the probe of a narrow table or
// k_cols_extract* writes) -> the rows of n_new genomes of ANOTHER result over contigs of the same lengths.  Every
// destination row is written whole, once: bits below n_old copied, bits n_old .. n_new - 1 from the blocks (genome j of
// block i is bit n_old + i * per + j), the rest zero; the bits at and past n_old of the source's last byte are dropped
// (the source comes from a file).  Composed of what was there before — k_cols_extract of all old genomes, k_cols_merge,
// k_cols_merge(accumulate) — every row is read and written more than twice, and a column copy of the whole bitmap is
// needed; here W_old + W_new + m / 8 bytes move per position.
// The source's tiles 0 .. ntiles - 1 are the destination's from contig dst_c0 on (same nkmers, contig by contig: the
// host checks it), the blocks are indexed by the source's tiles.
// ---------------------------------------------------------------------------
struct AppendArgs {
    const AnchorDesc *sad;          // the source's contigs, tiles and rows
    const uint32_t *stile_contig;
    const uint8_t *src;
    const AnchorDesc *dad;          // the destination's contigs and rows
    uint8_t *dst;
    const unsigned long long *cols;
    uint64_t part_words;            // distance between two blocks
    uint32_t ntiles, dst_c0, nparts, per, n_old, n_new;
};

// One-byte rows on both sides (n_new <= 8), after k_cols_merge_b1: 16 positions per lane, one aligned 16-byte load and
// store, COLS_TPW tiles per wave.  The up to 7 new genomes' two bytes are all asked for before the first one is used (in
// a loop over the genomes every load would be waited for in turn), beside the tiles' old rows.
__global__ __launch_bounds__(256) void k_rows_append_b1(AppendArgs A) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * COLS_TPW;
    if (t0 >= A.ntiles) return;  // wave-uniform
    const uint32_t m = A.n_new - A.n_old;  // (<= 8)
    uint4 old[COLS_TPW];
    uint4 *rowp[COLS_TPW];
    uint32_t valid[COLS_TPW], b2[COLS_TPW][8];
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        old[k] = make_uint4(0, 0, 0, 0);
        rowp[k] = nullptr;
        valid[k] = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) b2[k][q] = 0;
        if (t0 + k < A.ntiles) {  // (wave-uniform)
            const uint32_t tile = t0 + k, c = A.stile_contig[tile];
            const AnchorDesc sa = A.sad[c];
            const uint32_t p0 = (tile - sa.tile0) * PROBE_TILE + 16 * lane;
            if (p0 < sa.nkmers) {  // (rows are padded to 16 bytes per contig on both sides: the aligned 16-byte accesses stay inside)
                old[k] = *reinterpret_cast<const uint4 *>(A.src + sa.out_off + p0);
                rowp[k] = reinterpret_cast<uint4 *>(A.dst + A.dad[A.dst_c0 + c].out_off + p0);
                valid[k] = min(16u, sa.nkmers - p0);
                const uint8_t *in = reinterpret_cast<const uint8_t *>(A.cols) + ((uint64_t)tile * TILE_SLOTS + (lane >> 2)) * A.per * 8 + 2 * (lane & 3);
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q)
                    if (q < m) b2[k][q] = *reinterpret_cast<const uint16_t *>(in + (uint64_t)(q / A.per) * A.part_words * 8 + 8 * (q % A.per));
            }
        }
    }
    const uint32_t keep = ((1u << A.n_old) - 1u) * 0x01010101u;  // the old genomes' bits of four rows
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        if (!rowp[k]) continue;
        uint32_t w[4] = {old[k].x & keep, old[k].y & keep, old[k].z & keep, old[k].w & keep};
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            if (q >= m) break;  // (uniform)
            const uint32_t g = A.n_old + q;
            const uint32_t r0 = (b2[k][q] & 0xFFu) * 0x01010101u, r1 = (b2[k][q] >> 8) * 0x01010101u;  // bit i of a byte -> bit 0 of byte i
            w[0] |= ((((r0 & 0x08040201u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
            w[1] |= ((((r0 & 0x80402010u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
            w[2] |= ((((r1 & 0x08040201u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
            w[3] |= ((((r1 & 0x80402010u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u) << g;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {  // positions past the contig's end: the destination's padding stays zero whatever the source's and the blocks hold there
            const uint32_t nv = valid[k] > 4 * i ? min(4u, valid[k] - 4 * i) : 0u;
            w[i] &= nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
        }
        *rowp[k] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Every other pair of widths.  A lane owns one position, the wave one slot of 64 — the 64 W_old and 64 W_new bytes of a
// slot are each one contiguous span that starts on a 16-byte boundary (a contig's rows do; 64 W bytes per slot), and the wave covers it with ceil(W / 4) accesses of
// one 32-bit word per lane at a stride of W bytes: rows that start off word boundaries (odd widths) are read and written
// with unaligned words, which global memory serves, the span's cache lines being shared by the wave's few instructions
// back to back (k_cols_extract reads its rows the same way).  A row's tail of 1..3 bytes is stored as a 16-bit word and /
// or a byte: the next row belongs to the next lane.  The last word read of a row may reach up to 3 bytes past it — into
// the next row, the contig's padding or the 16 bytes of slack behind the buffer — and is masked to the old genomes' bits.
// The new genomes' u64 of a slot are the same for the whole wave: lane l fetches the one of bit l of the row word at hand
// (one coalesced access per 32 genomes, as in k_cols_merge) and the wave reads them lane by lane.  NW = words per new row,
// SPW = slots of one tile per wave: all of their loads, old words and column words, are in flight before the first is used;
// NW = 0: any width, word by word.  (One slot per wave — 1.6 million waves for 10^8 positions, each one waiting for its
// tile's contig number, then the contig's descriptor, then its rows — took 0.42 / 0.49 / 0.63 ms at 8 -> 9 / 16 -> 17 /
// 64 -> 65 genomes whatever the bytes: 9 to 34 % of the byte floor; profiles/add_rate.txt.)
struct __attribute__((packed)) U16 { uint16_t v; };
template <int NW, int SPW>
__global__ __launch_bounds__(256) void k_rows_append(AppendArgs A) {
    static_assert(TILE_SLOTS % SPW == 0, "a wave's slots lie in one tile");
    constexpr uint32_t WPT = TILE_SLOTS / SPW;  // waves per tile
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (uint64_t)A.ntiles * WPT) return;  // wave-uniform
    const uint32_t tile = (uint32_t)(wave / WPT), sub0 = (uint32_t)(wave % WPT) * SPW;
    const uint32_t c = A.stile_contig[tile];
    const AnchorDesc sa = A.sad[c];
    const uint32_t n_old = A.n_old, n_new = A.n_new, wo = (n_old + 7) / 8, wn = (n_new + 7) / 8;
    const uint32_t p0 = (tile - sa.tile0) * PROBE_TILE + sub0 * 64 + lane;  // this lane's position in the wave's first slot
    const uint64_t slot0 = (uint64_t)tile * TILE_SLOTS + sub0;
    const uint8_t *sbase = A.src + sa.out_off;
    uint8_t *dbase = A.dst + A.dad[A.dst_c0 + c].out_off;
    auto load_old = [&](uint32_t s, uint32_t d) -> uint32_t {  // word d of the old row of slot s
        const uint32_t p = p0 + 64u * s;
        return (p < sa.nkmers && 4u * d < wo) ? reinterpret_cast<const U32 *>(sbase + (uint64_t)p * wo + 4u * d)->v : 0u;
    };
    auto load_cols = [&](uint32_t s, uint32_t d) -> unsigned long long {  // lane l: slot s's u64 of genome 32 d + l, if it is a new one
        const uint32_t gl = 32u * d + ((uint32_t)lane & 31u);
        if (lane >= 32 || gl < n_old || gl >= n_new) return 0ull;
        const uint32_t q = gl - n_old;
        return A.cols[(uint64_t)(q / A.per) * A.part_words + (slot0 + s) * A.per + q % A.per];
    };
    auto store_word = [&](uint32_t s, uint32_t d, uint32_t oldw, unsigned long long mine) {
        const uint32_t lo = 32u * d;
        const uint32_t vb = n_old > lo ? min(32u, n_old - lo) : 0u;  // bits of this word that are old genomes'
        uint32_t w = oldw & (vb >= 32u ? 0xFFFFFFFFu : (1u << vb) - 1u);
        const uint32_t b_lo = vb, b_hi = n_new > lo ? min(32u, n_new - lo) : 0u;
        for (uint32_t b = b_lo; b < b_hi; ++b) {  // (uniform)
            const unsigned long long word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), (int)b) << 32) |
                                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, (int)b);
            w |= (__builtin_amdgcn_inverse_ballot_w64(word) ? 1u : 0u) << b;
        }
        const uint32_t p = p0 + 64u * s;
        if (p >= sa.nkmers) return;
        uint8_t *o = dbase + (uint64_t)p * wn + 4u * d;
        const uint32_t n = min(4u, wn - 4u * d);  // (uniform)
        if (n == 4) {
            reinterpret_cast<U32 *>(o)->v = w;
        } else {
            if (n >= 2) reinterpret_cast<U16 *>(o)->v = (uint16_t)w;
            if (n & 1) o[n - 1] = (uint8_t)(w >> (8 * (n - 1)));
        }
    };
    if constexpr (NW > 0) {
        uint32_t oldw[SPW][NW];
        unsigned long long mine[SPW][NW];
#pragma unroll
        for (int s = 0; s < SPW; ++s)
#pragma unroll
            for (int d = 0; d < NW; ++d) {
                oldw[s][d] = load_old(s, d);
                mine[s][d] = load_cols(s, d);
            }
#pragma unroll
        for (int s = 0; s < SPW; ++s)
#pragma unroll
            for (int d = 0; d < NW; ++d) store_word(s, d, oldw[s][d], mine[s][d]);
    } else {
        for (uint32_t s = 0; s < (uint32_t)SPW; ++s)
            for (uint32_t d = 0; 4u * d < wn; ++d) store_word(s, d, load_old(s, d), load_cols(s, d));
    }
}

// ---------------------------------------------------------------------------
// select (no reference counterpart: to drop or reorder samples the reference re-runs its whole workflow): the finished rows
// of n_old genomes of ONE result -> the rows of n_new genomes of ANOTHER result over contigs of the same lengths,
// destination bit j being source bit sel[j] (distinct, any order: columns dropped, permuted or both).  Every destination
// row is written whole, once, every source row read once; the bits at and past n_new are zero, the bits at and past n_old
// of the source's last byte are never looked at (the source comes from a file), and the destination's padding is not
// touched.  Composed of what was there before — one k_cols_extract per kept genome, then k_cols_merge — the rows are read
// n_new times and a column copy of the whole bitmap is needed; here W_old + W_new bytes move per position.
// The host compiles sel into segments (pg_select_host.h): runs of consecutive source bits that go to consecutive
// destination bits, each inside one destination word and so inside two neighbouring source words.  They are the same for
// every wave: read through the scalar cache, in a uniform loop whose length is the number of segments, not of genomes.
// Geometry as in k_rows_append*: the source's tiles 0 .. ntiles - 1 are the destination's from contig dst_c0 on.
// ---------------------------------------------------------------------------
struct SelectArgs {
    const AnchorDesc *sad;          // the source's contigs, tiles and rows
    const uint32_t *stile_contig;
    const uint8_t *src;
    const AnchorDesc *dad;          // the destination's contigs and rows
    uint8_t *dst;
    const SelSeg *segs;             // in the order of their destination bits
    uint32_t nseg, need;            // need: bit d = some segment reads source word d
    uint32_t ntiles, dst_c0, n_old, n_new;
};

// One-byte rows on both sides (n_old <= 8), after k_rows_append_b1: 16 positions per lane, one aligned 16-byte load and
// store, COLS_TPW tiles per wave.  A segment moves its bits of four rows at once: no bit leaves its byte, the mask cuts
// off what the right shift brings in from the next row.
__global__ __launch_bounds__(256) void k_rows_select_b1(SelectArgs A) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * COLS_TPW;
    if (t0 >= A.ntiles) return;  // wave-uniform
    uint4 old[COLS_TPW];
    uint4 *rowp[COLS_TPW];
    uint32_t valid[COLS_TPW];
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        old[k] = make_uint4(0, 0, 0, 0);
        rowp[k] = nullptr;
        valid[k] = 0;
        if (t0 + k < A.ntiles) {  // (wave-uniform)
            const uint32_t tile = t0 + k, c = A.stile_contig[tile];
            const AnchorDesc sa = A.sad[c];
            const uint32_t p0 = (tile - sa.tile0) * PROBE_TILE + 16 * lane;
            if (p0 < sa.nkmers) {  // (rows are padded to 16 bytes per contig on both sides: the aligned 16-byte accesses stay inside)
                old[k] = *reinterpret_cast<const uint4 *>(A.src + sa.out_off + p0);
                rowp[k] = reinterpret_cast<uint4 *>(A.dst + A.dad[A.dst_c0 + c].out_off + p0);
                valid[k] = min(16u, sa.nkmers - p0);
            }
        }
    }
    uint32_t w[COLS_TPW][4];
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k)
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) w[k][i] = 0;
    for (uint32_t i = 0; i < A.nseg; ++i) {  // (uniform: at most 8)
        const SelSeg g = A.segs[i];
        const uint32_t sh = g.shifts & 0xFFu, dsh = (g.shifts >> 8) & 0xFFu, m = g.mask * 0x01010101u;
#pragma unroll
        for (uint32_t k = 0; k < COLS_TPW; ++k) {
            w[k][0] |= ((old[k].x >> sh) & m) << dsh;
            w[k][1] |= ((old[k].y >> sh) & m) << dsh;
            w[k][2] |= ((old[k].z >> sh) & m) << dsh;
            w[k][3] |= ((old[k].w >> sh) & m) << dsh;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < COLS_TPW; ++k) {
        if (!rowp[k]) continue;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {  // positions past the contig's end: the destination's padding stays zero whatever the source's holds
            const uint32_t nv = valid[k] > 4 * i ? min(4u, valid[k] - 4 * i) : 0u;
            w[k][i] &= nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
        }
        *rowp[k] = make_uint4(w[k][0], w[k][1], w[k][2], w[k][3]);
    }
}

// Every other pair of widths, with k_rows_append's geometry: a lane owns one position, a wave SPW slots of 64 positions of
// one tile, rows are read and written as (unaligned) 32-bit words at a stride of the row width, a row's tail of 1..3 bytes
// is stored as a 16-bit word and / or a byte (the next row is the next lane's), and the last word read of a row may reach
// up to 3 bytes past it, into the next row, the contig's padding or the slack behind the buffer: no segment looks there.
// NWS = words per source row: the wave asks for every source word that some segment reads (A.need: 64 -> 8 genomes fetches
// one word of a row's two) of all its slots before it uses the first; the segment loop then picks its one or two words out
// of the registers by the segment's (uniform) word number.  NWS = 0: any width, the words fetched as the segments ask.
template <int NWS, int SPW>
__global__ __launch_bounds__(256) void k_rows_select(SelectArgs A) {
    static_assert(TILE_SLOTS % SPW == 0, "a wave's slots lie in one tile");
    constexpr uint32_t WPT = TILE_SLOTS / SPW;  // waves per tile
    constexpr int NR = NWS > 0 ? NWS : 1;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (uint64_t)A.ntiles * WPT) return;  // wave-uniform
    const uint32_t tile = (uint32_t)(wave / WPT), sub0 = (uint32_t)(wave % WPT) * SPW;
    const uint32_t c = A.stile_contig[tile];
    const AnchorDesc sa = A.sad[c];
    const uint32_t wo = (A.n_old + 7) / 8, wn = (A.n_new + 7) / 8;
    const uint32_t p0 = (tile - sa.tile0) * PROBE_TILE + sub0 * 64 + lane;  // this lane's position in the wave's first slot
    const uint8_t *sbase = A.src + sa.out_off;
    uint8_t *dbase = A.dst + A.dad[A.dst_c0 + c].out_off;
    auto load_old = [&](uint32_t s, uint32_t d) -> uint32_t {  // word d of the source row of slot s
        const uint32_t p = p0 + 64u * s;
        return (p < sa.nkmers && 4u * d < wo) ? reinterpret_cast<const U32 *>(sbase + (uint64_t)p * wo + 4u * d)->v : 0u;
    };
    auto store_word = [&](uint32_t s, uint32_t d, uint32_t w) {
        const uint32_t p = p0 + 64u * s;
        if (p >= sa.nkmers) return;
        uint8_t *o = dbase + (uint64_t)p * wn + 4u * d;
        const uint32_t n = min(4u, wn - 4u * d);  // (uniform)
        if (n == 4) {
            reinterpret_cast<U32 *>(o)->v = w;
        } else {
            if (n >= 2) reinterpret_cast<U16 *>(o)->v = (uint16_t)w;
            if (n & 1) o[n - 1] = (uint8_t)(w >> (8 * (n - 1)));
        }
    };
    uint32_t oldw[SPW][NR];
    if constexpr (NWS > 0) {
#pragma unroll
        for (int s = 0; s < SPW; ++s)
#pragma unroll
            for (int d = 0; d < NWS; ++d) oldw[s][d] = ((A.need >> d) & 1u) ? load_old(s, d) : 0u;  // (uniform)
    }
    // NWS = 0: the two source words fetched last (numbers ia < ib; the next segment of a selection that keeps its order wants
    // ib again, with ib + 1: each word is then fetched once)
    uint32_t ca[SPW], cb[SPW], ia = 0xFFFFFFFFu, ib = 0xFFFFFFFFu;
    auto fetch = [&](uint32_t lo, uint32_t two) {  // (uniform)
        if ((lo == ia || lo == ib) && (!two || lo + 1 == ib)) return;
        if (two && ib != lo) {
            ia = lo;
#pragma unroll
            for (int s = 0; s < SPW; ++s) ca[s] = load_old(s, lo);
        } else {  // what was fetched last stays
            ia = ib;
#pragma unroll
            for (int s = 0; s < SPW; ++s) ca[s] = cb[s];
        }
        ib = lo + two;
#pragma unroll
        for (int s = 0; s < SPW; ++s) cb[s] = load_old(s, ib);
    };
    auto word = [&](uint32_t s, uint32_t j) -> uint32_t {  // source word j (uniform) of slot s
        if constexpr (NWS > 0) {
            uint32_t r = 0;
#pragma unroll
            for (int d = 0; d < NWS; ++d) r = j == (uint32_t)d ? oldw[s][d] : r;
            return r;
        } else {
            return j == ia ? ca[s] : cb[s];
        }
    };
    uint32_t i = 0;
    for (uint32_t d = 0; 4u * d < wn; ++d) {  // (uniform, as is the loop inside: every destination word has a segment)
        uint32_t w[SPW];
#pragma unroll
        for (int s = 0; s < SPW; ++s) w[s] = 0;
        for (; i < A.nseg; ++i) {
            const SelSeg g = A.segs[i];
            if ((g.words >> 16) != d) break;
            const uint32_t sw = g.words & 0xFFFFu, sh = g.shifts & 0xFFu, dsh = (g.shifts >> 8) & 0xFFu, two = (g.shifts >> 16) & 1u;
            if constexpr (NWS == 0) fetch(sw, two);
#pragma unroll
            for (int s = 0; s < SPW; ++s) {
                const uint32_t lo = word(s, sw), hi = two ? word(s, sw + 1) : 0u;
                w[s] |= ((uint32_t)((((unsigned long long)hi << 32) | lo) >> sh) & g.mask) << dsh;
            }
        }
#pragma unroll
        for (int s = 0; s < SPW; ++s) store_word(s, d, w[s]);
    }
}

// every step-th row of bitmap.1 -> the low-resolution bitmap, for steps other than the 100 the statistics
// kernels fuse (index.py:101-106 lowres_step): one wave per tile, a handful of rows each
__global__ __launch_bounds__(64) void k_lowres(uint32_t N, const AnchorDesc *__restrict__ ad,
                                               const uint32_t *__restrict__ tile_contig, const uint8_t *__restrict__ out1,
                                               uint8_t *__restrict__ outlow, uint32_t step) {
    const uint32_t tile = blockIdx.x;
    const AnchorDesc a = ad[tile_contig[tile]];
    const uint32_t nbytes = (N + 7) / 8;
    const uint32_t ts = (tile - a.tile0) * PROBE_TILE, te = min(a.nkmers, ts + (uint32_t)PROBE_TILE);
    const uint64_t r0 = ((uint64_t)ts + step - 1) / step;
    for (uint64_t r = r0 + threadIdx.x; r * step < te; r += 64) {
        const uint8_t *src = out1 + a.out_off + r * step * nbytes;
        uint8_t *dst = outlow + a.out100_off + r * nbytes;
        for (uint32_t bb = 0; bb < nbytes; ++bb) dst[bb] = src[bb];
    }
}

hipError_t launch_rows_epilogue(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                                uint32_t ntiles, const uint8_t *out1, uint8_t *out100, uint32_t *bins,
                                unsigned long long *colsums, uint32_t flags, const uint2 *d_ranges, uint32_t nranges,
                                uint32_t range_tiles) {
    // d_ranges: the launch covers these nranges tile ranges (range_tiles tiles in all) instead of [0, ntiles)
    if (ntiles == 0 || (d_ranges && (nranges == 0 || range_tiles == 0))) return hipSuccess;
    const uint32_t work_tiles = d_ranges ? range_tiles : ntiles;
    const uint32_t maxb = epi_maxb_for(ngenomes);
    flags = (flags & 0xFFFF00FFu) | (maxb << 8);
    size_t lds = (((maxb * (ngenomes + 1) + 3) & ~3u) + ((ngenomes + 3) & ~3u)) * 4 + 16;
    // contiguous tile ranges per workgroup: enough workgroups to fill every CU, but no fewer than
    // a minimum number of tiles each so that the end-of-range reductions stay amortised
    const uint32_t maxg = 256u * (2048u / EPI_THREADS);
    // long ranges (PG_EPI_MIN_TILES tiles) keep the pass light beside a concurrent k_probe; but never
    // fewer than ~1024 workgroups (4 per CU) as long as each still gets 16 tiles, or small inputs
    // turn latency-bound
    uint32_t grid = (work_tiles + PG_EPI_MIN_TILES - 1) / PG_EPI_MIN_TILES;
    grid = std::max(grid, std::min(1024u, work_tiles / 16u));
    grid = grid < 1 ? 1 : (grid > maxg ? maxg : grid);
    uint32_t wpr = 0;
    auto per_range = [&]() {  // (ranges: the same number of workgroups for each, the grid a multiple of the range count)
        if (!d_ranges) return;
        wpr = std::max(1u, grid / nranges);
        grid = wpr * nranges;
    };
    // persistent workgroups: no more of them than the device holds at once (a second, partly filled round of
    // workgroups would leave CUs idle at the end: 8192 waves over 5120 slots cost the one-byte kernel 20 %)
    auto fit = [&](const void *kern, size_t lds_bytes) {
        static std::mutex mu;
        static std::map<std::pair<const void *, size_t>, uint32_t> caps;  // (the query is a driver call: once per kernel and LDS size)
        std::lock_guard<std::mutex> lk(mu);
        auto it = caps.find({kern, lds_bytes});
        if (it == caps.end()) {
            int per_cu = 0, dev = 0, cus = 0;
            uint32_t cap = ~0u;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, EPI_THREADS, lds_bytes) == hipSuccess && per_cu >= 1 &&
                hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
                cap = (uint32_t)per_cu * (uint32_t)cus;
            it = caps.emplace(std::make_pair(kern, lds_bytes), cap).first;
        }
        if (grid > it->second) grid = it->second;
    };
    // A TEST SWITCH, PG_EPI_WORKGROUPS=n in the environment (read at every launch, so that one process can run both shapes): no
    // more than n >= 1 workgroups.  The formula above gives a workgroup about 16 tiles until a launch holds more than 16 384 of
    // them, so the kernels' flushes of the counter planes in the middle of a contig (60 tiles of one contig in one workgroup for
    // rows of 2..16 bytes, 30 for 17..32) need 6 x 10^7 rows in one launch; under a bound of 1 or 2 a contig of 1.4 x 10^5 rows
    // reaches them (tests/test_gpu_planes_flush.py, tests/epi_walk.py).  Unset or empty: the shape above, untouched.  With tile
    // ranges every range still gets max(1, grid / nranges) workgroups.
    auto bound = [&]() {
        const char *e = getenv("PG_EPI_WORKGROUPS");
        if (!e || !*e) return;
        const unsigned long long v = strtoull(e, nullptr, 10);
        grid = std::min(grid, (uint32_t)std::min<unsigned long long>(std::max(v, 1ull), maxg));
    };
    auto launch = [&](decltype(&k_epilogue_b1) kern, size_t lds_bytes) {
        fit(reinterpret_cast<const void *>(kern), lds_bytes);
        bound();
        per_range();
        hipLaunchKernelGGL(kern, dim3(grid), dim3(EPI_THREADS), lds_bytes, st, ngenomes, ad, tile_contig, ntiles, out1, out100, bins,
                           colsums, flags, d_ranges, wpr);
    };
    const uint32_t nbytes = (ngenomes + 7) / 8;
    if (nbytes <= 8) {
        auto kern = k_epilogue_b1;
        switch (nbytes) {
            case 2: kern = k_epilogue_n<2>; break;
            case 3: kern = k_epilogue_n<3>; break;
            case 4: kern = k_epilogue_n<4>; break;
            case 5: kern = k_epilogue_n<5>; break;
            case 6: kern = k_epilogue_n<6>; break;
            case 7: kern = k_epilogue_n<7>; break;
            case 8: kern = k_epilogue_n<8>; break;
            default: break;
        }
        launch(kern, lds);
    }
    else if (nbytes <= 16) {  // 65..128 genomes: 16 rows per thread, three or four words per row
        auto kern = k_epilogue_w<16>;
        switch (nbytes) {
            case 9: kern = k_epilogue_w<9>; break;
            case 10: kern = k_epilogue_w<10>; break;
            case 11: kern = k_epilogue_w<11>; break;
            case 12: kern = k_epilogue_w<12>; break;
            case 13: kern = k_epilogue_w<13>; break;
            case 14: kern = k_epilogue_w<14>; break;
            case 15: kern = k_epilogue_w<15>; break;
            default: break;
        }
        launch(kern, lds);
    }
    else {  // more than 128 genomes, chunk-parallel: one launch, every row read once
        const uint32_t C = (nbytes + 15) / 16;  // (>= 2)
        if (C > 64) return hipErrorInvalidValue;
        const size_t lds_c = (((maxb * (ngenomes + 1) + 3) & ~3u) + ((64u / C + 15u) / 16u) * 128u * C) * 4 + 16;
        const bool exact = nbytes == 16u * C;
        auto kern = k_epilogue_chunks<0, false>;  // (compile-time C: the lanes-per-row shuffles and index arithmetic unroll)
        switch (C) {
            case 2: kern = exact ? k_epilogue_chunks<2, true> : k_epilogue_chunks<2, false>; break;
            case 3: kern = k_epilogue_chunks<3, false>; break;
            case 4: kern = exact ? k_epilogue_chunks<4, true> : k_epilogue_chunks<4, false>; break;
            default: break;
        }
        launch(kern, lds_c);
    }
    return hipGetLastError();
}

// The tiles' counters of a fused launch (FuseArgs) into the bins and the per-contig column sums.  A workgroup takes TR_TILES
// consecutive tiles; a thread owns an item — a histogram field (bin 0 / 1 of the tile, popcount) or a genome's column — adds its
// values up while the item's destination (the bin's row, the contig's row) stays the same, and flushes one atomic add when it
// changes: a bin of 200 000 rows is 195 tiles long.  Tiles of contigs whose bins are shorter than a tile carry no counters (the
// statistics pass did them).  Reads (4 (N + 1) + 64 ceil(nbytes / 4)) bytes per tile where the pass read 1024 rows.
constexpr uint32_t TR_TILES = 32;
__global__ __launch_bounds__(256) void k_tile_reduce(const FuseArgs fo, const AnchorDesc *__restrict__ ad, const uint32_t *__restrict__ tile_contig,
                                                     uint32_t ntiles, uint32_t *__restrict__ bins, unsigned long long *__restrict__ colsums,
                                                     uint32_t want_cs) {
    const uint32_t N = fo.ngenomes, N1 = N + 1u;
    const uint32_t nitems = 2u * N1 + (want_cs ? N : 0u);
    // a workgroup = as many groups of TR_TILES tiles as its threads hold items for (N = 12: 38 items, 6 groups per 256 threads)
    const uint32_t per = max(1u, blockDim.x / nitems), slot = threadIdx.x / nitems;
    const uint32_t it0 = nitems <= blockDim.x ? threadIdx.x - slot * nitems : threadIdx.x;
    const uint32_t grp = blockIdx.x * per + (nitems <= blockDim.x ? slot : 0u);
    if (nitems <= blockDim.x && slot >= per) return;
    const uint32_t t0 = grp * TR_TILES;
    if (t0 >= ntiles) return;
    const uint32_t t1 = min(ntiles, t0 + TR_TILES);
    for (uint32_t it = it0; it < nitems; it += blockDim.x) {
        const bool is_hist = it < 2u * N1;
        const uint32_t rel = is_hist ? it / N1 : 0u, pc = it - rel * N1, g = it - 2u * N1;
        // where the item's u16 sits in a tile's counters
        const uint32_t word = is_hist ? (it >> 1) : (g >> 5) * 16u + (g & 15u), shift = is_hist ? 16u * (it & 1u) : ((g & 16u) ? 16u : 0u);
        const uint32_t *src = (is_hist ? fo.tile_hist : fo.tile_cs) + word;
        const uint32_t stride = is_hist ? fo.hw : fo.csw;
        uint32_t v[TR_TILES];  // (every tile's word requested at once: the walk below is serial)
#pragma unroll
        for (uint32_t j = 0; j < TR_TILES; ++j) v[j] = src[(uint64_t)min(t0 + j, t1 - 1u) * stride];
        unsigned long long acc = 0, key = ~0ull;
        uint32_t cur_c = ~0u;
        AnchorDesc a;
        a.binlen = 0, a.tile0 = 0, a.bin_off = 0;
        auto flush = [&]() {
            if (acc) {
                if (is_hist) atomicAdd(&bins[key], (uint32_t)acc);
                else atomicAdd(&colsums[key], acc);
            }
            acc = 0;
        };
#pragma unroll
        for (uint32_t j = 0; j < TR_TILES; ++j) {
            const uint32_t t = t0 + j;
            if (t >= t1) break;
            const uint32_t c = tile_contig[t];
            if (c != cur_c) {
                cur_c = c;
                a = ad[c];
            }
            if (a.binlen < (uint32_t)PROBE_TILE) continue;  // (not fused: its counters were never written)
            const unsigned long long k2 = is_hist ? (a.bin_off + (uint64_t)(t - a.tile0) * PROBE_TILE / a.binlen + rel) * N1 + pc
                                                  : (unsigned long long)c * N + g;
            if (k2 != key) {
                flush();
                key = k2;
            }
            acc += (v[j] >> shift) & 0xFFFFu;
        }
        flush();
    }
}

hipError_t launch_tile_reduce(hipStream_t st, const FuseArgs &fo, const AnchorDesc *ad, const uint32_t *tile_contig, uint32_t ntiles,
                              uint32_t *bins, unsigned long long *colsums, uint32_t want_colsums) {
    if (ntiles == 0) return hipSuccess;
    const uint32_t nitems = 2u * (fo.ngenomes + 1u) + (want_colsums ? fo.ngenomes : 0u);
    const uint32_t per = std::max(1u, 256u / nitems), groups = (ntiles + TR_TILES - 1) / TR_TILES;
    hipLaunchKernelGGL(k_tile_reduce, dim3((groups + per - 1) / per), dim3(256), 0, st, fo, ad, tile_contig, ntiles, bins, colsums,
                       want_colsums);
    return hipGetLastError();
}

hipError_t launch_window_stats(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint64_t nrows, uint32_t nwin,
                               uint32_t pieces, const uint64_t *starts, const uint64_t *ends, unsigned long long *hist,
                               unsigned long long *cs) {
    if (nwin == 0) return hipSuccess;
    hipLaunchKernelGGL(k_window_stats, dim3(nwin, pieces), dim3(256), (2 * ngenomes + 1) * 4, st, ngenomes, rows, nrows,
                       starts, ends, hist, cs);
    return hipGetLastError();
}

hipError_t launch_cols_extract(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                               uint32_t tile_base, uint32_t ntiles, const uint8_t *out1, uint32_t g0, uint32_t width, void *dst) {
    if (ntiles == 0 || width == 0) return hipSuccess;
    if (ngenomes <= 8 && g0 < 8)  // one-byte rows
        hipLaunchKernelGGL(k_cols_extract_b1, dim3((unsigned)(((uint64_t)ntiles + 4 * COLS_TPW - 1) / (4 * COLS_TPW))), dim3(256), 0, st, ngenomes, ad, tile_contig, tile_base,
                           ntiles, out1, g0, width, static_cast<uint8_t *>(dst));
    else
        hipLaunchKernelGGL(k_cols_extract, dim3((unsigned)(((uint64_t)ntiles * TILE_SLOTS + 3) / 4)), dim3(256), 0, st, ngenomes, ad,
                           tile_contig, tile_base, ntiles, out1, g0, width, static_cast<unsigned long long *>(dst));
    return hipGetLastError();
}

hipError_t launch_cols_merge(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                             uint32_t tile_base, uint32_t ntiles, uint8_t *out1, const void *src, uint32_t part0,
                             uint32_t nparts, uint64_t part_words, uint32_t per, uint32_t accumulate) {
    if (ntiles == 0 || per == 0 || nparts == 0) return hipSuccess;
    if (ngenomes <= 8)  // one-byte rows
        hipLaunchKernelGGL(k_cols_merge_b1, dim3((unsigned)(((uint64_t)ntiles + 4 * COLS_TPW - 1) / (4 * COLS_TPW))), dim3(256), 0, st, ngenomes, ad, tile_contig, tile_base,
                           ntiles, out1, static_cast<const uint8_t *>(src), part0, nparts, part_words * 8, per, accumulate);
    else
        hipLaunchKernelGGL(k_cols_merge, dim3((unsigned)(((uint64_t)ntiles * TILE_SLOTS + 3) / 4)), dim3(256), 0, st, ngenomes, ad,
                           tile_contig, tile_base, ntiles, out1, static_cast<const unsigned long long *>(src), part0, nparts,
                           part_words, per, accumulate);
    return hipGetLastError();
}

hipError_t launch_rows_append(hipStream_t st, uint32_t n_old, uint32_t n_new, const AnchorDesc *src_ad, const uint32_t *src_tile_contig,
                              uint32_t ntiles, const uint8_t *src_rows, const AnchorDesc *dst_ad, uint32_t dst_first_contig,
                              uint8_t *dst_rows, const void *cols, uint32_t nparts, uint64_t part_words, uint32_t per) {
    if (ntiles == 0) return hipSuccess;
    AppendArgs A;
    A.sad = src_ad;
    A.stile_contig = src_tile_contig;
    A.src = src_rows;
    A.dad = dst_ad;
    A.dst = dst_rows;
    A.cols = static_cast<const unsigned long long *>(cols);
    A.part_words = part_words;
    A.ntiles = ntiles;
    A.dst_c0 = dst_first_contig;
    A.nparts = nparts;
    A.per = per;
    A.n_old = n_old;
    A.n_new = n_new;
    const uint32_t nw = ((n_new + 7) / 8 + 3) / 4;  // words per new row
    auto grid = [&](uint32_t spw) { return dim3((unsigned)(((uint64_t)ntiles * (TILE_SLOTS / spw) + 3) / 4)); };
    if (n_new <= 8) hipLaunchKernelGGL(k_rows_append_b1, dim3((unsigned)(((uint64_t)ntiles + 4 * COLS_TPW - 1) / (4 * COLS_TPW))), dim3(256), 0, st, A);
    else if (nw == 1) hipLaunchKernelGGL((k_rows_append<1, 8>), grid(8), dim3(256), 0, st, A);
    else if (nw == 2) hipLaunchKernelGGL((k_rows_append<2, 8>), grid(8), dim3(256), 0, st, A);
    else if (nw == 3) hipLaunchKernelGGL((k_rows_append<3, 4>), grid(4), dim3(256), 0, st, A);
    else if (nw == 4) hipLaunchKernelGGL((k_rows_append<4, 4>), grid(4), dim3(256), 0, st, A);
    else if (nw == 5) hipLaunchKernelGGL((k_rows_append<5, 4>), grid(4), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_rows_append<0, 4>), grid(4), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_rows_select(hipStream_t st, uint32_t n_old, uint32_t n_new, const AnchorDesc *src_ad, const uint32_t *src_tile_contig,
                              uint32_t ntiles, const uint8_t *src_rows, const AnchorDesc *dst_ad, uint32_t dst_first_contig,
                              uint8_t *dst_rows, const SelSeg *segs, uint32_t nseg, uint32_t need) {
    if (ntiles == 0) return hipSuccess;
    SelectArgs A;
    A.sad = src_ad;
    A.stile_contig = src_tile_contig;
    A.src = src_rows;
    A.dad = dst_ad;
    A.dst = dst_rows;
    A.segs = segs;
    A.nseg = nseg;
    A.need = need;
    A.ntiles = ntiles;
    A.dst_c0 = dst_first_contig;
    A.n_old = n_old;
    A.n_new = n_new;
    const uint32_t nws = ((n_old + 7) / 8 + 3) / 4;  // words per source row
    auto grid = [&](uint32_t spw) { return dim3((unsigned)(((uint64_t)ntiles * (TILE_SLOTS / spw) + 3) / 4)); };
    if (n_old <= 8) hipLaunchKernelGGL(k_rows_select_b1, dim3((unsigned)(((uint64_t)ntiles + 4 * COLS_TPW - 1) / (4 * COLS_TPW))), dim3(256), 0, st, A);
    else if (nws == 1) hipLaunchKernelGGL((k_rows_select<1, 8>), grid(8), dim3(256), 0, st, A);
    else if (nws == 2) hipLaunchKernelGGL((k_rows_select<2, 8>), grid(8), dim3(256), 0, st, A);
    else if (nws == 3) hipLaunchKernelGGL((k_rows_select<3, 4>), grid(4), dim3(256), 0, st, A);
    else if (nws == 4) hipLaunchKernelGGL((k_rows_select<4, 4>), grid(4), dim3(256), 0, st, A);
    else if (nws == 5) hipLaunchKernelGGL((k_rows_select<5, 4>), grid(4), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_rows_select<0, 4>), grid(4), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_lowres(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                         uint32_t ntiles, const uint8_t *out1, uint8_t *outlow, uint32_t step) {
    if (ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lowres, dim3(ntiles), dim3(64), 0, st, ngenomes, ad, tile_contig, out1, outlow, step);
    return hipGetLastError();
}

hipError_t preload_rows_kernels() {  // (any kernel of this unit loads its code object)
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_lowres));
}

}  // namespace pg
