// pg_planes.h — the column sums' carry-save counter planes (statistics kernels of pg_rows.hip), once.
//
// Per 32-bit word of a row a thread keeps VERTICAL counters: bit g of plane q is bit q of the number of rows seen with bit g
// set.  EIGHT planes per word behind a Harley-Seal carry-save tree: four rows enter the ones / twos planes per call (9
// instructions), their carry of weight 4 is held back every other call and enters the fours plane together with the next one
// (3), likewise the eights (3 per 8 rows), and only every 16 rows a carry ripples through the four upper planes (8): 3.3
// instructions per row and word (profiles/r4e_ab_stats_harley_seal.txt, r4e_ab_stats_harley_seal_mid.txt).  (Rounds 2-4 kept
// four planes, emptied every 12 rows into byte-sliced accumulators — 64 instructions per word — and those every 252 rows
// into LDS: 8.3 per row and word, a third of the wide pass's instructions, and 48 registers where this takes 40.)
// Which carries are held back follows from the number of rows in the planes (a multiple of 4, block-uniform in the kernels,
// who keep it beside the planes of their words): odd4 / odd8 below.
//
// The integer part compiles as plain C++ as well (tools/planes_check.cpp); the two ways to empty the planes into a
// workgroup's LDS column counters — the wave exchange and the per-lane adds — are device code.  The kernels' flushes in the
// MIDDLE of a contig (after PLANES_FLUSH rows of a thread; k_epilogue_w: once another group would pass PLANES_CEIL, at 248 or
// 252 rows with carries held back) run in the suite on the device: tests/test_gpu_planes_flush.py bounds the statistics
// launch to one and two workgroups (PG_EPI_WORKGROUPS, pg_rows.hip), so that contigs of 1.4 x 10^5 rows reach them at every row
// width; tests/epi_walk.py states which thread meets which flush.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PG_PLANES_HD __host__ __device__ __forceinline__
#else
#define PG_PLANES_HD
#endif

namespace pg {

constexpr uint32_t PLANES_CEIL = 255;   // what eight planes count to: no more rows than this between two flushes
constexpr uint32_t PLANES_FLUSH = 240;  // rows after which the kernels flush: whole 16-row blocks, and room for one more block

// One word's planes: a VIEW of storage the kernel declares as three arrays over its words (uint32_t vp[NW][8], pf[NW], pe[NW]:
// as one array of structs k_epilogue_w<15> takes 4 more bytes of scratch), built where it is used: Planes(vp[w], pf[w], pe[w]).
struct Planes {
    uint32_t (&p)[8], &pf, &pe;  // the planes; the carries of weight 4 and 8 held back
    PG_PLANES_HD Planes(uint32_t (&p_)[8], uint32_t &pf_, uint32_t &pe_) : p(p_), pf(pf_), pe(pe_) {}
    // carries held back while `rows` rows (a multiple of 4) are in the planes
    static PG_PLANES_HD bool odd4(uint32_t rows) { return (rows & 4u) != 0; }
    static PG_PLANES_HD bool odd8(uint32_t rows) { return (rows & 8u) != 0; }
    // add a word of carries of weight 2^q0 to the planes q0 .. 7 (no carry leaves plane 7: fewer than 256 rows)
    PG_PLANES_HD void ripple(uint32_t cw, int q0) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q >= q0) {
                const uint32_t n = p[q] & cw;
                p[q] ^= cw;
                cw = n;
            }
    }
    // four rows' words; o4 / o8 = odd4 / odd8 of the rows in the planes BEFORE these four (block-uniform)
    PG_PLANES_HD void add4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, bool o4, bool o8) {
        const uint32_t x = p[0];
        const uint32_t t1 = x ^ r0, s1 = t1 ^ r1, ca = (t1 & r1) | (~t1 & x);      // x + r0 + r1
        const uint32_t t2 = s1 ^ r2, s2 = t2 ^ r3, cb = (t2 & r3) | (~t2 & s1);    // .. + r2 + r3
        p[0] = s2;
        const uint32_t y = p[1];
        const uint32_t t3 = y ^ ca, cc = (t3 & cb) | (~t3 & y);                     // twos + ca + cb -> a carry of weight 4
        p[1] = t3 ^ cb;
        if (!o4) {  // held back: the next four rows' carry joins it
            pf = cc;
            return;
        }
        const uint32_t z = p[2], t4 = z ^ pf, c8 = (t4 & cc) | (~t4 & z);          // fours + both carries -> weight 8
        p[2] = t4 ^ cc;
        if (!o8) {
            pe = c8;
            return;
        }
        const uint32_t u = p[3], t5 = u ^ pe, c16 = (t5 & c8) | (~t5 & u);         // eights + both carries -> weight 16
        p[3] = t5 ^ c8;
        ripple(c16, 4);
    }
    // the carries still held back join their planes (a flush between whole 16-row blocks); o4 / o8 of the rows in the planes
    PG_PLANES_HD void settle(bool o4, bool o8) {
        if (o4) ripple(pf, 2);
        if (o8) ripple(pe, 3);
    }
    // transposition into byte counters: byte b of the result counts bit 8 b + q of the word (up to 255 rows)
    PG_PLANES_HD uint32_t bytes(int q) const {
        uint32_t v = 0;
#pragma unroll
        for (int pl = 0; pl < 8; ++pl) v |= ((p[pl] >> q) & 0x01010101u) << pl;
        return v;
    }
    PG_PLANES_HD void zero_planes() {  // (after a flush: settle has spent the carries)
#pragma unroll
        for (int q = 0; q < 8; ++q) p[q] = 0;
    }
    PG_PLANES_HD void clear() {
        zero_planes();
        pf = pe = 0;
    }
};

#ifdef __HIPCC__
// Planes of word `ws` of the rows -> the workgroup's N plain LDS counters `cs`, by a halving exchange over the wave (17
// shuffles per word) that leaves each column's total in one lane, which adds it.  Wave-uniform call sites only.
// (How the loop nest of the exchange compiles depends on the function it is inlined into: profiles/stats_share_isa.txt.)
__device__ __forceinline__ void planes_flush_wave(Planes P, uint32_t ws, uint32_t N, uint32_t *cs, int lane, bool o4, bool o8) {
    P.settle(o4, o8);
    uint32_t R[16];
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // byte b of v counts genome 32 ws + 8 b + q
        const uint32_t v = P.bytes(q);
        R[2 * q] = v & 0x00FF00FFu;
        R[2 * q + 1] = (v >> 8) & 0x00FF00FFu;
    }
    P.zero_planes();
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
        if (g0 < N && (R[0] & 0xFFFFu)) atomicAdd(&cs[g0], R[0] & 0xFFFFu);
        if (g0 + 16 < N && (R[0] >> 16)) atomicAdd(&cs[g0 + 16], R[0] >> 16);
    }
}
// Planes of one word -> the 32 LDS counters `cw` of that word in the lane's own copy: one add per lane and non-zero count
// (the chunk kernel, whose lanes hold different words of a row).
__device__ __forceinline__ void planes_flush_lanes(Planes P, uint32_t *cw, bool o4, bool o8) {
    P.settle(o4, o8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // bits j, 8 + j, 16 + j, 24 + j of the word: their four counts as the bytes of v
        const uint32_t v = P.bytes(j);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t cnt = (v >> (8 * b)) & 255u;
            if (cnt) atomicAdd(&cw[8 * b + j], cnt);
        }
    }
    P.zero_planes();
}
#endif

}  // namespace pg
