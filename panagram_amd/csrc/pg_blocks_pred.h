// pg_blocks_pred.h — the predecessor search of the run kernels: k_run_blocks (pg_blocks.hip) and k_link_variants
// (pg_variants.hip) both give every lane of a 256-lane tile the LAST KEPT run before it.  Device code only.
#pragma once
#include "pg_blocks_link.h"

namespace pg {

struct RunPred {
    uint32_t pe, pml;  // exclusive end and last mate word of the predecessor (pml BLOCKS_NONE: there is none)
    uint64_t kb;       // the wave's kept-ballot
    uint64_t kbelow;   // ... below this lane
};

// One tile step, one run per lane (e, ml of a lane that is not kept are never handed on).  Inside a wave: the highest set bit
// of the kept-ballot below the lane and a shuffle from that lane; below the wave: the last kept run of the waves before it in
// the tile (wlast, LDS), then of the tiles before (carry_e / carry_ml, a register every lane holds; updated to the last kept
// run up to and with this tile).  wlast / wfirst: four entries each.  FIRST: the tile's first kept run goes to first_s /
// first_m once (have_first), for a pass that leaves its chunk's first kept run to the host.
// Holds ONE barrier, reached by every lane of the workgroup; the caller places another before the next call (wlast and wfirst
// are read behind this one and written again by the next call).
template <bool FIRST>
__device__ __forceinline__ RunPred blocks_pred(bool kept, uint32_t s, uint32_t e, uint32_t m, uint32_t ml, uint2 *wlast, uint2 *wfirst,
                                               uint32_t &carry_e, uint32_t &carry_ml, uint32_t &first_s, uint32_t &first_m,
                                               bool &have_first) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    RunPred r;
    r.kb = __ballot(kept);
    const uint64_t kb = r.kb;
    const uint64_t below = (1ull << lane) - 1ull;
    // the wave's last and first kept run
    if (kb ? lane == 63u - (uint32_t)__clzll((long long)kb) : lane == 0) wlast[wave] = make_uint2(e, kb ? ml : BLOCKS_NONE);
    if (kb && lane == (uint32_t)__ffsll((long long)kb) - 1u) wfirst[wave] = make_uint2(s, m);
    // the predecessor inside the wave: every lane takes part in the shuffles
    r.kbelow = kb & below;
    const int src = r.kbelow ? 63 - __clzll((long long)r.kbelow) : 0;
    r.pe = (uint32_t)__shfl((int)e, src);
    r.pml = (uint32_t)__shfl((int)ml, src);
    __syncthreads();
    uint32_t under_e = carry_e, under_ml = carry_ml;  // the last kept run below this wave
    uint32_t next_e = carry_e, next_ml = carry_ml;    // ... and below the next tile
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint2 l = wlast[w];
        if (l.y != BLOCKS_NONE) {
            if (w < wave) under_e = l.x, under_ml = l.y;
            next_e = l.x, next_ml = l.y;
            if (FIRST && !have_first) {
                const uint2 f = wfirst[w];
                first_s = f.x, first_m = f.y, have_first = true;
            }
        }
    }
    if (!r.kbelow) r.pe = under_e, r.pml = under_ml;
    carry_e = next_e, carry_ml = next_ml;
    return r;
}

}  // namespace pg
