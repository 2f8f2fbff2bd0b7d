// pg_tablestats.hip — shared distinct k-mer counts straight from the pan table ON THE GPU (gfx950).  The table holds every
// distinct canonical k-mer once with its N-bit presence mask; ONE pass over its slots gives
//   pairs[a][b]  distinct k-mers held by both genome a and genome b (the diagonal: the distinct k-mers of a),
//   occ[n]       distinct k-mers held by exactly n genomes (occ[N] the core, occ[0] whatever slot holds a key and no bit),
//   priv[g]      k-mers whose only bit is genome g,
//   nkeys        the slots counted
// — the exact Jaccard index of every pair at the table's own k, where the reference's `mash triangle` step
// (workflow/Snakefile:124-149) estimates it from a sketch at k = 21.
//
// A slot counts when its key < TOMB_KEY (empty and retired slots are skipped, as in k_export / k_rehash); only its W words in
// use are read, and the bits at and past N are masked off.  Keys and masks are addressed through key_ptr / mask_ptr (SlotWalk of
// pg_tablescan.h, which k_table_screen of pg_screen.hip walks the table with too) — a lane's
// slot of chunk 0 and the distance from one chunk to the next, both layouts' arrays being affine in the line number — so the
// kernel is the same in the slots (W = 1, 2), inline (W = 3) and split (W >= 4) layouts.
//
// grid = (blocks, 1, slices), 256 threads.  A chunk = the slots of 64 / slots-per-line whole lines (64 slots at 8 or 16 slots
// per line, 60 at the inline layout's 6), one slot per lane; wave w of block x takes chunks 4 x + w, 4 (x + blocks) + w, ...
//   scan       a lane reads its slot's key (the next chunk's is in flight meanwhile); a chunk without a key costs that read and a
//              ballot, nothing more.  The production table is sparse (1.25 keys per 8-slot line at BASELINE configs[1]: 10 keys
//              per chunk), so the lanes that hold a key COMPACT their W mask words into the wave's queue in LDS (a ring of 128
//              entries, positions from the ballot's prefix count) and the wave scans on until 64 are queued or its chunks end.
//   pop        lane i takes queue entry i: from here on a wave works on 64 keys, not on 64 slots.  Measured on an MI355X
//              against the kernel without the queue (one pair stage per 256 slots): profiles/kmerstats_rate.txt.
//   transpose  as in k_pair_counts: the ballot of bit c over the wave is the 64-key word of column c (pg_pairblocks.h)
//   occ, priv  one LDS add per key into the WAVE's counters (a lane's popcount; the bit of a lone one), flushed once per block
//              with 64-bit atomics; slice 0 only
//   pairs      the 4 x 4 blocks of pg_pairblocks.h.
//              N <= 64 (PRIVATE): every wave keeps counters of its own for all blocks (block lane, lane + 64, lane + 128 — the
//              136 blocks of N = 64 fit three rounds, the 55 of N = 40 one) and adds its own column words: no barrier anywhere,
//              the waves of a block never wait for each other.
//              Beyond: the thread block shares the blocks as k_pair_counts does (slice z takes blocks [768 z, 768 (z + 1))), in
//              ROUNDS: every wave scans until it can pop, the four words meet behind one barrier, and a wave whose chunks have
//              run out brings an empty word (flagged: the pair stage passes it over) until all four have.  Two buffers of words
//              and flags, so one barrier per round.
//
// A thread's pair counters (and the LDS counters) are 32 bits wide.  The GRID is sized so that a block visits fewer than 2^32
// slots: launch_table_pair_counts starts TABLESTATS_BLOCKS = 2048 blocks per slice wherever the table has that many chunks, and
// more where 2048 would leave a wave 2^24 chunks or more.  A table has at most 2^31 lines (alloc_sub) of at most 16 slots — 2^29
// chunks, 2^16 per wave, 2^24 slots per block — so the second rule never fires on a table the library can create: a 288 GB
// table in its densest layout (16 bytes per slot) is 1.8e10 slots, 8.8e6 per block.
// N <= 128 (MAXW = 4): a lane holds its entry's words in registers; beyond, up to PAIRS_MAX_GENOMES (MAXW = 0), it reads them
// from the queue word by word.
#include "pg_kernels.h"
#include "pg_rowread.h"
#include "pg_pairblocks.h"
#include "pg_tablescan.h"  // the chunks, a lane's walk over its slots, the grid
#include <algorithm>

namespace pg {

// LDS of one block, in 32-bit words behind the column words: the four queues, the round flags, the four waves' counters
__host__ __device__ __forceinline__ size_t ts_lds_bytes(uint32_t N, uint32_t W, bool priv_mode) {
    const uint32_t NC = (N + 63) & ~63u;
    return (size_t)(priv_mode ? 1 : 2) * 4 * NC * 8 + ((size_t)4 * TS_QCAP * W + 8 + (size_t)4 * (2 * N + 1)) * 4;
}

template <uint32_t MAXW, uint32_t ROUNDS, bool PRIVATE>
__global__ __launch_bounds__(256) void k_table_pair_counts(SubTable st, uint32_t N, uint64_t nchunks, uint32_t chunk_lines,
                                                           unsigned long long *__restrict__ pairs_out,
                                                           unsigned long long *__restrict__ occ_out,
                                                           unsigned long long *__restrict__ priv_out,
                                                           unsigned long long *__restrict__ nkeys_out) {
    extern __shared__ __align__(16) uint64_t tsm[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t W = min(st.W, (N + 31) / 32);
    const uint32_t NC = (N + 63) & ~63u;
    constexpr uint32_t NBUF = PRIVATE ? 1 : 2;
    uint32_t *queue = reinterpret_cast<uint32_t *>(tsm + (size_t)NBUF * 4 * NC) + (size_t)wave * TS_QCAP * W;
    uint32_t *flags = reinterpret_cast<uint32_t *>(tsm + (size_t)NBUF * 4 * NC) + (size_t)4 * TS_QCAP * W;
    uint32_t *occ_s = flags + 8 + wave * (2 * N + 1), *priv_s = occ_s + N + 1;  // (this wave's)
    const bool stats = blockIdx.z == 0;
    for (uint32_t i = lane; i < 2 * N + 1; i += 64) occ_s[i] = 0;
    PairBlocks<ROUNDS> pb;
    if (PRIVATE) pb.init(lane, 0, N, 64);
    else pb.init(tid, blockIdx.z, N);
    // this lane's slot of every chunk (byte-mask layout: the same walk by pointer steps, a byte read where the others read words)
    const SlotWalk sw(st, lane, nchunks, chunk_lines);
    const uint64_t cstride = (uint64_t)gridDim.x * 4;
    uint64_t c = (uint64_t)blockIdx.x * 4 + wave;
    uint64_t next_key = sw.key_of(c);
    uint32_t qh = 0, qn = 0;  // the queue's head and its entries (wave-uniform)
    uint32_t nk = 0;          // keys popped (wave-uniform)
    uint32_t buf = 0;
    wave_lds_sync();
    for (;;) {
        // scan: until 64 keys are queued or the wave's chunks have run out
        while (qn < 64 && c < nchunks) {
            const bool act = next_key < TOMB_KEY;  // (neither empty nor a retired copy)
            const uint64_t cur = c;
            c += cstride;
            next_key = sw.key_of(c);
            const uint64_t keys = __ballot(act);
            if (keys == 0) continue;  // (wave-uniform)
            if (act) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(keys >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)keys, 0u));
                uint32_t *e = queue + ((qh + qn + rank) & (TS_QCAP - 1)) * W;
                const uint32_t *m = sw.mask_words(cur);
                if (sw.bm) e[0] = sw.mask_byte(cur) & valid_bits(N, 0);
                else for (uint32_t d = 0; d < W; ++d) e[d] = m[d] & valid_bits(N, d);
            }
            qn += (uint32_t)__popcll(keys);
        }
        // pop: lane i takes entry i
        const uint32_t take = min(qn, 64u);
        if (PRIVATE && take == 0) break;  // (wave-uniform: nothing queued, nothing left to scan)
        uint64_t *cols = tsm + (size_t)buf * 4 * NC;
        uint64_t *mycols = cols + wave * NC;
        if (!PRIVATE && lane == 0) flags[4 * buf + wave] = take;
        if (take) {  // (wave-uniform)
            wave_lds_sync();
            const bool act = lane < take;
            const uint32_t *e = queue + ((qh + lane) & (TS_QCAP - 1)) * W;
            uint32_t pc = 0, g = 0;  // the key's genomes; the last of them
            if (MAXW) {
                uint32_t w[MAXW ? MAXW : 1];
#pragma unroll
                for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
                    w[d] = act && d < W ? e[d] : 0u;
                    pc += (uint32_t)__popc(w[d]);
                    g = w[d] ? 32 * d + 31 - (uint32_t)__clz((int)w[d]) : g;
                }
                uint64_t col = 0;
#pragma unroll
                for (uint32_t d = 0; d < (MAXW ? MAXW : 1); ++d) {
                    if (d < W) col = pairs_ballot_word(w[d], d, N, lane, col);
                    if ((d & 1) && 32 * (d - 1) < NC) {
                        mycols[32 * (d - 1) + lane] = col;
                        col = 0;
                    }
                }
            } else {
                for (uint32_t q = 0; 64 * q < NC; ++q) {
                    uint64_t col = 0;
                    for (uint32_t d = 2 * q; d < min(2 * q + 2, W); ++d) {
                        const uint32_t w = act ? e[d] : 0u;
                        pc += (uint32_t)__popc(w);
                        g = w ? 32 * d + 31 - (uint32_t)__clz((int)w) : g;
                        col = pairs_ballot_word(w, d, N, lane, col);
                    }
                    mycols[64 * q + lane] = col;
                }
            }
            if (stats) {
                nk += take;
                if (act) atomicAdd(&occ_s[pc], 1u);
                if (act && pc == 1) atomicAdd(&priv_s[g], 1u);
            }
            qh = (qh + take) & (TS_QCAP - 1);
            qn -= take;
        }
        if (PRIVATE) {
            wave_lds_sync();
#pragma unroll
            for (uint32_t r = 0; r < ROUNDS; ++r)
                if (pb.have[r]) pb.add(r, mycols);
            // (the next transpose writes these words behind the wave's own reads of them: LDS takes a wave's operations in order)
        } else {
            __syncthreads();
            const uint4 fl = *reinterpret_cast<const uint4 *>(flags + 4 * buf);  // (block-uniform)
            const uint32_t f[4] = {fl.x, fl.y, fl.z, fl.w};
            if ((f[0] | f[1] | f[2] | f[3]) == 0) break;  // every wave is through its chunks and its queue
#pragma unroll
            for (uint32_t r = 0; r < ROUNDS; ++r) {
                if (!pb.have[r]) continue;
#pragma unroll
                for (uint32_t wv = 0; wv < 4; ++wv)
                    if (f[wv]) pb.add(r, cols + wv * NC);
            }
            // (no second barrier: the next round goes to the other buffer and the other flags, and these are written again
            // only behind the next round's barrier, which every wave passes after these reads)
            buf ^= 1;
        }
    }
    pb.flush(pairs_out, N);
    if (!stats) return;  // (block-uniform)
    wave_lds_sync();
    for (uint32_t i = lane; i < N + 1; i += 64)
        if (occ_s[i]) atomicAdd(&occ_out[i], (unsigned long long)occ_s[i]);
    for (uint32_t i = lane; i < N; i += 64)
        if (priv_s[i]) atomicAdd(&priv_out[i], (unsigned long long)priv_s[i]);
    if (lane == 0 && nk) atomicAdd(nkeys_out, (unsigned long long)nk);
}

template <uint32_t MAXW, uint32_t ROUNDS, bool PRIVATE>
static hipError_t launch_ts(hipStream_t st, dim3 grid, size_t lds, const SubTable &t, uint32_t N, uint64_t nchunks, uint32_t chunk_lines,
                            unsigned long long *pairs, unsigned long long *occ, unsigned long long *priv, unsigned long long *nkeys) {
    auto fn = k_table_pair_counts<MAXW, ROUNDS, PRIVATE>;
    if (lds > 48 * 1024) {  // (beyond the default limit of dynamic LDS: N > 256 or so)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, grid, dim3(256), lds, st, t, N, nchunks, chunk_lines, pairs, occ, priv, nkeys);
    return hipGetLastError();
}

hipError_t launch_table_pair_counts(hipStream_t st, const SubTable &t, uint32_t ngenomes, unsigned long long *pairs,
                                    unsigned long long *occ, unsigned long long *priv, unsigned long long *nkeys) {
    if (ngenomes < 1 || ngenomes > PAIRS_MAX_GENOMES || t.slots < 1 || t.slots > 64 || 32ull * t.W < ngenomes)
        return hipErrorInvalidValue;
    if (t.nbuckets == 0) return hipSuccess;
    // fewer than 2^24 chunks per wave, so fewer than 2^32 slots per block (the file header)
    uint32_t chunk_lines;
    uint64_t nchunks;
    const uint64_t blocks = tablescan_blocks(t, chunk_lines, nchunks);
    if (blocks == 0) return hipErrorInvalidValue;
    const uint32_t W = std::min<uint32_t>(t.W, (ngenomes + 31) / 32), NB = (ngenomes + 3) / 4, nblk = NB * (NB + 1) / 2;
    const bool priv_mode = ngenomes <= 64;
    const uint32_t slices = priv_mode ? 1 : (nblk + PAIRS_ROUNDS * 256 - 1) / (PAIRS_ROUNDS * 256);
    const size_t lds = ts_lds_bytes(ngenomes, W, priv_mode);
    const dim3 grid((uint32_t)blocks, 1, slices);
    if (priv_mode && nblk <= 64) return launch_ts<4, 1, true>(st, grid, lds, t, ngenomes, nchunks, chunk_lines, pairs, occ, priv, nkeys);
    if (priv_mode) return launch_ts<4, PAIRS_ROUNDS, true>(st, grid, lds, t, ngenomes, nchunks, chunk_lines, pairs, occ, priv, nkeys);
    if (W <= 4) return launch_ts<4, PAIRS_ROUNDS, false>(st, grid, lds, t, ngenomes, nchunks, chunk_lines, pairs, occ, priv, nkeys);
    return launch_ts<0, PAIRS_ROUNDS, false>(st, grid, lds, t, ngenomes, nchunks, chunk_lines, pairs, occ, priv, nkeys);
}

}  // namespace pg
