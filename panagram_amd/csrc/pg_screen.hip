// pg_screen.hip — WHICH of the indexed genomes does a sample hold (gfx950)?  The pan table holds every distinct canonical k-mer of
// every genome once, with its presence mask.  A sample — reads, or an assembly — is streamed through the table itself and
// counted per SLOT, and one pass over the slots joins the counts with the masks: per genome the k-mers the sample recovers, its
// private ones among them, the same by occupancy, and the depth histograms.  `mash screen`'s question, at the table's own k
// against the exact k-mer sets.
//
// Definitions (tests/screen_ref.py is the same in numpy):
//   valid window   as everywhere: a window holding a non-ACGT base does not exist, a contig shorter than k has none.
//   depth(key)     the valid windows of the sample whose canonical key is `key` — both strands, every set marked since the plane
//                  was cleared — saturating at SCREEN_DEPTH_MAX = 255.
//   the plane      one BYTE per slot beside the table: the byte of line l, slot s at l * st.slots + s in every layout (a 64-bit
//                  index: a table can hold 2^35 slots).  It belongs to one geometry of one table; the host refuses a stale one.
//
//   k_table_mark    one launch over the (contig, piece) jobs of a sequence set, the table read-only.  A valid window finds its
//                   slot (lane_find: the walk of lane_lookup) and adds 1 to the slot's byte.  Equal slots are folded inside the
//                   wave first (wave_fold_add, pg_keytable_dev.h, over the 64-bit index of the byte).  The add is a
//                   saturating add on the byte by a compare-and-swap on its aligned dword: the three neighbouring bytes are
//                   other slots' and go back as they were read, so no carry ever reaches them; a byte that reads 255 is left
//                   alone without an atomic.  Neighbouring positions of a read share their minimizer and so their home line:
//                   that is all the locality there is, the lines are not staged.  windows and hits: a ballot per wave, one
//                   atomic per block.
//   k_table_screen  one pass over the table's slots with the plane beside them, addressed as k_table_pair_counts does
//                   (pg_tablescan.h): the slots, inline, split and byte-mask layouts.  The production table is sparse (10 keys
//                   per 64-slot chunk), so the lanes that hold a key compact their mask words and their depth into the wave's
//                   queue in LDS and the wave works on 64 KEYS at a time, as that kernel does.  Per 64 keys: the ballot of bit
//                   c is column c's word (pg_pairblocks.h), the ballot of depth >= min_count the seen word; two popcounts per
//                   column give distinct and seen; a lane's popcount gives occ and seen_occ, a lone bit's lane private and
//                   private_seen; the depth bins are folded per wave (wave_fold_bins, pg_keytable_dev.h: one add per distinct
//                   bin among the wave's keys).  All of it into the BLOCK's 32-bit counters in LDS, flushed once with 64-bit
//                   atomics: no block waits for another.  The grid keeps a block below 2^32 slots (tablescan_blocks).
// Every write to HBM is a vector store or a vector atomic.
#include "pg_kernels.h"
#include "pg_keytable_dev.h"  // contig_view, window_valid, copy_key, the wave folds, block_add
#include "pg_rowread.h"       // valid_bits
#include "pg_pairblocks.h"
#include "pg_tablescan.h"

namespace pg {

static_assert(SCREEN_BINS == 64, "one bin per lane of a wave");

// byte `idx` of the plane += n, saturating at SCREEN_DEPTH_MAX
__device__ __forceinline__ void plane_add(uint8_t *plane, uint64_t idx, uint32_t n) {
    if (*reinterpret_cast<volatile uint8_t *>(plane + idx) == SCREEN_DEPTH_MAX) return;
    uint32_t *word = reinterpret_cast<uint32_t *>(plane + (idx & ~3ull));
    const uint32_t sh = 8u * (uint32_t)(idx & 3u);
    uint32_t cur = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t b = (cur >> sh) & 0xFFu;
        if (b == SCREEN_DEPTH_MAX) return;
        const uint32_t nb = min(b + n, SCREEN_DEPTH_MAX);  // (n <= 64: no overflow of the sum)
        const uint32_t seen = atomicCAS(word, cur, (cur & ~(0xFFu << sh)) | (nb << sh));
        if (seen == cur) return;
        cur = seen;
    }
}

// job = positions [y * SCREEN_JOB, (y + 1) * SCREEN_JOB) of contig x, which holds at least k bases.  ctr[0] += the valid windows,
// ctr[1] += those whose key the table holds
__global__ __launch_bounds__(256) void k_table_mark(SubTable st, int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                    const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                    uint8_t *plane, unsigned long long *ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint2 job = jobs[blockIdx.x];
    const ContigView v = contig_view(sd, job.x, seqw_all, nmw_all, has_n, k);
    const uint64_t p0 = (uint64_t)job.y * SCREEN_JOB, p1 = min(v.nkmers, p0 + SCREEN_JOB);
    uint32_t nvalid = 0, found = 0;  // (per wave)
    for (uint64_t q = p0; q < p1; q += 256) {  // (bounds uniform over the block)
        const uint64_t p = q + threadIdx.x;
        const bool valid = p < p1 && window_valid(v, p, k);
        uint32_t line = 0, slot = 0;
        const bool hit = valid && lane_find(st, copy_key(v.seqw, p, k), line, slot);
        const uint64_t idx = (uint64_t)line * st.slots + slot;
        nvalid += (uint32_t)__popcll(__ballot(valid));
        found += (uint32_t)__popcll(__ballot(hit));
        wave_fold_add(hit, idx, lane, [&](uint64_t i, uint32_t n) { plane_add(plane, i, n); });
    }
    const uint32_t sums[2] = {nvalid, found};
    block_add(sums, ctr);
}

// LDS of one block of k_table_screen, in 32-bit words: the block's counters, then the four waves' queues of W mask words and a depth
__host__ __device__ __forceinline__ uint32_t screen_counters(uint32_t N) { return 4 * N + 2 * (N + 1) + 2 * SCREEN_BINS; }
__host__ __device__ __forceinline__ size_t screen_lds_bytes(uint32_t N, uint32_t W) {
    return ((size_t)screen_counters(N) + (size_t)4 * TS_QCAP * (W + 1)) * 4;
}

// out: distinct [N], seen [N], private [N], private_seen [N], occ [N + 1], seen_occ [N + 1], depth_hist [64], core_depth_hist
// [64], nkeys [1] — the order of the block's counters in LDS
__global__ __launch_bounds__(256) void k_table_screen(SubTable st, uint32_t N, uint64_t nchunks, uint32_t chunk_lines,
                                                      const uint8_t *__restrict__ plane, uint32_t min_count,
                                                      unsigned long long *__restrict__ out) {
    extern __shared__ __align__(16) uint32_t ssm[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t W = min(st.W, (N + 31) / 32), E = W + 1;  // mask words in use; words of a queue entry
    const uint32_t ncnt = screen_counters(N);
    uint32_t *distinct_s = ssm, *seen_s = distinct_s + N, *priv_s = seen_s + N, *pseen_s = priv_s + N;
    uint32_t *occ_s = pseen_s + N, *socc_s = occ_s + N + 1, *dh_s = socc_s + N + 1, *ch_s = dh_s + SCREEN_BINS;
    uint32_t *queue = ssm + ncnt + (size_t)wave * TS_QCAP * E;
    for (uint32_t i = tid; i < ncnt; i += 256) ssm[i] = 0;
    __syncthreads();
    const SlotWalk sw(st, lane, nchunks, chunk_lines);
    const uint64_t cstride = (uint64_t)gridDim.x * 4;
    uint64_t c = (uint64_t)blockIdx.x * 4 + wave;
    uint64_t next_key = sw.key_of(c);
    uint32_t qh = 0, qn = 0;  // the queue's head and its entries (wave-uniform)
    uint32_t nk = 0;          // keys popped (wave-uniform)
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
                uint32_t *e = queue + ((qh + qn + rank) & (TS_QCAP - 1)) * E;
                if (sw.bm) {
                    e[0] = sw.mask_byte(cur) & valid_bits(N, 0);
                } else {
                    const uint32_t *m = sw.mask_words(cur);
                    for (uint32_t d = 0; d < W; ++d) e[d] = m[d] & valid_bits(N, d);
                }
                e[W] = plane[sw.line_of(cur) * st.slots + sw.s];  // (the line is below st.nbuckets: key_of found a key there)
            }
            qn += (uint32_t)__popcll(keys);
        }
        // pop: lane i takes entry i
        const uint32_t take = min(qn, 64u);
        if (take == 0) break;  // (wave-uniform: nothing queued, nothing left to scan)
        wave_lds_sync();
        const bool act = lane < take;
        const uint32_t *e = queue + ((qh + lane) & (TS_QCAP - 1)) * E;
        const uint32_t dep = act ? e[W] : 0u;
        const bool seen = act && dep >= min_count;
        const uint64_t seenw = __ballot(seen);
        uint32_t pc = 0, g = 0;  // the key's genomes; the last of them
        for (uint32_t q = 0; 64 * q < N; ++q) {
            uint64_t col = 0;  // the 64-key word of column 64 q + lane
            for (uint32_t d = 2 * q; d < min(2 * q + 2, W); ++d) {
                const uint32_t w = act ? e[d] : 0u;
                pc += (uint32_t)__popc(w);
                g = w ? 32 * d + 31 - (uint32_t)__clz((int)w) : g;
                col = pairs_ballot_word(w, d, N, lane, col);
            }
            if (col) {  // (a column at or past N has no bit: the masks were cut to N)
                atomicAdd(&distinct_s[64 * q + lane], (uint32_t)__popcll(col));
                const uint32_t ns = (uint32_t)__popcll(col & seenw);
                if (ns) atomicAdd(&seen_s[64 * q + lane], ns);
            }
        }
        if (act) atomicAdd(&occ_s[pc], 1u);
        if (seen) atomicAdd(&socc_s[pc], 1u);
        if (act && pc == 1) atomicAdd(&priv_s[g], 1u);
        if (seen && pc == 1) atomicAdd(&pseen_s[g], 1u);
        // the depth bins: one turn per distinct bin among the wave's keys, 64 at the most
        const uint32_t bin = min(dep, SCREEN_BINS - 1);
        const bool core = act && pc == N;
        wave_fold_bins(act, bin, [&](uint32_t b, uint64_t m) {
            const uint64_t mc = __ballot(core && bin == b);
            if (lane == 0) atomicAdd(&dh_s[b], (uint32_t)__popcll(m));
            if (lane == 0 && mc) atomicAdd(&ch_s[b], (uint32_t)__popcll(mc));
        });
        nk += take;
        qh = (qh + take) & (TS_QCAP - 1);
        qn -= take;
        wave_lds_sync();  // (the entries were read before the next scan writes the ring again)
    }
    if (lane == 0 && nk) atomicAdd(&out[ncnt], (unsigned long long)nk);
    __syncthreads();
    for (uint32_t i = tid; i < ncnt; i += 256)
        if (ssm[i]) atomicAdd(&out[i], (unsigned long long)ssm[i]);
}

hipError_t launch_table_mark(hipStream_t st, const SubTable &t, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, uint8_t *plane, unsigned long long *ctr) {
    if (njobs == 0) return hipSuccess;
    if (t.k < 1 || t.k > 32 || t.nbuckets == 0 || t.slots < 1 || t.slots > 64 || !t.buckets || !plane || !ctr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_table_mark, dim3(njobs), dim3(256), 0, st, t, (int)t.k, sd, jobs, seqw, nmw, has_n, plane, ctr);
    return hipGetLastError();
}

hipError_t launch_table_screen(hipStream_t st, const SubTable &t, uint32_t ngenomes, const uint8_t *plane, uint32_t min_count,
                               unsigned long long *out) {
    if (ngenomes < 1 || ngenomes > PAIRS_MAX_GENOMES || t.slots < 1 || t.slots > 64 || 32ull * t.W < ngenomes || !plane || !out ||
        min_count < 1 || min_count > SCREEN_DEPTH_MAX)
        return hipErrorInvalidValue;
    if (t.nbuckets == 0) return hipSuccess;
    uint32_t chunk_lines;
    uint64_t nchunks;
    const uint64_t blocks = tablescan_blocks(t, chunk_lines, nchunks);
    if (blocks == 0) return hipErrorInvalidValue;
    const uint32_t W = std::min<uint32_t>(t.W, (ngenomes + 31) / 32);
    const size_t lds = screen_lds_bytes(ngenomes, W);
    if (lds > 48 * 1024) {  // (beyond the default limit of dynamic LDS; 512 genomes in 16 words stay below it)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_table_screen), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_table_screen, dim3((uint32_t)blocks), dim3(256), lds, st, t, ngenomes, nchunks, chunk_lines, plane, min_count, out);
    return hipGetLastError();
}

}  // namespace pg
