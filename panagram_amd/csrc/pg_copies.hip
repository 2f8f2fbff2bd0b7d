// pg_copies.hip — HOW OFTEN does a genome hold the k-mer at a position of a target sequence (gfx950)?  The bitmap rows answer
// whether; the position table of pg_synteny.hip answers where, for k-mers that occur once.  This unit counts: a hash table of the
// targets' canonical k-mers with counter planes beside it, a genome streamed through it per plane, and the counts reduced along
// the targets into a histogram of depths per target contig and genome.
//
// Definitions (tests/copies_ref.py is the same in numpy):
//   valid window   as everywhere: a window holding a non-ACGT base does not exist, a contig shorter than k has none.
//   depth_G(key)   the valid windows of genome G, over all its contigs, whose canonical key is `key` — both strands count through
//                  the canonical form.
//   d(p)           of position p of a target contig: depth_G(key(p)) when the window at p is valid; the position is invalid
//                  otherwise.  Targets are not deduplicated: a key repeated inside the targets has one slot, and every position
//                  that has the key reads the same depth.
//   hist[t][G][c]  the valid positions of target contig t with min(d, COPIES_BINS - 1) == c;  valid[t] = their number.
//   track          depth[G][koff[t] + p] = min(d, 65534) as u16, 65535 at an invalid position (koff: the k-mer positions of the
//                  contigs before t).
//
// The table: `nslots` (a power of two, at most 2^31) 8-byte keys — a key table, laid out and walked as pg_keytable_dev.h says.
// Beside the keys, planes of nslots u32 counters: plane g of slot s at planes[g * nslots + s].
//   k_copy_insert   one launch over (contig, chunk) jobs of the targets, as k_pos_insert walks them.  A lane claims its key's
//                   slot or finds it claimed already (key_claim); a lane that runs out of probes sets ctr[0].  The keys
//                   newly claimed are counted: a ballot per wave, one atomic per block (ctr[1]).
//   k_copy_count    the same walk over a whole genome, the table read-only: a valid window looks its key up (no target's key:
//                   nothing to do) and adds 1 to the plane's counter of its slot.  Integer atomic adds:
//                   the result is exact whatever order and contention.  Equal slots are folded inside a wave first
//                   (wave_fold_add, pg_keytable_dev.h).  Measured (profiles/copies_rate.txt): 100 Mb with a fifth in repeats
//                   1.81 ms, against 56.6 ms with one atomic per lane and 29.0 ms when only runs of neighbouring lanes are
//                   folded; no cost where every hit has a slot of its own.
//                   Hits: a ballot per wave, one atomic per block, as k_pos_mates counts mates.
//   k_copy_profile  the structure of k_presence_profile: one block per chunk of COPIES_CHUNK positions of one target contig, no
//                   block waits for another, no global atomic.  A lane resolves the slot of its 16 positions once (LDS: a slot
//                   number, or the marks INVALID / ABSENT — a key that is not in the table reads depth 0).  Then per plane: the
//                   depths from the plane, the 64-bin histogram in LDS — per wave, one plain add by lane 0 per distinct bin among
//                   the wave's lanes (wave_fold_bins, pg_keytable_dev.h) — the four waves' sums to partial[], and the u16
//                   depths to the track when one is asked for.  The host sums a contig's chunks (pg_copies_host.h).
// Every write to HBM is a vector store or a vector atomic.
#include "pg_kernels.h"
#include "pg_keytable_dev.h"  // the walk, copy_key, copy_lookup, the slot marks, the wave folds and block_add

namespace pg {

static_assert(COPIES_CHUNK % 256 == 0, "a chunk is a whole number of tiles");
static_assert(COPIES_BINS == 64, "one bin per lane of a wave");

// job = positions [y * COPIES_JOB, (y + 1) * COPIES_JOB) of contig x, which holds at least k bases
__global__ __launch_bounds__(256) void k_copy_insert(int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                     const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                     unsigned long long *keys, uint64_t nslots, uint32_t max_probe,
                                                     unsigned long long *ctr) {
    const uint2 job = jobs[blockIdx.x];
    const ContigView v = contig_view(sd, job.x, seqw_all, nmw_all, has_n, k);
    const uint64_t p0 = (uint64_t)job.y * COPIES_JOB, p1 = min(v.nkmers, p0 + COPIES_JOB);
    const uint64_t smask = nslots - 1;
    uint32_t nclaimed = 0;  // (per wave: every lane of a wave holds the same sum)
    for (uint64_t q = p0; q < p1; q += 256) {  // (bounds uniform over the block: every lane reaches the ballot)
        const uint64_t p = q + threadIdx.x;
        bool claimed = false;
        if (p < p1 && window_valid(v, p, k) && key_claim(keys, smask, max_probe, copy_key(v.seqw, p, k), claimed) == KEY_ABSENT)
            atomicOr(reinterpret_cast<unsigned int *>(ctr), 1u);
        nclaimed += (uint32_t)__popcll(__ballot(claimed));
    }
    block_add(nclaimed, ctr + 1);
}

__global__ __launch_bounds__(256) void k_copy_count(int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                    const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                    const unsigned long long *__restrict__ keys, uint64_t nslots, uint32_t max_probe,
                                                    uint32_t *plane, unsigned long long *hits) {
    const uint32_t lane = threadIdx.x & 63;
    const uint2 job = jobs[blockIdx.x];
    const ContigView v = contig_view(sd, job.x, seqw_all, nmw_all, has_n, k);
    const uint64_t p0 = (uint64_t)job.y * COPIES_JOB, p1 = min(v.nkmers, p0 + COPIES_JOB);
    const uint64_t smask = nslots - 1;
    uint32_t found = 0;  // (per wave)
    for (uint64_t q = p0; q < p1; q += 256) {  // (bounds uniform over the block)
        const uint64_t p = q + threadIdx.x;
        uint32_t slot = SLOT_ABSENT;
        if (p < p1 && window_valid(v, p, k)) slot = copy_lookup(keys, smask, max_probe, copy_key(v.seqw, p, k));
        const bool hit = slot != SLOT_ABSENT;
        found += (uint32_t)__popcll(__ballot(hit));
        wave_fold_add(hit, slot, lane, [&](uint32_t s, uint32_t n) { atomicAdd(&plane[s], n); });
    }
    block_add(found, hits);
}

// chunk = positions [y * COPIES_CHUNK, (y + 1) * COPIES_CHUNK) of contig x, which holds at least k bases
__global__ __launch_bounds__(256) void k_copy_profile(int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ chunks,
                                                      const uint64_t *__restrict__ koff, const uint64_t *seqw_all,
                                                      const uint32_t *nmw_all, const uint32_t *has_n,
                                                      const unsigned long long *__restrict__ keys, uint64_t nslots, uint32_t max_probe,
                                                      const uint32_t *__restrict__ planes, uint32_t nplanes,
                                                      uint32_t *__restrict__ partial, uint32_t *__restrict__ valid_partial,
                                                      uint16_t *__restrict__ depth, uint64_t depth_stride) {
    __shared__ uint32_t slot[COPIES_CHUNK];
    __shared__ uint32_t whist[4][COPIES_BINS];
    __shared__ uint32_t wvalid[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint2 ck = chunks[blockIdx.x];
    const ContigView v = contig_view(sd, ck.x, seqw_all, nmw_all, has_n, k);
    const uint64_t c0 = (uint64_t)ck.y * COPIES_CHUNK, ce = min(v.nkmers, c0 + COPIES_CHUNK);
    const uint64_t smask = nslots - 1;
    // the slots: entry i of the chunk is written and read by thread i & 255 alone
    uint32_t nvalid = 0;  // (per wave)
    for (uint32_t i = tid; i < COPIES_CHUNK; i += 256) {
        const uint64_t p = c0 + i;
        uint32_t s = SLOT_INVALID;
        if (p < ce && window_valid(v, p, k)) s = copy_lookup(keys, smask, max_probe, copy_key(v.seqw, p, k));
        slot[i] = s;
        nvalid += (uint32_t)__popcll(__ballot(s != SLOT_INVALID));
    }
    if (lane == 0) wvalid[wave] = nvalid;
    __syncthreads();
    if (tid == 0) valid_partial[blockIdx.x] = wvalid[0] + wvalid[1] + wvalid[2] + wvalid[3];
    uint16_t *track = depth ? depth + koff[ck.x] + c0 : nullptr;
    for (uint32_t g = 0; g < nplanes; ++g) {
        const uint32_t *pl = planes + (uint64_t)g * nslots;
        whist[wave][lane] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < COPIES_CHUNK; i += 256) {
            const uint32_t s = slot[i];
            const bool valid = s != SLOT_INVALID;
            const uint32_t dp = valid && s != SLOT_ABSENT ? pl[s] : 0u;
            if (track && c0 + i < ce) track[(uint64_t)g * depth_stride + i] = (uint16_t)(valid ? min(dp, COPIES_DEPTH_MAX) : COPIES_DEPTH_INVALID);
            const uint32_t bin = min(dp, COPIES_BINS - 1);
            wave_fold_bins(valid, bin, [&](uint32_t b, uint64_t m) {
                if (lane == 0) whist[wave][b] += (uint32_t)__popcll(m);
            });
        }
        __syncthreads();
        if (tid < COPIES_BINS)
            partial[((uint64_t)blockIdx.x * nplanes + g) * COPIES_BINS + tid] = whist[0][tid] + whist[1][tid] + whist[2][tid] + whist[3][tid];
        __syncthreads();
    }
}

static bool table_ok(int k, uint64_t nslots, const void *keys) {
    return k >= 1 && k <= 32 && nslots != 0 && !(nslots & (nslots - 1)) && nslots <= COPIES_MAX_SLOTS && keys;
}

hipError_t launch_copy_insert(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                              const uint32_t *nmw, const uint32_t *has_n, unsigned long long *keys, uint64_t nslots,
                              uint32_t max_probe, unsigned long long *ctr) {
    if (njobs == 0) return hipSuccess;
    if (!table_ok(k, nslots, keys) || !ctr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_copy_insert, dim3(njobs), dim3(256), 0, st, k, sd, jobs, seqw, nmw, has_n, keys, nslots, max_probe, ctr);
    return hipGetLastError();
}

hipError_t launch_copy_count(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys, uint64_t nslots,
                             uint32_t max_probe, uint32_t *plane, unsigned long long *hits) {
    if (njobs == 0) return hipSuccess;
    if (!table_ok(k, nslots, keys) || !plane || !hits) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_copy_count, dim3(njobs), dim3(256), 0, st, k, sd, jobs, seqw, nmw, has_n, keys, nslots,
                       max_probe, plane, hits);
    return hipGetLastError();
}

hipError_t launch_copy_profile(hipStream_t st, int k, const SeqDesc *sd, const uint2 *chunks, uint32_t nchunks, const uint64_t *koff,
                               const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys,
                               uint64_t nslots, uint32_t max_probe, const uint32_t *planes, uint32_t nplanes, uint32_t *partial,
                               uint32_t *valid_partial, uint16_t *depth, uint64_t depth_stride) {
    if (nchunks == 0) return hipSuccess;
    if (!table_ok(k, nslots, keys) || !planes || nplanes == 0 || !partial || !valid_partial || !koff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_copy_profile, dim3(nchunks), dim3(256), 0, st, k, sd, chunks, koff, seqw, nmw, has_n, keys, nslots, max_probe,
                       planes, nplanes, partial, valid_partial, depth, depth_stride);
    return hipGetLastError();
}

}  // namespace pg
