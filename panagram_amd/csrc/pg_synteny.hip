// pg_synteny.hip — WHERE in genome B does the k-mer at a position of genome A lie (gfx950)?  The bitmap rows answer whether B
// holds it; this unit carries the positions: a hash table of canonical k-mers with one position field per side, the mate of
// every position of A, and the maximal collinear runs of mates — the unique-match segments a dot plot draws.
//
// Definitions (tests/synteny_ref.py is the same in numpy):
//   position   of a k-mer of a side = the global base offset of its first base in the concatenation of the side's contigs
//              (off[c] = the lengths of the contigs before c).  Windows holding a non-ACGT base do not exist.
//   key, rc    key = canonical_from_le(X); rc = 1 iff value(forward) > value(reverse complement), i.e. X > B in the notation
//              of pg_device.h (value(fwd) = ~B, value(revcomp) = ~X); a reverse-complement palindrome has X == B: rc = 0.
//   word       pos << 1 | rc: below POS_MULTI for pos <= 2^31 - 2, which the host checks (a side holds at most 2^31 - 1 bases).
//   unique     exactly one valid window of the side has the key (both strands count).
//   mate       of position i of A, iff its key is unique in A and in B: wordB ^ rcA = posB << 1 | (rcA ^ rcB); NO_MATE otherwise.
//   run        a maximal range [a, b) of consecutive k-mer positions of ONE contig of A whose mates have one strand and whose
//              posB advances by +1 per position on strand 0, by -1 on strand 1: mate[j] == mate[j - 1] + 2 / - 2.
//
// The table: `slots` (a power of two) 16-byte slots {u64 key, u32 word of side 0, u32 word of side 1}, all bytes 0xFF when empty
// — a key table, laid out and walked as pg_keytable_dev.h says: a lane whose claim reaches the bound sets flags[0] and gives up.
//   k_pos_insert   one launch per side over (contig, chunk) jobs as k_sketch_set.  A lane claims its key's slot (key_claim)
//                  and then  old = atomicCAS(&word[side], POS_EMPTY, mine): old a position -> the field becomes
//                  POS_MULTI.  A field only ever goes EMPTY -> word -> MULTI, whoever comes first: after the launch it holds
//                  the single occurrence's word or MULTI, whatever the order the lanes ran in.
//   k_pos_mates    the same walk over A; mates[koff[c] + p] for k-mer position p of contig c (contigs back to back), and the
//                  number of mated positions: a ballot per wave, one atomic per block.
//   k_mate_runs    the run scan of pg_runscan.h over chunks of MATE_CHUNK positions of one contig; a position's value is its
//                  mate, the halo one load.  With M = mated, P = predecessor mated, C = continues:
//                    run starts  M & ~C        run ends (exclusive)  P & ~C, and one at the contig's end when its last is mated
//                  counts[chunk] = {mated, starts, ends, 0}; beside a start goes its mate.
// Every write to HBM is a vector store or a vector atomic.
#include "pg_kernels.h"

#include "pg_postable_dev.h"  // PosSlot, kmer_key_rc, mate_continues; with it pg_keytable_dev.h
#include "pg_runscan.h"

namespace pg {

// job = positions [y * SYNTENY_JOB, (y + 1) * SYNTENY_JOB) of contig x, which holds at least k bases
__global__ __launch_bounds__(256) void k_pos_insert(int k, uint32_t side, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                    const uint32_t *__restrict__ off, const uint64_t *seqw_all, const uint32_t *nmw_all,
                                                    const uint32_t *has_n, PosSlot *slots, uint64_t nslots, uint32_t max_probe,
                                                    unsigned long long *flags) {
    const uint2 job = jobs[blockIdx.x];
    const ContigView v = contig_view(sd, job.x, seqw_all, nmw_all, has_n, k);
    const uint64_t p0 = (uint64_t)job.y * SYNTENY_JOB, p1 = min(v.nkmers, p0 + SYNTENY_JOB);
    const uint32_t base = off[job.x];
    const uint64_t smask = nslots - 1;
    for (uint64_t p = p0 + threadIdx.x; p < p1; p += 256) {
        if (!window_valid(v, p, k)) continue;
        uint64_t key;
        const uint32_t rc = kmer_key_rc(v.seqw, p, k, key) ? 1u : 0u;
        const uint32_t mine = ((base + (uint32_t)p) << 1) | rc;
        bool claimed;
        const uint64_t s = key_claim(slots, smask, max_probe, key, claimed);
        if (s == KEY_ABSENT) {
            atomicOr(reinterpret_cast<unsigned int *>(flags), 1u);
            continue;
        }
        const uint32_t old = atomicCAS(&slots[s].word[side], POS_EMPTY, mine);
        if (old != POS_EMPTY && old != POS_MULTI) atomicExch(&slots[s].word[side], POS_MULTI);
    }
}

__global__ __launch_bounds__(256) void k_pos_mates(int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                   const uint32_t *__restrict__ off, const uint32_t *__restrict__ koff,
                                                   const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                   const PosSlot *slots, uint64_t nslots, uint32_t max_probe,
                                                   uint32_t *__restrict__ mates, unsigned long long *nmated) {
    const uint2 job = jobs[blockIdx.x];
    const ContigView v = contig_view(sd, job.x, seqw_all, nmw_all, has_n, k);
    const uint64_t p0 = (uint64_t)job.y * SYNTENY_JOB, p1 = min(v.nkmers, p0 + SYNTENY_JOB);
    const uint32_t base = off[job.x];
    uint32_t *out = mates + koff[job.x];
    const uint64_t smask = nslots - 1;
    uint32_t found = 0;  // (per wave: every lane of a wave holds the same sum)
    for (uint64_t q = p0; q < p1; q += 256) {  // (bounds uniform over the block: every lane reaches the ballot)
        const uint64_t p = q + threadIdx.x;
        uint32_t mate = NO_MATE;
        if (p < p1 && window_valid(v, p, k)) {
            uint64_t key;
            const uint32_t rc = kmer_key_rc(v.seqw, p, k, key) ? 1u : 0u;
            const uint32_t mine = ((base + (uint32_t)p) << 1) | rc;
            PosSlot hit;
            if (key_find(slots, smask, max_probe, key, KEY_ABSENT, &hit) != KEY_ABSENT) {
                // unique in A: the field of side 0 is this very position; unique in B: the field of side 1 is a position
                const uint32_t a = hit.word[0], b = hit.word[1];
                if (a == mine && b != POS_EMPTY && b != POS_MULTI) mate = b ^ rc;
            }
        }
        if (p < p1) out[p] = mate;
        found += (uint32_t)__popcll(__ballot(mate != NO_MATE));
    }
    block_add(found, nmated);
}

// contigs[c] = {first entry of contig c in mates, its k-mer positions}; chunk = {contig, first position}
template <bool EMIT>
__global__ __launch_bounds__(256) void k_mate_runs(const uint32_t *__restrict__ mates, const uint2 *__restrict__ contigs,
                                                   const uint2 *__restrict__ chunks, uint4 *__restrict__ counts,
                                                   const ulonglong2 *__restrict__ offs, uint64_t total,
                                                   uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_end,
                                                   uint32_t *__restrict__ run_mate) {
    const uint2 ck = chunks[blockIdx.x];
    const uint2 cd = contigs[ck.x];
    const uint32_t *cm = mates + cd.x;
    // the chunk's halo: the mate of position c0 - 1 (every lane the same entry: one broadcast load)
    const uint32_t halo = ck.y > 0 ? cm[ck.y - 1] : NO_MATE;
    const ulonglong2 off = EMIT ? offs[blockIdx.x] : make_ulonglong2(0, 0);
    const uint4 c = chunk_runs<EMIT, MATE_CHUNK>(
        ck.y, cd.y, NO_MATE, halo, off, total, [&](uint32_t j) { return cm[j]; },
        [](bool act, uint32_t prev, uint32_t m, bool &starts, bool &ends) {
            const bool cont = act && mate_continues(prev, m);
            starts = act && m != NO_MATE && !cont;
            ends = act && prev != NO_MATE && !cont;
        },
        [](uint32_t tail) { return tail != NO_MATE; }, [](uint32_t m) { return m != NO_MATE; }, no_tally(),
        [&](uint64_t at, uint32_t j, uint32_t, uint32_t m) {
            run_start[at] = j;
            run_mate[at] = m;
        },
        [&](uint64_t at, uint32_t j, uint32_t, uint32_t) { run_end[at] = j; });
    if (!EMIT && threadIdx.x == 0) counts[blockIdx.x] = c;
}

hipError_t launch_pos_insert(hipStream_t st, int k, uint32_t side, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs,
                             const uint32_t *off, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, void *slots,
                             uint64_t nslots, uint32_t max_probe, unsigned long long *flags) {
    if (njobs == 0) return hipSuccess;
    if (k < 1 || k > 32 || side > 1 || nslots == 0 || (nslots & (nslots - 1)) || !slots || !flags) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pos_insert, dim3(njobs), dim3(256), 0, st, k, side, sd, jobs, off, seqw, nmw, has_n,
                       static_cast<PosSlot *>(slots), nslots, max_probe, flags);
    return hipGetLastError();
}

hipError_t launch_pos_mates(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint32_t *off,
                            const uint32_t *koff, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                            const void *slots, uint64_t nslots, uint32_t max_probe, uint32_t *mates, unsigned long long *nmated) {
    if (njobs == 0) return hipSuccess;
    if (k < 1 || k > 32 || nslots == 0 || (nslots & (nslots - 1)) || !slots || !mates || !nmated) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pos_mates, dim3(njobs), dim3(256), 0, st, k, sd, jobs, off, koff, seqw, nmw, has_n,
                       static_cast<const PosSlot *>(slots), nslots, max_probe, mates, nmated);
    return hipGetLastError();
}

hipError_t launch_mate_runs(hipStream_t st, const uint32_t *mates, const uint2 *contigs, const uint2 *chunks, uint32_t nchunks,
                            uint4 *counts, const ulonglong2 *offs, uint64_t total, uint32_t *run_start, uint32_t *run_end,
                            uint32_t *run_mate) {
    if (nchunks == 0) return hipSuccess;
    const bool emit = offs != nullptr;
    if (!mates || (emit ? (!run_start || !run_end || !run_mate) : !counts)) return hipErrorInvalidValue;
    if (emit)
        hipLaunchKernelGGL(k_mate_runs<true>, dim3(nchunks), dim3(256), 0, st, mates, contigs, chunks, counts, offs, total, run_start,
                           run_end, run_mate);
    else
        hipLaunchKernelGGL(k_mate_runs<false>, dim3(nchunks), dim3(256), 0, st, mates, contigs, chunks, counts, offs, total, run_start,
                           run_end, run_mate);
    return hipGetLastError();
}

}  // namespace pg
