// pg_genotype.hip — WHICH ALLELE of a variant does a sample carry (gfx950)?  pg_variants.hip gives the variants of genome B against
// genome A; the count table of pg_copies.hip counts k-mers per plane.  This unit works on allele ranges instead of whole contigs:
// the k-mers that span an allele go into the count table, and three planes — depth in the allele's own genome, in the other
// genome, in the sample — are reduced along those k-mers to four integers per range.  Nothing per position leaves HBM.
//
// Definitions (tests/genotype_ref.py is the same in numpy), k the table's k:
//   allele range   (c, s, l): bases [s, s + l) of contig c of a sequence set, s + l <= the contig's length L.  l = 0 is the
//                  junction between base s - 1 and base s.
//   allele windows the k-mer positions p of contig c with max(0, s - k + 1) <= p < min(L - k + 1, s + l): every window that
//                  overlaps the allele.  For l = 0 the k - 1 windows that hold both neighbours of the junction.  None when L < k,
//                  none for a junction at s = 0 or s = L.  A window holding a non-ACGT base does not exist, as everywhere.
//   informative    given planes own, other and sample of the table, an allele window with canonical key κ — the strand of the
//                  variant plays no part — is informative when own[κ] == 1 && other[κ] == 0: the k-mer occurs exactly once in the
//                  genome the allele comes from and nowhere in the other.  It is seen when also sample[κ] >= min_count.  A key
//                  the table does not hold reads 0 in all three planes and is never informative.
//   per range i    windows[i] = the allele windows that exist, inf[i] = the informative ones, seen[i] = the seen ones, depth[i] =
//                  the sum of sample[κ] over the informative ones, in 64 bits.
//
// Both kernels work on pieces: the host cuts every range's window interval into pieces of at most ALLELE_PIECE = 64 windows
// (pg_genotype_host.h) and uploads the list.  One wave takes one piece, one window per lane; a block of 256 threads takes four
// pieces.  No wave loops over an allele — a deletion of 65 536 bases is 1 025 pieces —, no block waits for another.
//   k_allele_insert   a lane whose window exists claims its key (key_claim).  Overflow and the keys newly claimed are kept as
//                     k_copy_insert keeps them: the flag in ctr[0], a ballot per wave and block_add into ctr[1].
//   k_allele_support  such a lane looks its key up (copy_lookup) and reads the three planes at the slot.  The wave reduces
//                     windows, inf and seen by ballot and popcount, and the 64-bit depth by a shuffle tree; lane 0 writes the
//                     piece's partial in one 16-byte vector store.  No atomics.  The host adds a range's pieces in 64 bits.
// The piece of a wave is wave-uniform, so every lane reaches every ballot and shuffle.  Every write to HBM is a vector store or a
// vector atomic.
#include "pg_kernels.h"
#include "pg_keytable_dev.h"  // the walk, copy_key, copy_lookup, window_valid and block_add

namespace pg {

static_assert(ALLELE_PIECE == 64, "one window per lane of a wave");
static_assert(sizeof(AllelePiece) == 16 && sizeof(AllelePartial) == 16, "read and written as 16 bytes");

// the window of this lane: does it exist?  v and p are set when the lane lies inside the piece
__device__ __forceinline__ bool allele_lane(const AllelePiece &pc, uint32_t lane, int k, const SeqDesc *__restrict__ sd,
                                            const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n, ContigView &v,
                                            uint64_t &p) {
    if (lane >= pc.n) return false;
    v = contig_view(sd, pc.contig, seqw_all, nmw_all, has_n, k);
    p = pc.p0 + lane;
    return window_valid(v, p, k);
}

__global__ __launch_bounds__(256) void k_allele_insert(int k, const SeqDesc *__restrict__ sd, const AllelePiece *__restrict__ pieces,
                                                       uint32_t npieces, const uint64_t *seqw_all, const uint32_t *nmw_all,
                                                       const uint32_t *has_n, unsigned long long *keys, uint64_t nslots,
                                                       uint32_t max_probe, unsigned long long *ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t pi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (wave-uniform)
    const uint64_t smask = nslots - 1;
    bool claimed = false;
    if (pi < npieces) {
        const AllelePiece pc = pieces[pi];
        ContigView v = {};
        uint64_t p = 0;
        if (allele_lane(pc, lane, k, sd, seqw_all, nmw_all, has_n, v, p) &&
            key_claim(keys, smask, max_probe, copy_key(v.seqw, p, k), claimed) == KEY_ABSENT)
            atomicOr(reinterpret_cast<unsigned int *>(ctr), 1u);
    }
    block_add((uint32_t)__popcll(__ballot(claimed)), ctr + 1);  // (every lane of the block reaches this)
}

__global__ __launch_bounds__(256) void k_allele_support(int k, const SeqDesc *__restrict__ sd, const AllelePiece *__restrict__ pieces,
                                                        uint32_t npieces, const uint64_t *seqw_all, const uint32_t *nmw_all,
                                                        const uint32_t *has_n, const unsigned long long *__restrict__ keys,
                                                        uint64_t nslots, uint32_t max_probe, const uint32_t *__restrict__ own,
                                                        const uint32_t *__restrict__ other, const uint32_t *__restrict__ sample,
                                                        uint32_t min_count, AllelePartial *__restrict__ partial) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t pi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (wave-uniform)
    if (pi >= npieces) return;                                          // (the whole wave: no barrier follows)
    const uint64_t smask = nslots - 1;
    const AllelePiece pc = pieces[pi];
    ContigView v = {};
    uint64_t p = 0;
    const bool exists = allele_lane(pc, lane, k, sd, seqw_all, nmw_all, has_n, v, p);
    bool inf = false;
    uint32_t d = 0;
    if (exists) {
        const uint32_t s = copy_lookup(keys, smask, max_probe, copy_key(v.seqw, p, k));
        if (s != SLOT_ABSENT && own[s] == 1u && other[s] == 0u) {
            inf = true;
            d = sample[s];
        }
    }
    const uint64_t nwin = (uint64_t)__popcll(__ballot(exists)), ninf = (uint64_t)__popcll(__ballot(inf));
    const uint64_t nseen = (uint64_t)__popcll(__ballot(inf && d >= min_count));
    uint64_t depth = d;  // (0 in a lane that is not informative)
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)depth, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(depth >> 32), off);
        depth += (uint64_t)lo | ((uint64_t)hi << 32);
    }
    if (lane == 0) {
        const ulonglong2 out = make_ulonglong2(nwin | ninf << 16 | nseen << 32, depth);
        *reinterpret_cast<ulonglong2 *>(partial + pi) = out;
    }
}

static bool allele_table_ok(int k, uint64_t nslots, const void *keys) {
    return k >= 1 && k <= 32 && nslots != 0 && !(nslots & (nslots - 1)) && nslots <= COPIES_MAX_SLOTS && keys;
}

hipError_t launch_allele_insert(hipStream_t st, int k, const SeqDesc *sd, const AllelePiece *pieces, uint32_t npieces, const uint64_t *seqw,
                                const uint32_t *nmw, const uint32_t *has_n, unsigned long long *keys, uint64_t nslots,
                                uint32_t max_probe, unsigned long long *ctr) {
    if (npieces == 0) return hipSuccess;
    if (!allele_table_ok(k, nslots, keys) || !pieces || !ctr || npieces > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_allele_insert, dim3((npieces + 3) / 4), dim3(256), 0, st, k, sd, pieces, npieces, seqw, nmw, has_n, keys, nslots,
                       max_probe, ctr);
    return hipGetLastError();
}

hipError_t launch_allele_support(hipStream_t st, int k, const SeqDesc *sd, const AllelePiece *pieces, uint32_t npieces,
                                 const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys,
                                 uint64_t nslots, uint32_t max_probe, const uint32_t *own, const uint32_t *other, const uint32_t *sample,
                                 uint32_t min_count, AllelePartial *partial) {
    if (npieces == 0) return hipSuccess;
    if (!allele_table_ok(k, nslots, keys) || !pieces || !own || !other || !sample || min_count == 0 || !partial || npieces > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_allele_support, dim3((npieces + 3) / 4), dim3(256), 0, st, k, sd, pieces, npieces, seqw, nmw, has_n, keys, nslots,
                       max_probe, own, other, sample, min_count, partial);
    return hipGetLastError();
}

}  // namespace pg
