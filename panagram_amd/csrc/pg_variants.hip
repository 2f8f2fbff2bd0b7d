// pg_variants.hip — the links of the synteny blocks (pg_blocks.hip) as VARIANTS of B against A (gfx950): every link of every block
// is classified, compared base by base and emitted with its alleles.  Runs, blocks and sequences stay in HBM, only variants leave.
//
// Definitions (tests/variants_ref.py is the same in numpy); run, kept, predecessor, link, dA, dB, strand σ are those of
// pg_blocks.hip and pg_blocks_link.h.  For a link i -> j write p = e_i - 1, the A position of run i's last k-mer; s = s_j;
// bl = the B position of run i's last k-mer; b = b_j.  Positions of A are contig-relative, positions of B global, as in the
// mate words.
//   overlap     t = max(0, k - min(dA, dB)); min(dA, dB) >= 1, so t <= k - 1.  The two matched flanks overlap by t bases on the
//               shorter side — an indel inside a short tandem repeat — and the difference is placed at the leftmost place in A
//               that the flanks allow.
//   A allele    bases [posA, posA + lenA) of the contig of A, posA = p + k - t, lenA = dA - k + t.  Base posA - 1 always exists,
//               lies in run i's last matched k-mer, is ACGT and identical in B: the anchor base a VCF indel needs.
//   B allele    lenB = dB - k + t bases: [bl + k - t, b) on strand 0, [b + k, bl + t) on strand 1; posB is the lowest base of
//               that range, which lies inside one contig of B (a link requires bl and b in the same contig).  "In A's
//               orientation": as stored on strand 0, reverse-complemented on strand 1 — A base posA + i faces B base posB + i
//               on strand 0 and the complement of B base posB + lenB - 1 - i on strand 1.
//   mismatches  defined only when lenA == lenB: the number of i in [0, lenA) where the facing bases differ or either is
//               non-ACGT.  0 otherwise.
//   class       0 same: lenA == lenB and mismatches == 0 (lenA == 0 included: the run broke on k-mers that are not unique, not
//               on a difference) — counted, never emitted; 1 snp: lenA == lenB == 1, mismatches == 1; 2 mnp: lenA == lenB >= 2,
//               mismatches >= 1; 3 ins: lenA == 0 < lenB; 4 del: lenB == 0 < lenA; 5 complex: both positive and unequal.
//   N flag      either allele range holds a non-ACGT base.
//   record      one per link of class != 0: contig of A, posA, lenA, posB, lenB, info = σ | class << 1 | code of A base
//               posA - 1 << 4 | N flag << 6, mismatches, and two 64-bit words: the first min(len, 32) bases of the A allele and
//               of the B allele in A's orientation, 2 bits per base, base i at bits 2i and 2i + 1 (the seqset's own packing),
//               the unused high bits zero.
//   Records are sorted by (contig of A, run j) = (contig, posA), the same on every call.
//   Invariant: for every block, A's bases from the first run's start to the last run's end + k - 1 with each emitted record's
//   A allele replaced by its B allele in A's orientation are exactly B's range of the block, reverse-complemented on strand 1.
//
// k_link_variants<EMIT> has the shape of k_run_blocks: chunks of RUN_CHUNK runs of one contig of A, tiles of 256, waves of 64,
// one run per lane, the predecessor by blocks_pred (pg_blocks_pred.h) and the link by blocks_link (pg_blocks_link.h).  The
// predecessor of a chunk's first kept run is the carry of the blocks' stitch (BlockChunkOffs::carry_e / carry_ml): both passes
// run after blocks_stitch.
//   count (EMIT = false)  per chunk a VariantChunkCount: the links of every class.
//   host                  an exclusive scan of the chunks' records (classes 1..5).
//   emit                  the record planes at those offsets.
// A lane whose run links reads both packed planes and both N-mask planes 32 bases per step: at most max_gap / 32 <= 2048 steps
// (the host refuses max_gap above VARIANTS_MAX_GAP).  A contig's planes carry two zero words behind the last base and none in
// front: a strand-1 window is read downwards from the range's top, and where it would begin before base 0 of B's contig it is
// read from base 0 and shifted — no word index below the contig's seq_off is ever formed; every base index is held below the
// contig's length.  No atomics, every barrier is reached by every lane, every write to HBM is a vector store.
#include "pg_kernels.h"

#include "pg_blocks_pred.h"

namespace pg {

constexpr uint32_t VAR_TILE = 256;
static_assert(RUN_CHUNK % VAR_TILE == 0, "a chunk is a whole number of tiles");

namespace {

// the planes of one contig
struct ContigView {
    const uint64_t *w;
    const uint32_t *n;
    uint64_t last;  // the contig's last base (a contig that holds a run has one)
};
__device__ __forceinline__ ContigView view_of(const SeqDesc *sd, uint32_t c, const uint64_t *seqw, const uint32_t *nmw) {
    const SeqDesc d = sd[c];
    ContigView v;
    v.w = seqw + d.seq_off;
    v.n = nmw + d.seq_off;
    v.last = d.len ? d.len - 1 : 0;
    return v;
}
// 32 bases / their 32 "not ACGT" bits from base p on (p held inside the contig: the reads stay inside its words)
__device__ __forceinline__ uint64_t bases_at(const ContigView &v, uint64_t p) { return extract_bases(v.w, p < v.last ? p : v.last); }
__device__ __forceinline__ uint32_t nmask_at(const ContigView &v, uint64_t p) {
    return (uint32_t)extract_nmask64(v.n, p < v.last ? p : v.last);
}
__device__ __forceinline__ uint64_t low_bases(uint32_t n) { return n >= 32 ? ~0ull : ((1ull << (2 * n)) - 1ull); }
__device__ __forceinline__ uint32_t low_bits(uint32_t n) { return n >= 32 ? ~0u : ((1u << n) - 1u); }
// bit i of x at bit 2 i
__device__ __forceinline__ uint64_t spread_bits(uint32_t x32) {
    uint64_t x = x32;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// up to 32 bases of B's allele in A's orientation from allele base i on (i < len), and their "not ACGT" bits: lo = the allele's
// lowest base inside B's contig.  Strand 1: allele base i is the complement of B base lo + len - 1 - i — the window ends at
// top = lo + len - i (exclusive) and begins 32 bases below it, or at base 0 of the contig, shifted.  Bits past the allele's end
// are whatever lies there: the caller masks.
__device__ __forceinline__ void b_window(const ContigView &v, uint32_t strand, uint64_t lo, uint32_t len, uint32_t i, uint64_t *bases,
                                         uint32_t *nm) {
    if (!strand) {
        *bases = bases_at(v, lo + i);
        *nm = nmask_at(v, lo + i);
        return;
    }
    const uint64_t top = lo + len - i;  // >= 1
    const uint64_t from = top >= 32 ? top - 32 : 0;
    const uint32_t sh = 32u - (uint32_t)(top - from);  // 0..31
    *bases = pair_reverse64(~bases_at(v, from)) >> (2 * sh);
    *nm = __brev(nmask_at(v, from)) >> sh;
}

}  // namespace

// contigs[c] = {first run of contig c in the run arrays, its runs}; chunk = {contig, first run inside the contig}; boff: nb
// ascending offsets of B's contigs, the first 0, ncb = B's contigs.  out32: 6 planes of `total` words (posA, lenA, posB, lenB,
// info, mismatches), out64: 2 planes (A allele, B allele).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_link_variants(const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ run_end,
                                                       const uint32_t *__restrict__ run_mate, const uint2 *__restrict__ contigs,
                                                       const uint2 *__restrict__ chunks, const uint64_t *__restrict__ boff, uint32_t nb,
                                                       uint32_t ncb, uint32_t k, uint32_t min_run, uint32_t max_gap, uint32_t max_shift,
                                                       const BlockChunkOffs *__restrict__ offs, const SeqDesc *__restrict__ sdA,
                                                       const uint64_t *__restrict__ seqwA, const uint32_t *__restrict__ nmwA,
                                                       const SeqDesc *__restrict__ sdB, const uint64_t *__restrict__ seqwB,
                                                       const uint32_t *__restrict__ nmwB, VariantChunkCount *__restrict__ counts,
                                                       const uint64_t *__restrict__ voffs, uint64_t total, uint32_t *__restrict__ out32,
                                                       uint64_t *__restrict__ out64) {
    __shared__ uint2 wlast[4];       // {e, ml} of every wave's last kept run (ml BLOCKS_NONE: the wave has none)
    __shared__ uint2 wfirst[4];      // (blocks_pred's; not read here)
    __shared__ uint32_t wcls[4][8];  // the links of classes 0..5 of every wave, [6] = its records
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint2 ck = chunks[blockIdx.x];
    const uint2 cd = contigs[ck.x];
    const uint32_t *rs = run_start + cd.x, *re = run_end + cd.x, *rm = run_mate + cd.x;
    const uint32_t nr = cd.y, c0 = ck.y, ce = min(c0 + RUN_CHUNK, nr);  // this chunk: runs [c0, ce) of the contig, c0 < ce <= nr
    const BlockChunkOffs o = offs[blockIdx.x];
    uint32_t carry_e = o.carry_e, carry_ml = o.carry_ml;  // the last kept run before the tile, the chunks before included
    const ContigView va = view_of(sdA, ck.x, seqwA, nmwA);
    uint32_t ncls[6] = {0, 0, 0, 0, 0, 0};  // of the tiles before
    uint32_t nrec = 0;
    const uint64_t voff = EMIT ? voffs[blockIdx.x] : 0;
    uint32_t unused_s = 0, unused_m = 0;
    bool unused_first = false;
    for (uint32_t t0 = c0; t0 < ce; t0 += VAR_TILE) {  // (bounds uniform over the block)
        const uint32_t j = t0 + tid;
        const bool act = j < ce;
        const uint32_t s = act ? rs[j] : 0u, e = act ? re[j] : 1u, m = act ? rm[j] : 0u;
        const uint32_t n = e - s;
        const bool kept = act && n >= min_run;
        const uint32_t ml = blocks_last_mate(m, n);
        const RunPred pr = blocks_pred<false>(kept, s, e, m, ml, wlast, wfirst, carry_e, carry_ml, unused_s, unused_m, unused_first);
        bool shifted = false;
        const bool link = kept && blocks_link(pr.pe, pr.pml, s, m, max_gap, max_shift, boff, nb, &shifted);
        uint32_t cls = 6;  // no link
        uint32_t posA = 0, lenA = 0, posB = 0, lenB = 0, info = 0, mism = 0;
        uint64_t alA = 0, alB = 0;
        if (link) {
            const uint32_t strand = m & 1u;
            const uint32_t p = pr.pe - 1u, bl = pr.pml >> 1, b = m >> 1;
            const uint32_t dA = s - p, dB = strand ? bl - b : b - bl;  // 1..max_gap each
            const uint32_t dmin = dA < dB ? dA : dB;
            const uint32_t t = k > dmin ? k - dmin : 0u;
            posA = p + k - t;
            lenA = dA - k + t;
            lenB = dB - k + t;
            posB = strand ? b + k : bl + k - t;
            // B's contig and the allele's place inside it
            uint32_t cb = blocks_rank(boff, nb, (uint64_t)bl);
            cb = cb ? cb - 1u : 0u;
            if (cb >= ncb) cb = ncb - 1u;
            const ContigView vb = view_of(sdB, cb, seqwB, nmwB);
            const uint64_t lo = (uint64_t)posB - boff[cb];
            const bool equal = lenA == lenB;
            const uint32_t lmax = lenA > lenB ? lenA : lenB;  // <= max_gap <= VARIANTS_MAX_GAP: at most 2048 steps
            uint32_t anyn = 0;
            for (uint32_t i = 0; i < lmax; i += 32) {
                uint64_t a = 0, bw = 0;
                uint32_t na = 0, nbm = 0;
                if (i < lenA) {
                    const uint32_t left = lenA - i;
                    a = bases_at(va, (uint64_t)posA + i) & low_bases(left);
                    na = nmask_at(va, (uint64_t)posA + i) & low_bits(left);
                }
                if (i < lenB) {
                    const uint32_t left = lenB - i;
                    b_window(vb, strand, lo, lenB, i, &bw, &nbm);
                    bw &= low_bases(left);
                    nbm &= low_bits(left);
                }
                if (i == 0) alA = a, alB = bw;
                anyn |= na | nbm;
                if (equal) {
                    const uint64_t x = a ^ bw;
                    mism += (uint32_t)__popcll(((x | (x >> 1)) & 0x5555555555555555ull) | spread_bits(na | nbm));
                }
            }
            cls = equal ? (mism == 0 ? 0u : (lenA == 1 ? 1u : 2u)) : (lenA == 0 ? 3u : (lenB == 0 ? 4u : 5u));
            const uint32_t anchor = (uint32_t)(bases_at(va, (uint64_t)posA - 1u) & 3ull);  // (posA >= p + 1)
            info = strand | (cls << 1) | (anchor << 4) | ((anyn ? 1u : 0u) << 6);
        }
        const uint64_t em = __ballot(cls >= 1 && cls <= 5);
        uint32_t mine[6];
#pragma unroll
        for (uint32_t c = 0; c < 6; ++c) mine[c] = (uint32_t)__popcll(__ballot(cls == c));
        if (lane == 0) {
#pragma unroll
            for (uint32_t c = 0; c < 6; ++c) wcls[wave][c] = mine[c];
            wcls[wave][6] = (uint32_t)__popcll(em);
        }
        __syncthreads();
        // (wlast is read before this barrier and written again behind it, wcls is read behind it and written again behind the
        // next tile's first)
        uint32_t under = 0, tile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            if (w == wave) under = tile;
            tile += wcls[w][6];
#pragma unroll
            for (uint32_t c = 0; c < 6; ++c) ncls[c] += wcls[w][c];
        }
        if (EMIT && ((em >> lane) & 1ull)) {
            const uint64_t at = voff + nrec + under + (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
            if (at < total) {
                out32[at] = posA;
                out32[total + at] = lenA;
                out32[2 * total + at] = posB;
                out32[3 * total + at] = lenB;
                out32[4 * total + at] = info;
                out32[5 * total + at] = mism;
                out64[at] = alA;
                out64[total + at] = alB;
            }
        }
        nrec += tile;
    }
    if (EMIT || tid != 0) return;  // (behind the last barrier)
    VariantChunkCount c;
    c.records = nrec;
#pragma unroll
    for (uint32_t i = 0; i < 6; ++i) c.cls[i] = ncls[i];
    c.pad = 0;
    counts[blockIdx.x] = c;
}

hipError_t launch_link_variants(hipStream_t st, const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate,
                                const uint2 *contigs, const uint2 *chunks, uint32_t nchunks, const uint64_t *boff, uint32_t nb,
                                uint32_t k, uint32_t min_run, uint32_t max_gap, uint32_t max_shift, const BlockChunkOffs *offs,
                                const SeqDesc *sdA, const uint64_t *seqwA, const uint32_t *nmwA, const SeqDesc *sdB, uint32_t ncb,
                                const uint64_t *seqwB, const uint32_t *nmwB, VariantChunkCount *counts, const uint64_t *voffs,
                                uint64_t total, uint32_t *out32, uint64_t *out64) {
    if (nchunks == 0) return hipSuccess;
    const bool emit = voffs != nullptr;
    if (!run_start || !run_end || !run_mate || !contigs || !chunks || !boff || !offs || !sdA || !seqwA || !nmwA || !sdB || !seqwB ||
        !nmwB || ncb < 1 || nb != ncb + 1 || k < 1 || k > 32 || min_run < 1 || max_gap < 1 || max_gap > VARIANTS_MAX_GAP ||
        max_shift > BLOCKS_MAX_GAP || (emit ? !(out32 && out64) : !counts))
        return hipErrorInvalidValue;
    if (emit)
        hipLaunchKernelGGL(k_link_variants<true>, dim3(nchunks), dim3(256), 0, st, run_start, run_end, run_mate, contigs, chunks, boff, nb,
                           ncb, k, min_run, max_gap, max_shift, offs, sdA, seqwA, nmwA, sdB, seqwB, nmwB, counts, voffs, total, out32,
                           out64);
    else
        hipLaunchKernelGGL(k_link_variants<false>, dim3(nchunks), dim3(256), 0, st, run_start, run_end, run_mate, contigs, chunks, boff,
                           nb, ncb, k, min_run, max_gap, max_shift, offs, sdA, seqwA, nmwA, sdB, seqwB, nmwB, counts, voffs, total,
                           out32, out64);
    return hipGetLastError();
}

}  // namespace pg
