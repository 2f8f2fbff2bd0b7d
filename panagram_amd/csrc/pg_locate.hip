// pg_locate.hip — WHERE in a genome G do query sequences Q lie (gfx950)?  pg_synteny.hip answers that for k-mers unique on both
// sides and writes a mate word per position of the streamed side; here only Q must hold a k-mer once, G is streamed through the
// table and nothing but the collinear runs of its hits is written: a genome of any size, every copy of a query.
//
// Definitions (tests/locate_ref.py is the same in numpy):
//   table      a position table (pg_synteny.hip) whose side 1 holds the queries Q; side 0 is ignored.
//   hit word   of k-mer position p of contig c of a streamed sequence set G: defined when the window is valid and the side-1
//              field w of its canonical key is a position (neither POS_EMPTY nor POS_MULTI): h = w ^ rcG = posQ << 1 | (rcG ^ rcQ),
//              posQ global in Q's contigs laid end to end.  NO_MATE otherwise.  Nothing is asked of the key's multiplicity in G.
//   hit run    the run of pg_synteny.hip with hit words in place of mates: a maximal [a, b) of consecutive k-mer positions of
//              ONE contig of G, each continuing its predecessor under mate_continues (pg_postable_dev.h).  Contig edges of G cut
//              runs.  For k >= 2 a run lies inside one query: the global Q positions of two neighbouring contigs' k-mers differ
//              by at least k.
// Positions of G are contig-relative everywhere: G's total is unlimited, one contig holds at most 2^32 - 1 k-mer positions.
//   k_hit_runs  the run scan of pg_runscan.h over chunks of LOCATE_CHUNK positions of one contig; a position's value is its hit
//               word, from a probe (the walk of k_pos_mates without its condition on side 0), the halo ONE extra probe of
//               position c0 - 1.  With H = hit, P = predecessor hit, C = continues:
//                 run starts  H & ~C        run ends (exclusive)  P & ~C, and one at the contig's end when its last is a hit
//               counts[chunk] = {hits, starts, ends, 0}; beside a start goes its hit word.
// Both passes probe: the table is only read, so both see the same words.  The table's policy stands in pg_keytable_dev.h; the
// walk here is key_find's, kept as a copy of its own in hit_word for its speed.  No atomics; every write to HBM is a vector store.
#include "pg_kernels.h"

#include "pg_postable_dev.h"  // PosSlot, kmer_key_rc, mate_continues; with it pg_keytable_dev.h
#include "pg_runscan.h"

namespace pg {

// the hit word of position p of a contig (p below its k-mer positions).  (The view by value: by reference the kernel comes out
// a few instructions different.)
__device__ __forceinline__ uint32_t hit_word(int k, const ContigView v, uint64_t p, const PosSlot *__restrict__ slots, uint64_t smask,
                                             uint32_t max_probe) {
    if (!window_valid(v, p, k)) return NO_MATE;
    uint64_t key;
    const uint32_t rc = kmer_key_rc(v.seqw, p, k, key) ? 1u : 0u;
    // key_find's walk (pg_keytable_dev.h), written out: through key_find this kernel was up to 2 % slower on the MI355X, whether the
    // word was read behind the walk or handed back by it (profiles/keytable_ab.txt); as it stands here its assembly is what it was.
    // A change to the table's policy comes here too.
    uint64_t s = sketch_hash(key) & smask;
    for (uint32_t probes = 0; probes < max_probe; ++probes, s = (s + 1) & smask) {
        const unsigned long long cur = slots[s].key;
        if (cur == EMPTY_KEY) break;
        if (cur != key) continue;
        const uint32_t w = slots[s].word[1];
        return w != POS_EMPTY && w != POS_MULTI ? w ^ rc : NO_MATE;
    }
    return NO_MATE;
}

// chunk = {contig, first position}: a contig of at least k bases, 0 <= first position < its k-mer positions
template <bool EMIT>
__global__ __launch_bounds__(256) void k_hit_runs(int k, const SeqDesc *__restrict__ sd, const uint2 *__restrict__ chunks,
                                                  const uint64_t *seqw_all, const uint32_t *nmw_all, const uint32_t *has_n,
                                                  const PosSlot *__restrict__ slots, uint64_t nslots, uint32_t max_probe,
                                                  uint4 *__restrict__ counts, const ulonglong2 *__restrict__ offs, uint64_t total,
                                                  uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_end,
                                                  uint32_t *__restrict__ run_hit) {
    const uint2 ck = chunks[blockIdx.x];
    const ContigView v = contig_view(sd, ck.x, seqw_all, nmw_all, has_n, k);
    const uint64_t smask = nslots - 1;
    // positions in 64 bits: nk <= 2^32 - 1, but c0 + LOCATE_CHUNK may pass 2^32
    const uint64_t c0 = ck.y;
    // the chunk's halo: the hit word of position c0 - 1 (every lane the same probe: broadcast loads)
    const uint32_t halo = c0 > 0 ? hit_word(k, v, c0 - 1, slots, smask, max_probe) : NO_MATE;
    const ulonglong2 off = EMIT ? offs[blockIdx.x] : make_ulonglong2(0, 0);
    const uint4 c = chunk_runs<EMIT, LOCATE_CHUNK>(
        c0, v.nkmers, NO_MATE, halo, off, total, [&](uint64_t j) { return hit_word(k, v, j, slots, smask, max_probe); },
        [](bool act, uint32_t prev, uint32_t h, bool &starts, bool &ends) {
            const bool cont = act && mate_continues(prev, h);
            starts = act && h != NO_MATE && !cont;
            ends = act && prev != NO_MATE && !cont;
        },
        [](uint32_t tail) { return tail != NO_MATE; }, [](uint32_t h) { return h != NO_MATE; }, no_tally(),
        [&](uint64_t at, uint64_t j, uint32_t, uint32_t h) {
            run_start[at] = (uint32_t)j;
            run_hit[at] = h;
        },
        [&](uint64_t at, uint64_t j, uint32_t, uint32_t) { run_end[at] = (uint32_t)j; });
    if (!EMIT && threadIdx.x == 0) counts[blockIdx.x] = c;
}

hipError_t launch_hit_runs(hipStream_t st, int k, const SeqDesc *sd, const uint2 *chunks, uint32_t nchunks, const uint64_t *seqw,
                           const uint32_t *nmw, const uint32_t *has_n, const void *slots, uint64_t nslots, uint32_t max_probe,
                           uint4 *counts, const ulonglong2 *offs, uint64_t total, uint32_t *run_start, uint32_t *run_end,
                           uint32_t *run_hit) {
    if (nchunks == 0) return hipSuccess;
    const bool emit = offs != nullptr;
    if (k < 1 || k > 32 || nslots == 0 || (nslots & (nslots - 1)) || !slots || !sd || !chunks || !seqw || !nmw || !has_n ||
        (emit ? (!run_start || !run_end || !run_hit) : !counts))
        return hipErrorInvalidValue;
    const PosSlot *ps = static_cast<const PosSlot *>(slots);
    if (emit)
        hipLaunchKernelGGL(k_hit_runs<true>, dim3(nchunks), dim3(256), 0, st, k, sd, chunks, seqw, nmw, has_n, ps, nslots, max_probe,
                           counts, offs, total, run_start, run_end, run_hit);
    else
        hipLaunchKernelGGL(k_hit_runs<false>, dim3(nchunks), dim3(256), 0, st, k, sd, chunks, seqw, nmw, has_n, ps, nslots, max_probe,
                           counts, offs, total, run_start, run_end, run_hit);
    return hipGetLastError();
}

}  // namespace pg
