// pg_unitigs.hip — the solid novel k-mers of a novel table (pg_novel.hip) compacted into sequences (gfx950).  The solid novel keys
// form a de Bruijn graph; its non-branching paths, the unitigs, are the novel sequences themselves: an inserted gene is one long
// unitig, a SNP against every indexed genome a bubble of two unitigs of k k-mers, a plasmid one circular unitig.  The novel table is
// only read; every lookup is key_find of pg_keytable_dev.h, every neighbour key is made in registers from the 2-bit key.
//
// Definitions (tests/unitigs_ref.py is the same over a dict of integer keys), over a novel table, its k (2 <= k <= 32) and a min_count:
//   node            a solid novel key: a canonical k-mer of the novel table with depth >= min_count.  Keys below min_count and k-mers
//                   the pan table holds are not nodes: they cut paths.
//   oriented k-mer  w: a node's k-mer x or its reverse complement; canon(w) is its node.  As a number: first base most significant,
//                   A < C < G < T — a key is the smaller of the two numbers.
//   out(w)          the bases b for which canon(w[1:] + b) is a node (0 to 4);  in(w) = out(rc(w)), complemented.
//   link byte       of node x, in the canonical orientation: bit b (b < 4) is set when canon(x[1:] + b) is a node, bit 4 + b when
//                   canon(b + x[:-1]) is a node.
//   compactable edge  w -> w': out(w) = {the base that gives w'}, in(w') holds exactly one base, canon(w) != canon(w') (no self-loop
//                   such as A..A, no hairpin w -> rc(w)), and neither node is its own reverse complement (even k only).  w -> w' is
//                   compactable iff rc(w') -> rc(w) is.
//   unitig          a maximal path w1 .. wn along compactable edges, all nodes distinct; its sequence is w1 plus the last base of each
//                   further wi: n + k - 1 bases.  A node that is its own reverse complement is a unitig of n = 1.  Every node lies
//                   in exactly one unitig.
//   circular unitig a component in which every node has a compactable edge on both sides: a simple cycle that meets every node in one
//                   orientation only.  Emitted once, from its smallest key in that key's canonical orientation, walking to the right:
//                   n nodes, n + k - 1 bases, the last k - 1 repeating the first.
//   linear unitig   has two ends; the walk that starts at the end with the smaller key emits it, for n = 1 the walk in the canonical
//                   orientation.  (The host takes the smaller of the sequence and its reverse complement.)
//   depth_sum       the sum of the nodes' depths, 64 bits.
//
// Two byte planes of nslots beside the table: `links` (the link byte of every node, 0 elsewhere) and `marks`.
//   k_unitig_links  one lane per slot, the slots cut per block as k_novel_scan cuts them.  A solid slot probes its eight neighbours —
//                   the eight home slots are loaded together, then the depths of the slots found — and stores its link byte.
//   unitig_step     THE rule, once on the device: an oriented k-mer and its link byte to the next oriented k-mer, its slot and its
//                   link byte, or "no compactable edge".
//   k_unitig_walk   count, then emit, with the host's exclusive scan of the blocks' counts between them; one lane per slot.
//                   Linear round — count: a side of a node without a compactable edge is a start (the step from the other
//                   orientation fails); the lane walks from it to the far end, learns n and the far key and decides whether it wins;
//                   the winning side (at most one per slot) goes into the slot's mark byte, the block's winners and their nodes go
//                   out.  Emit: the winners walk again for n and depth_sum, marking every node they pass (MARK_COVERED, by a
//                   32-bit atomic OR: each node has one writer, its byte's other bits are its owner's); the tile's unitigs and
//                   bases are numbered behind the walk, where every lane arrives; the winners walk a last time and write the bases.
//                   Circular round (the host runs it when the winners' nodes are fewer than the solid keys): every node not covered
//                   walks to the right until it is back at itself, keeping the smallest key seen; the lane whose own key that is
//                   wins.  Quadratic in a cycle's length, in parallel across its nodes.
// Nothing spins: a walk is bounded by `bound` (the solid keys; in the circular round the nodes not covered), a lookup by max_probe.
// A walk that reaches its bound, a neighbour the table does not hold or a link byte that contradicts the step taken raises flag[0]:
// the host answers PG_E_INTERNAL.  The walk is serial per lane by design — one key lookup and one byte per step, each an HBM miss —
// and lanes diverge in length: no wave-collective stands inside a walk loop.
// Every write to HBM is a vector store or a vector atomic.
//
// Cleaning (opt-in; tests/unitigs_clean_ref.py is the same over a dict): error tips clipped and bubbles popped before the compaction.
// Over the graph G of the current nodes, with tip_kmers T and bubble_kmers B (1 to 1024), a ratio Rm in per mille (1 to 999: strictly
// below 1, so two branches never remove each other) and a number of rounds (0 to 64):
//   side        the right side of a linear unitig U = w1 .. wn is out(wn), the left side in(w1).  A side is DEAD when that set is
//               empty, ATTACHED BY v when it holds exactly one base and the oriented k-mer v it names is a node that is none of U's
//               nodes on either strand (tested outright: the walk compares every node of U with canon(v)) and not its own reverse
//               complement; every other side is open.
//   tip         n <= T, one side dead, the other attached by v.  S = the other oriented k-mers with an edge into v on that side (a
//               held k-mer is no node: a fork whose only sibling is held has no S).  U is clipped iff S is not empty and
//               depth(attached end node) * 1000 <= Rm * max over S of depth(s), in 64 bits.  A unitig dead on both sides stays.
//   bubble      n <= B, the left side attached by p, the right side by q.  A parallel U' starts at another oriented successor
//               s != w1 of p with in(s) = {p's base}, walks to the right along compactable edges for n' <= B nodes, none of them
//               canon(p) or canon(q), and its right side is attached by the same oriented q: U' is asked of on its left side what
//               it is asked of on its right, so the rule reads the same from either end of U.  With e(X) = min(depth of X's two end
//               nodes), U is popped iff some parallel U' has e(U) * 1000 <= Rm * e(U').  p = q is nothing special; a unitig
//               parallel to its own reverse complement has equal e and stays.
//   rounds      Jacobi: every decision of round r is taken on G_r, D_r is what it drops, G_{r+1} = G_r minus D_r; the rounds stop
//               at the first empty D_r or after `rounds` of them.  The final graph is compacted as any other.
// A dropped node is no node: a third byte plane `drop` (NULL: nothing was cleaned, and every kernel does what it did without it)
// that the solid predicate of k_unitig_links (own slot and the eight neighbours), k_unitig_links_emit and k_unitig_walk honours.
//   k_unitig_clean  one lane per slot, cut as above.  READS the table, the depths and the link plane of G_r alone — a dropped node's
//                   link byte is 0 and no byte names it, so it is never a start that matters and never met — and WRITES drop bytes
//                   alone, which only the next k_unitig_links reads: a round has no race and no order.  A side that starts a unitig
//                   walks at most max(T, B) nodes and abandons beyond; the end with the smaller key decides (n = 1: side 0), as in
//                   the count pass; it classifies the two sides from the link bytes, looks up a tip's siblings (at most 3
//                   key_find) or walks a bubble's at most 3 siblings for at most B nodes each, and then walks once more to set the
//                   drop byte of U's nodes by a 32-bit atomic OR, one writer per node.  counts[4 b ..] = the block's {tips, their
//                   nodes, bubbles, their nodes}.  A contradiction between planes and table raises flag[0].
#include "pg_kernels.h"
#include "pg_keytable_dev.h"  // key_find

namespace pg {

constexpr uint32_t MARK_COVERED = 1, MARK_WIN0 = 2, MARK_WIN1 = 4, MARK_WINC = 8;  // a winner's walk passed; side 0 / side 1 / the cycle's walk wins

// what every kernel here reads: the novel table and the two planes
struct UnitigTable {
    const unsigned long long *keys;
    const uint32_t *depth;
    const uint8_t *links;
    uint64_t smask, kmask;
    uint32_t max_probe, min_count;
    int k;
    const uint8_t *drop;  // NULL: nothing was cleaned
};

// the reverse complement of an oriented k-mer (first base most significant)
__device__ __forceinline__ uint64_t rc_kmer(uint64_t w, int k, uint64_t kmask) { return ~(pair_reverse64(w) >> (64 - 2 * k)) & kmask; }
// a set of bases complemented: bit b <-> bit 3 - b
__device__ __forceinline__ uint32_t comp4(uint32_t m) { return ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3); }
// out(w) and in(w) from the link byte of canon(w); fwd: w is the canonical orientation
__device__ __forceinline__ uint32_t out_of(uint32_t link, bool fwd) { return fwd ? (link & 15u) : comp4(link >> 4); }
__device__ __forceinline__ uint32_t in_of(uint32_t link, bool fwd) { return fwd ? (link >> 4) : comp4(link & 15u); }

// the letter of a base code: A C G T
__device__ __forceinline__ uint8_t base_char(uint32_t code) { return (uint8_t)(0x54474341u >> (8 * code)); }

constexpr int STEP_NONE = 0, STEP_OK = 1, STEP_BROKEN = -1;

// the compactable edge out of w (link: the link byte of canon(w)): STEP_OK with the next oriented k-mer, its slot and its link byte;
// STEP_NONE; STEP_BROKEN when the planes contradict the table (the neighbour the link byte names is not held, or does not link back)
__device__ __forceinline__ int unitig_step(const UnitigTable &t, uint64_t w, uint32_t link, uint64_t &w2, uint32_t &slot2, uint32_t &link2) {
    const uint64_t r = rc_kmer(w, t.k, t.kmask);
    if (r == w) return STEP_NONE;  // (its own reverse complement: a unitig of 1)
    const uint32_t out = out_of(link, w < r);
    if (__popc(out) != 1) return STEP_NONE;
    w2 = ((w << 2) | (uint32_t)__builtin_ctz(out)) & t.kmask;
    const uint64_t r2 = rc_kmer(w2, t.k, t.kmask);
    const uint64_t c = min(w, r), c2 = min(w2, r2);
    if (r2 == w2 || c2 == c) return STEP_NONE;  // (a palindromic node; a self-loop or a hairpin)
    slot2 = key_find<uint32_t>(t.keys, t.smask, t.max_probe, c2, SLOT_ABSENT);
    if (slot2 == SLOT_ABSENT) return STEP_BROKEN;
    link2 = t.links[slot2];
    const uint32_t in2 = in_of(link2, w2 < r2);
    if (!((in2 >> (uint32_t)(w >> (2 * (t.k - 1)))) & 1u)) return STEP_BROKEN;  // (w's first base leads into w2)
    return __popc(in2) == 1 ? STEP_OK : STEP_NONE;
}

// the sum of v over the block's lanes (every lane reaches this; lds: 4 words; all lanes get the sum)
__device__ __forceinline__ uint64_t block_sum64(uint64_t v, unsigned long long *lds) {
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, off), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), off);
        v += (uint64_t)lo | ((uint64_t)hi << 32);
    }
    __syncthreads();  // (lds of an earlier call has been read)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// ---- the link plane ----
// block b: slots [b * per, (b + 1) * per), per = novel_scan_per_block(nslots), cut at nslots.  links[s] = the link byte of a solid
// slot, 0 of every other.  drop != NULL: a slot whose drop byte is set is no node, as a slot and as a neighbour; block_nodes != NULL:
// block_nodes[b] = the nodes of block b.
__global__ __launch_bounds__(256) void k_unitig_links(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ depth,
                                                      uint64_t nslots, uint32_t max_probe, uint32_t min_count, int k,
                                                      uint8_t *__restrict__ links, const uint8_t *__restrict__ drop,
                                                      uint32_t *__restrict__ block_nodes) {
    __shared__ unsigned long long sum_s[4];
    uint64_t mine = 0;
    const uint64_t per = novel_scan_per_block(nslots), s0 = (uint64_t)blockIdx.x * per, s1 = min(nslots, s0 + per);
    const uint64_t smask = nslots - 1, kmask = kmer_mask(k);
    for (uint64_t s = s0 + threadIdx.x; s < s1; s += 256) {
        const unsigned long long x = keys[s];
        uint32_t link = 0;
        if (x != EMPTY_KEY && depth[s] >= min_count && !(drop && drop[s])) {
            ++mine;
            // the eight neighbours' keys, their home slots loaded together; a home that holds another key walks on (key_find)
            uint64_t nb[8], home[8];
            unsigned long long at_home[8];
            uint32_t slot[8], d[8];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                nb[b] = canonical_from_le(~(((x << 2) | b) & kmask), k);                              // canon(x[1:] + b)
                nb[4 + b] = canonical_from_le(~((x >> 2) | ((uint64_t)b << (2 * (k - 1)))), k);       // canon(b + x[:-1])
            }
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                home[i] = sketch_hash(nb[i]) & smask;
                at_home[i] = keys[home[i]];
            }
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                slot[i] = at_home[i] == nb[i]     ? (uint32_t)home[i]
                          : at_home[i] == EMPTY_KEY ? SLOT_ABSENT
                                                    : key_find<uint32_t>(keys, smask, max_probe, nb[i], SLOT_ABSENT);
            }
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) d[i] = slot[i] != SLOT_ABSENT && !(drop && drop[slot[i]]) ? depth[slot[i]] : 0u;
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) link |= (d[i] >= min_count ? 1u : 0u) << i;  // (min_count >= 1: an absent key's 0 is below it)
        }
        links[s] = (uint8_t)link;
    }
    if (block_nodes) {  // (uniform over the grid: every lane reaches the barriers)
        const uint64_t all = block_sum64(mine, sum_s);
        if (threadIdx.x == 0) block_nodes[blockIdx.x] = (uint32_t)all;
    }
}

// the solid keys and their link bytes in slot order: k_novel_scan's emit pass with the link plane in the depths' place.  offs[b] =
// the solid keys of all blocks before b (the scan's count pass); entries at or past cap are never written
__global__ __launch_bounds__(256) void k_unitig_links_emit(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ depth,
                                                           const uint8_t *__restrict__ links, uint64_t nslots, uint32_t min_count,
                                                           const uint64_t *__restrict__ offs, uint64_t cap,
                                                           unsigned long long *__restrict__ out_keys, uint8_t *__restrict__ out_links,
                                                           const uint8_t *__restrict__ drop) {
    __shared__ uint32_t wsolid[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t per = novel_scan_per_block(nslots), s0 = (uint64_t)blockIdx.x * per, s1 = min(nslots, s0 + per);
    uint64_t at0 = offs[blockIdx.x];
    for (uint64_t g = s0; g < s1; g += 256) {  // (bounds uniform over the block: every lane reaches the barriers)
        const uint64_t s = g + tid;
        const unsigned long long key = s < s1 ? keys[s] : EMPTY_KEY;
        const bool solid = key != EMPTY_KEY && depth[s] >= min_count && !(drop && drop[s]);
        const uint64_t sm = __ballot(solid);
        if (lane == 0) wsolid[wave] = (uint32_t)__popcll(sm);
        __syncthreads();
        uint32_t below = 0, tile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            if (w == wave) below = tile;
            tile += wsolid[w];
        }
        if (solid) {
            const uint64_t at = at0 + below + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
            if (at < cap) {
                out_keys[at] = key;
                out_links[at] = links[s];
            }
        }
        at0 += tile;
        __syncthreads();  // (wsolid is read before the next tile writes it)
    }
}

// ---- the walks ----
// from the oriented k-mer w of slot `slot` (link: its byte) to the right.  CIRC false: along compactable edges to the far end.
// CIRC true: until the walk is back at w; a step that fails on the way is a broken plane.  n = the nodes, dsum = their depths,
// far = the far end's key (CIRC: the smallest key met).  MARK: every node passed gets MARK_COVERED.  bases != NULL: the sequence
// goes to bases[b0 ..], cut at cap.  Returns false when the planes are broken or the walk reaches `bound` nodes without its end.
template <bool CIRC, bool MARK>
__device__ __forceinline__ bool unitig_walk(const UnitigTable &t, uint64_t w, uint32_t slot, uint32_t link, uint64_t bound, uint32_t *marks,
                                            uint8_t *bases, uint64_t b0, uint64_t cap, uint64_t &n, uint64_t &dsum, uint64_t &far) {
    const uint64_t w0 = w;
    n = 1;
    dsum = t.depth[slot];
    far = min(w, rc_kmer(w, t.k, t.kmask));
    if (MARK) atomicOr(&marks[slot >> 2], MARK_COVERED << (8 * (slot & 3u)));
    if (bases)
        for (int i = 0; i < t.k; ++i)
            if (b0 + (uint64_t)i < cap) bases[b0 + i] = base_char((uint32_t)(w >> (2 * (t.k - 1 - i))) & 3u);
    for (;;) {  // (no wave-collective in here: the lanes of a wave leave at different lengths)
        uint64_t w2 = 0;
        uint32_t slot2 = 0, link2 = 0;
        const int r = unitig_step(t, w, link, w2, slot2, link2);
        if (r == STEP_BROKEN) return false;
        if (r == STEP_NONE) return !CIRC;  // (a cycle's node has an edge on both sides)
        if (CIRC && w2 == w0) return true;
        if (n >= bound) return false;
        w = w2;
        slot = slot2;
        link = link2;
        const uint64_t c = min(w, rc_kmer(w, t.k, t.kmask));
        far = CIRC ? min(far, c) : c;
        dsum += t.depth[slot];
        if (MARK) atomicOr(&marks[slot >> 2], MARK_COVERED << (8 * (slot & 3u)));
        if (bases && b0 + (uint64_t)t.k - 1 + n < cap) bases[b0 + t.k - 1 + n] = base_char((uint32_t)w & 3u);
        ++n;
    }
}

// block b: slots [b * per, (b + 1) * per) as above, a tile of 256 at a time, one lane per slot.
//   EMIT false  counts[b] = {the block's winners, their nodes}; the winning side of every slot goes into its mark byte (linear round:
//               the byte written whole, MARK_COVERED cleared; circular round: MARK_WINC added to it)
//   EMIT true   offs[b] = {the unitigs, the bases} in front of the block's (of both rounds: the circular ones stand behind the
//               linear ones).  Unitig u: offsets[u], kmers[u], depth_sum[u], circular[u] for u < cap_u; base i of the bases for
//               i < cap_b — nothing at or past a cap is written.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_unitig_walk(UnitigTable t, uint64_t nslots, uint32_t circ, uint64_t bound, uint8_t *marks8,
                                                     ulonglong2 *__restrict__ counts, const ulonglong2 *__restrict__ offs, uint64_t cap_u,
                                                     uint64_t cap_b, uint64_t *__restrict__ offsets, uint32_t *__restrict__ kmers,
                                                     uint64_t *__restrict__ depth_sum, uint8_t *__restrict__ circular,
                                                     uint8_t *__restrict__ bases, uint32_t *flag) {
    __shared__ unsigned long long sum_s[4];
    __shared__ unsigned long long wbase[4];
    __shared__ uint32_t wwin[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t per = novel_scan_per_block(nslots), s0 = (uint64_t)blockIdx.x * per, s1 = min(nslots, s0 + per);
    uint32_t *marks32 = reinterpret_cast<uint32_t *>(marks8);
    uint64_t nwin = 0, nnodes = 0;  // (count: this lane's)
    uint64_t u0 = 0, b0 = 0;        // (emit: in front of the tile)
    bool broken = false;
    if (EMIT) {
        const ulonglong2 o = offs[blockIdx.x];
        u0 = o.x;
        b0 = o.y;
    }
    for (uint64_t g = s0; g < s1; g += 256) {  // (bounds uniform over the block: every lane reaches the barriers)
        const uint64_t s = g + tid;
        const bool act = s < s1;
        const unsigned long long x = act ? t.keys[s] : EMPTY_KEY;
        const bool solid = x != EMPTY_KEY && t.depth[s] >= t.min_count && !(t.drop && t.drop[s]);
        const uint32_t link = solid ? t.links[s] : 0u;
        const uint32_t mark = act && (EMIT || circ) ? marks8[s] : 0u;
        const uint64_t xr = rc_kmer(x, t.k, t.kmask);
        uint64_t n = 0, dsum = 0, far = 0;
        if (!EMIT) {
            uint32_t win = 0;
            if (solid && !circ) {
#pragma unroll 1
                for (uint32_t side = 0; side < 2; ++side) {
                    const uint64_t w = side ? xr : x, wl = side ? x : xr;  // (wl: the orientation that walks off w's left side)
                    uint64_t w2;
                    uint32_t slot2, link2;
                    const int left = unitig_step(t, wl, link, w2, slot2, link2);
                    if (left == STEP_BROKEN) broken = true;
                    if (left != STEP_NONE) continue;
                    if (!unitig_walk<false, false>(t, w, (uint32_t)s, link, bound, nullptr, nullptr, 0, 0, n, dsum, far)) broken = true;
                    if (n == 1 ? side == 0 : x < far) {
                        win = side ? MARK_WIN1 : MARK_WIN0;
                        ++nwin;
                        nnodes += n;
                    }
                }
            } else if (solid && !(mark & MARK_COVERED)) {
                if (!unitig_walk<true, false>(t, x, (uint32_t)s, link, bound, nullptr, nullptr, 0, 0, n, dsum, far)) broken = true;
                if (far == x) {
                    win = MARK_WINC;
                    ++nwin;
                    nnodes += n;
                }
            }
            if (act) marks8[s] = (uint8_t)(circ ? (mark | win) : win);  // (this slot's owner is its byte's only writer in a count pass)
        } else {
            const uint32_t won = solid ? (mark & (circ ? MARK_WINC : (MARK_WIN0 | MARK_WIN1))) : 0u;
            const uint64_t w = (won & MARK_WIN1) ? xr : x;
            if (won) {  // once for n and depth_sum, marking the nodes passed
                const bool ok = circ ? unitig_walk<true, false>(t, w, (uint32_t)s, link, bound, nullptr, nullptr, 0, 0, n, dsum, far)
                                     : unitig_walk<false, true>(t, w, (uint32_t)s, link, bound, marks32, nullptr, 0, 0, n, dsum, far);
                if (!ok) broken = true;
            }
            // behind the walk: the tile's unitigs and bases numbered in slot order
            const uint64_t wm = __ballot(won != 0);
            uint64_t mine = won ? n + (uint64_t)t.k - 1 : 0, incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, off), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), off);
                if (lane >= (uint32_t)off) incl += (uint64_t)lo | ((uint64_t)hi << 32);
            }
            if (lane == 63) wbase[wave] = incl;
            if (lane == 0) wwin[wave] = (uint32_t)__popcll(wm);
            __syncthreads();
            uint64_t ubelow = 0, bbelow = 0, utile = 0, btile = 0;
#pragma unroll
            for (uint32_t v = 0; v < 4; ++v) {
                if (v == wave) {
                    ubelow = utile;
                    bbelow = btile;
                }
                utile += wwin[v];
                btile += wbase[v];
            }
            if (won) {
                const uint64_t u = u0 + ubelow + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull)), at = b0 + bbelow + incl - mine;
                if (u < cap_u) {
                    offsets[u] = at;
                    kmers[u] = (uint32_t)n;
                    depth_sum[u] = dsum;
                    circular[u] = circ ? 1 : 0;
                }
                if (at < cap_b) {  // the walk that writes
                    const bool ok = circ ? unitig_walk<true, false>(t, w, (uint32_t)s, link, bound, nullptr, bases, at, cap_b, n, dsum, far)
                                         : unitig_walk<false, false>(t, w, (uint32_t)s, link, bound, nullptr, bases, at, cap_b, n, dsum, far);
                    if (!ok) broken = true;
                }
            }
            u0 += utile;
            b0 += btile;
            __syncthreads();  // (wbase and wwin are read before the next tile writes them)
        }
    }
    if (broken) atomicOr(flag, 1u);
    if (!EMIT) {
        const uint64_t a = block_sum64(nwin, sum_s), b = block_sum64(nnodes, sum_s);
        if (tid == 0) counts[blockIdx.x] = make_ulonglong2(a, b);
    }
}

// ---- cleaning ----
constexpr uint64_t NO_KEY = ~0ull;  // (no canonical key: a key is at most its reverse complement, and these two add up to all ones)

// from the oriented k-mer w of slot `slot` (link: its byte) to the right along compactable edges, at most `limit` nodes: 1 with n and
// the far end (its oriented k-mer, slot and link byte), 0 when the unitig holds more, -1 when the planes are broken.  met: a node
// on the way is a1 or a2 (canonical keys, NO_KEY: none).  drop32 != NULL: every node's drop byte is set
__device__ __forceinline__ int clean_walk(const UnitigTable &t, uint64_t w, uint32_t slot, uint32_t link, uint32_t limit, uint64_t a1, uint64_t a2,
                                          uint32_t *drop32, uint32_t &n, uint64_t &wf, uint32_t &slotf, uint32_t &linkf, bool &met) {
    n = 1;
    met = false;
    for (;;) {  // (no wave-collective in here)
        const uint64_t c = min(w, rc_kmer(w, t.k, t.kmask));
        if (c == a1 || c == a2) met = true;
        if (drop32) atomicOr(&drop32[slot >> 2], 1u << (8 * (slot & 3u)));
        uint64_t w2 = 0;
        uint32_t slot2 = 0, link2 = 0;
        const int r = unitig_step(t, w, link, w2, slot2, link2);
        if (r == STEP_BROKEN) return -1;
        if (r == STEP_NONE) {
            wf = w;
            slotf = slot;
            linkf = link;
            return 1;
        }
        if (n >= limit) return 0;
        w = w2;
        slot = slot2;
        link = link2;
        ++n;
    }
}

// the right side of the oriented end e (link: the byte of canon(e)): 0 dead, 1 one successor v that is not its own reverse
// complement (attached, if v lies outside the unitig), 2 open
__device__ __forceinline__ uint32_t clean_side(const UnitigTable &t, uint64_t e, uint32_t link, uint64_t &v) {
    const uint32_t out = out_of(link, e < rc_kmer(e, t.k, t.kmask));
    if (!out) return 0;
    if (__popc(out) != 1) return 2;
    v = ((e << 2) | (uint32_t)__builtin_ctz(out)) & t.kmask;
    return rc_kmer(v, t.k, t.kmask) == v ? 2u : 1u;
}

// the tip whose attached end node is e (slot slot_e), attached by v on e's right: 1 clipped, 0 stays, -1 broken planes
__device__ __forceinline__ int clean_tip(const UnitigTable &t, uint64_t e, uint32_t slot_e, uint64_t v, uint32_t rm) {
    const uint64_t rv = rc_kmer(v, t.k, t.kmask);
    const uint32_t sv = key_find<uint32_t>(t.keys, t.smask, t.max_probe, min(v, rv), SLOT_ABSENT);
    if (sv == SLOT_ABSENT) return -1;
    const uint32_t in = in_of(t.links[sv], v < rv);
    if (!((in >> (uint32_t)(e >> (2 * (t.k - 1)))) & 1u)) return -1;
    uint32_t deepest = 0;
    bool any = false;
#pragma unroll 1
    for (uint32_t b = 0; b < 4; ++b) {
        if (!((in >> b) & 1u)) continue;
        const uint64_t s = (v >> 2) | ((uint64_t)b << (2 * (t.k - 1)));
        if (s == e) continue;
        const uint32_t ss = key_find<uint32_t>(t.keys, t.smask, t.max_probe, min(s, rc_kmer(s, t.k, t.kmask)), SLOT_ABSENT);
        if (ss == SLOT_ABSENT) return -1;
        deepest = max(deepest, t.depth[ss]);
        any = true;
    }
    return any && (uint64_t)t.depth[slot_e] * 1000ull <= (uint64_t)rm * deepest ? 1 : 0;
}

// the bubble w1 (first node, oriented) .. between p and q with e(U) = e_u: 1 popped, 0 stays, -1 broken planes
__device__ __forceinline__ int clean_bubble(const UnitigTable &t, uint64_t w1, uint64_t p, uint64_t q, uint64_t e_u, uint32_t limit, uint32_t rm) {
    const uint64_t rp = rc_kmer(p, t.k, t.kmask), cp = min(p, rp), cq = min(q, rc_kmer(q, t.k, t.kmask));
    const uint32_t sp = key_find<uint32_t>(t.keys, t.smask, t.max_probe, cp, SLOT_ABSENT);
    if (sp == SLOT_ABSENT) return -1;
    const uint32_t out = out_of(t.links[sp], p < rp);
    if (!((out >> ((uint32_t)w1 & 3u)) & 1u)) return -1;
#pragma unroll 1
    for (uint32_t b = 0; b < 4; ++b) {
        if (!((out >> b) & 1u)) continue;
        const uint64_t s = ((p << 2) | b) & t.kmask;
        if (s == w1) continue;
        const uint64_t rs = rc_kmer(s, t.k, t.kmask);
        const uint32_t ss = key_find<uint32_t>(t.keys, t.smask, t.max_probe, min(s, rs), SLOT_ABSENT);
        if (ss == SLOT_ABSENT) return -1;
        const uint32_t ls = t.links[ss];
        if (__popc(in_of(ls, s < rs)) != 1) continue;
        uint32_t n2 = 0, slotf = 0, linkf = 0;
        uint64_t wf = 0, v2 = 0;
        bool met = false;
        const int r = clean_walk(t, s, ss, ls, limit, cp, cq, nullptr, n2, wf, slotf, linkf, met);
        if (r < 0) return -1;
        if (r == 0 || met) continue;
        if (clean_side(t, wf, linkf, v2) != 1 || v2 != q) continue;
        const uint64_t e_o = min(t.depth[ss], t.depth[slotf]);
        if (e_u * 1000ull <= (uint64_t)rm * e_o) return 1;
    }
    return 0;
}

// block b: slots [b * per, (b + 1) * per) as above, one lane per slot.  counts[4 b ..] = {tips, their nodes, bubbles, their nodes}
__global__ __launch_bounds__(256) void k_unitig_clean(UnitigTable t, uint64_t nslots, uint32_t tip_kmers, uint32_t bubble_kmers, uint32_t rm,
                                                      uint8_t *drop8, uint64_t *__restrict__ counts, uint32_t *flag) {
    __shared__ unsigned long long sum_s[4];
    const uint64_t per = novel_scan_per_block(nslots), s0 = (uint64_t)blockIdx.x * per, s1 = min(nslots, s0 + per);
    uint32_t *drop32 = reinterpret_cast<uint32_t *>(drop8);
    const uint32_t longest = max(tip_kmers, bubble_kmers);
    uint64_t tips = 0, tip_nodes = 0, bubbles = 0, bubble_nodes = 0;
    bool broken = false;
    for (uint64_t s = s0 + threadIdx.x; s < s1; s += 256) {
        const uint32_t link = t.links[s];
        if (!link) continue;  // (no node, a dropped node, or a node dead on both sides: never dropped)
        const unsigned long long x = t.keys[s];
        const uint64_t xr = rc_kmer(x, t.k, t.kmask);
#pragma unroll 1
        for (uint32_t side = 0; side < 2; ++side) {
            const uint64_t w = side ? xr : x, wl = side ? x : xr;  // (wl: the orientation that walks off w's left side)
            uint64_t w2, vl = 0, vr = 0, wf = 0;
            uint32_t slot2, link2, n = 0, slotf = 0, linkf = 0;
            bool met = false;
            const int left = unitig_step(t, wl, link, w2, slot2, link2);
            if (left == STEP_BROKEN) broken = true;
            if (left != STEP_NONE) continue;
            uint32_t kl = clean_side(t, wl, link, vl);  // (vl: the reverse complement of p)
            int r = clean_walk(t, w, (uint32_t)s, link, longest, kl == 1 ? min(vl, rc_kmer(vl, t.k, t.kmask)) : NO_KEY, NO_KEY, nullptr, n, wf, slotf,
                               linkf, met);
            if (r < 0) broken = true;
            if (r <= 0) continue;
            if (!(n == 1 ? side == 0 : x < min(wf, rc_kmer(wf, t.k, t.kmask)))) continue;  // (the other end decides)
            if (kl == 1 && met) kl = 2;
            uint32_t kr = clean_side(t, wf, linkf, vr);
            if (kl == 2 || kr == 2 || kl + kr == 0) continue;
            if (kr == 1) {  // q outside U, outright
                uint32_t n1, sf1, lf1;
                uint64_t wf1;
                r = clean_walk(t, w, (uint32_t)s, link, n, min(vr, rc_kmer(vr, t.k, t.kmask)), NO_KEY, nullptr, n1, wf1, sf1, lf1, met);
                if (r <= 0) broken = true;
                if (r <= 0 || met) continue;
            }
            int hit = 0;
            const bool tip = kl + kr == 1;
            if (tip) {
                if (n > tip_kmers) continue;
                hit = kr == 1 ? clean_tip(t, wf, slotf, vr, rm) : clean_tip(t, wl, (uint32_t)s, vl, rm);
            } else {
                if (n > bubble_kmers) continue;
                hit = clean_bubble(t, w, rc_kmer(vl, t.k, t.kmask), vr, min(t.depth[s], t.depth[slotf]), bubble_kmers, rm);
            }
            if (hit < 0) broken = true;
            if (hit <= 0) continue;
            uint32_t n1, sf1, lf1;
            uint64_t wf1;
            if (clean_walk(t, w, (uint32_t)s, link, n, NO_KEY, NO_KEY, drop32, n1, wf1, sf1, lf1, met) <= 0) broken = true;
            if (tip) {
                ++tips;
                tip_nodes += n;
            } else {
                ++bubbles;
                bubble_nodes += n;
            }
        }
    }
    if (broken) atomicOr(flag, 1u);
    const uint64_t a = block_sum64(tips, sum_s), b = block_sum64(tip_nodes, sum_s), c = block_sum64(bubbles, sum_s),
                   d = block_sum64(bubble_nodes, sum_s);
    if (threadIdx.x == 0) {
        counts[4 * (uint64_t)blockIdx.x] = a;
        counts[4 * (uint64_t)blockIdx.x + 1] = b;
        counts[4 * (uint64_t)blockIdx.x + 2] = c;
        counts[4 * (uint64_t)blockIdx.x + 3] = d;
    }
}

static bool unitig_ok(const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t min_count, int k) {
    return keys && depth && nslots >= 2 && !(nslots & (nslots - 1)) && nslots <= COPIES_MAX_SLOTS && min_count >= 1 && k >= 2 && k <= 32;
}

hipError_t launch_unitig_links(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                               uint32_t min_count, int k, uint8_t *links, const uint8_t *drop, uint32_t *block_nodes) {
    if (!unitig_ok(keys, depth, nslots, min_count, k) || !links) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_unitig_links, dim3(novel_scan_blocks(nslots)), dim3(256), 0, st, keys, depth, nslots, max_probe, min_count, k, links, drop,
                       block_nodes);
    return hipGetLastError();
}

hipError_t launch_unitig_links_emit(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, const uint8_t *links, uint64_t nslots,
                                    uint32_t min_count, const uint64_t *offs, uint64_t cap, unsigned long long *out_keys, uint8_t *out_links,
                                    const uint8_t *drop) {
    if (!unitig_ok(keys, depth, nslots, min_count, 2) || !links || !offs || !out_keys || !out_links) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_unitig_links_emit, dim3(novel_scan_blocks(nslots)), dim3(256), 0, st, keys, depth, links, nslots, min_count, offs, cap,
                       out_keys, out_links, drop);
    return hipGetLastError();
}

hipError_t launch_unitig_clean(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                               uint32_t min_count, int k, const uint8_t *links, uint8_t *drop, uint32_t tip_kmers, uint32_t bubble_kmers,
                               uint32_t ratio_milli, uint64_t *counts, uint32_t *flag) {
    if (!unitig_ok(keys, depth, nslots, min_count, k) || !links || !drop || !counts || !flag || tip_kmers < 1 ||
        tip_kmers > UNITIG_CLEAN_MAX_KMERS || bubble_kmers < 1 || bubble_kmers > UNITIG_CLEAN_MAX_KMERS || ratio_milli < 1 || ratio_milli > 999)
        return hipErrorInvalidValue;
    const UnitigTable t = {keys, depth, links, nslots - 1, k == 32 ? ~0ull : ((1ull << (2 * k)) - 1), max_probe, min_count, k, nullptr};
    hipLaunchKernelGGL(k_unitig_clean, dim3(novel_scan_blocks(nslots)), dim3(256), 0, st, t, nslots, tip_kmers, bubble_kmers, ratio_milli, drop,
                       counts, flag);
    return hipGetLastError();
}

hipError_t launch_unitig_walk(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                              uint32_t min_count, int k, const uint8_t *links, uint8_t *marks, bool circular, uint64_t bound, ulonglong2 *counts,
                              const ulonglong2 *offs, uint64_t cap_unitigs, uint64_t cap_bases, uint64_t *offsets, uint32_t *kmers,
                              uint64_t *depth_sum, uint8_t *circ_out, uint8_t *bases, uint32_t *flag, const uint8_t *drop) {
    const bool emit = offs != nullptr;
    if (!unitig_ok(keys, depth, nslots, min_count, k) || !links || !marks || !flag || bound < 1 || (emit ? false : !counts))
        return hipErrorInvalidValue;
    if (emit && ((cap_unitigs && (!offsets || !kmers || !depth_sum || !circ_out)) || (cap_bases && !bases))) return hipErrorInvalidValue;
    const UnitigTable t = {keys, depth, links, nslots - 1, k == 32 ? ~0ull : ((1ull << (2 * k)) - 1), max_probe, min_count, k, drop};
    const uint32_t blocks = novel_scan_blocks(nslots);
    if (emit)
        hipLaunchKernelGGL(k_unitig_walk<true>, dim3(blocks), dim3(256), 0, st, t, nslots, circular ? 1u : 0u, bound, marks, counts, offs,
                           cap_unitigs, cap_bases, offsets, kmers, depth_sum, circ_out, bases, flag);
    else
        hipLaunchKernelGGL(k_unitig_walk<false>, dim3(blocks), dim3(256), 0, st, t, nslots, circular ? 1u : 0u, bound, marks, counts, offs,
                           cap_unitigs, cap_bases, offsets, kmers, depth_sum, circ_out, bases, flag);
    return hipGetLastError();
}

}  // namespace pg
