// pg_anchor.hip — the anchor hot path on gfx950 (CDNA4, wave64): integer / HBM-bound, no MFMA.
//
// Replaces (reference, kjenike/panagram): KMC CKMCFile::GetCountersForRead as called from
// KMCdb::write_bits (cpp/anchor.cpp:112-195) and Genome._write_bitmap / _query_kmc_bytes
// (index.py:932-969).  What reads the finished rows — the statistics pass and its side paths — is pg_rows.hip.
//
// Instruction count per position is what bounds k_probe once the table fetches are shared between
// neighbouring positions (minimizer homes) and between the anchor genomes of a pangenome
// (co-scheduled tiles):
//
//   k_probe      ONE WAVE = one tile of TILE consecutive k-mer positions, no barriers, 4.6 KB of LDS
//                (32 waves per CU).  Per batch of 64 lanes (lane = one position, neighbours =
//                neighbouring positions):
//                  * canonical k-mer from the LDS-staged 2-bit sequence (~0.25 B/pos from HBM)
//                  * minimizer = sliding minimum over the W_C m-mer ranks of the neighbouring
//                    lanes (DPP wave shifts) -> home line; runs of equal home line are found with
//                    one ballot (leaders) and numbered with mbcnt
//                  * LDS-STAGED PROBE BATCH: the batch's distinct table lines (~15 for 58
//                    positions) are fetched cooperatively and coalesced — 8 lanes x 16 B = one
//                    128-byte line — into a per-wave LDS buffer, then every lane scans the 8
//                    slots of ITS line out of LDS
//                  * the presence row goes straight to bitmap.1; a key absent from a FULL line
//                    joins the tile's in-wave overflow queue (position, next line, step), which
//                    drain_queue works off in dense 64-entry batches, level by level
//
// Bytes from HBM per position: 0.25 (sequence) + 128 x (lines missed in L2 per
// position: 0.34 with one launch per genome, 0.095 co-scheduled) + row bytes written + re-read.
#include "pg_kernels.h"

// ---- translation units (round 6) ----
// k_probe and k_insert_tile are instantiated per minimizer window (0, 3..8) x row mode x layout x (fused): 320 kernels, three
// minutes of hipcc in one unit.  panagram_amd/build.py compiles this file THREE times in parallel, each unit instantiating the
// windows of its part (probe_part<N> / insert_part<N> below); part 0 also holds the two launchers and the preload.
// -1 (the default: tools/isa.sh, a -DPG_PHASE_TIMING build, a plain `hipcc pg_anchor.hip`): everything in one unit.
#ifndef PG_ANCHOR_PART
#define PG_ANCHOR_PART -1
#endif
#define PG_HAS_PART(n) (PG_ANCHOR_PART == -1 || PG_ANCHOR_PART == (n))
#define PG_MAIN_PART (PG_ANCHOR_PART <= 0)
#if defined(PG_PHASE_TIMING) && PG_ANCHOR_PART != -1
#error "a -DPG_PHASE_TIMING build keeps its counters in one device variable: compile pg_anchor.hip as ONE unit (PG_ANCHOR_PART unset)"
#endif

namespace pg {

// windows 0, 3, 4 -> part 0; 5, 6 -> part 1; 7, 8 -> part 2
hipError_t probe_part0(hipStream_t s, uint32_t w, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                       const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig, const uint32_t *sched, uint32_t tile_base, uint8_t *out1,
                       uint32_t nbytes, const RowCols &rc, int rowmode, const FuseArgs *fuse);
hipError_t probe_part1(hipStream_t s, uint32_t w, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                       const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig, const uint32_t *sched, uint32_t tile_base, uint8_t *out1,
                       uint32_t nbytes, const RowCols &rc, int rowmode, const FuseArgs *fuse);
hipError_t probe_part2(hipStream_t s, uint32_t w, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                       const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig, const uint32_t *sched, uint32_t tile_base, uint8_t *out1,
                       uint32_t nbytes, const RowCols &rc, int rowmode, const FuseArgs *fuse);
hipError_t insert_part0(hipStream_t s, uint32_t win, uint32_t ntiles, const SubTable &st, int w, uint32_t bits, uint32_t count_mode, const uint64_t *seqw,
                        const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd, const uint32_t *tile0, uint32_t ncontigs,
                        unsigned long long *counters, uint32_t max_probe);
hipError_t insert_part1(hipStream_t s, uint32_t win, uint32_t ntiles, const SubTable &st, int w, uint32_t bits, uint32_t count_mode, const uint64_t *seqw,
                        const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd, const uint32_t *tile0, uint32_t ncontigs,
                        unsigned long long *counters, uint32_t max_probe);
hipError_t insert_part2(hipStream_t s, uint32_t win, uint32_t ntiles, const SubTable &st, int w, uint32_t bits, uint32_t count_mode, const uint64_t *seqw,
                        const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd, const uint32_t *tile0, uint32_t ncontigs,
                        unsigned long long *counters, uint32_t max_probe);
hipError_t preload_part1();
hipError_t preload_part2();

constexpr int PROBE_SEQW = ((PROBE_TILE + 31) / 32 + 6 + 3) & ~3;  // staged 32-base words per tile
// The tile's packed bases are staged TWICE: as they are (sw) and reverse-complemented (rw: base j of rw = complement of
// base 32 PROBE_SEQW - 1 - j of sw).  The reverse complement of the k-mer at base p is then the k bases of rw from
// 32 PROBE_SEQW - p - k on — the same three LDS reads and two funnel shifts as the forward window, instead of a
// 64-bit bit reversal, pair swap, complement and shift per position (14 instructions).
#ifndef PG_ABLATE
#define PG_ABLATE 0  // timing experiments of k_probe (tools/ab_ablate.sh); 0 = the product
#endif
constexpr uint32_t PROBE_SEQ_BASES = 32u * PROBE_SEQW;
// k_probe's workgroup is ONE wave: what its lanes hand each other through LDS (the staged lines, the batch's line numbers, the
// overflow queue) needs no barrier, and a __syncthreads() there costs an s_waitcnt lgkmcnt(0).  The barriers say what is
// meant; wavefront-scope fences in their place changed no timing: profiles/r6z_ab_wave_sync.txt.
// -DPG_PHASE_TIMING: a measuring build (tools/phase_timing.py) — every wave of k_probe stamps s_memtime at its phase
// boundaries and adds the phases' cycles to pg_phase_cycles at the end of its tile: where a wave's time goes, waits for
// the other waves of its SIMD included.  Slots: 0 prologue, 1 front end, 2 wait for the lines, 3 staging, 4 issue of the
// next fetch, 5 slot scan, 6 row store, 7 loop bookkeeping, 8 drain + tail, 9 waves, 10 overflow entries.
#ifdef PG_PHASE_TIMING
__device__ unsigned long long pg_phase_cycles[1024 * 16];  // (1024 sets, by block number: ten same-address atomics per wave serialise the launch)
#define PG_PH_DECL uint32_t ph_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; uint32_t ph_t = (uint32_t)__builtin_readcyclecounter();
#define PG_PH(i) { const uint32_t ph_n = (uint32_t)__builtin_readcyclecounter(); ph_acc[i] += ph_n - ph_t; ph_t = ph_n; }
#define PG_PH_FLUSH { if (threadIdx.x == 0) { for (int ph_i = 0; ph_i < 9; ++ph_i) atomicAdd(&pg_phase_cycles[(blockIdx.x & 1023u) * 16u + ph_i], (unsigned long long)ph_acc[ph_i]); atomicAdd(&pg_phase_cycles[(blockIdx.x & 1023u) * 16u + 9], 1ull); atomicAdd(&pg_phase_cycles[(blockIdx.x & 1023u) * 16u + 10], (unsigned long long)ph_acc[10]); } }
#else
#define PG_PH_DECL
#define PG_PH(i)
#define PG_PH_FLUSH
#endif
// (rcb = PROBE_SEQ_BASES - k, handed in: written as PROBE_SEQ_BASES - p - k the compiler adds p and k per position first)
__device__ __forceinline__ uint64_t revcomp_window(const uint64_t *rw, uint32_t p, uint64_t kmask, uint32_t rcb) {
    return extract_bases32(reinterpret_cast<const uint32_t *>(rw), rcb - p) & kmask;
}

// scan the 8 slots of a line staged in LDS.  Lines fill front to back without holes (an insert
// claims the first EMPTY slot and slots never revert), so "full" == last slot used.
// returns 1 = found, 0 = absent (line not full), -1 = absent from a full line
// A table line {key, m0, m1} x SLOTS is staged into LDS as SLOTS keys followed by SLOTS mask pairs: the scan then takes its
// keys in SLOTS / 2 ds_read_b128 — 4 LDS cycles per 16 bytes and lane — where one ds_read2_b64 per two slots of the
// interleaved line took 8 (MI355X_MICROARCH.md, LDS table): 16 instead of 32 LDS cycles per batch for the 8 keys, the
// largest single item of a batch's ~95.  The staging lane's 16-byte chunk leaves as two 8-byte stores (6 + 6 cycles
// against 13 for the one ds_write_b128).
__device__ __forceinline__ void stage_chunk(uint4 *line, uint32_t slot, int slots, const uint4 v) {
    uint2 *const p = reinterpret_cast<uint2 *>(line);
    p[slot] = make_uint2(v.x, v.y);
    p[slots + slot] = make_uint2(v.z, v.w);
}
template <bool TWO, int SLOTS>
__device__ __forceinline__ int scan_line_lds(const uint4 *line, uint64_t key, uint32_t &m0, uint32_t &m1) {
    // all SLOTS key reads are issued together (one LDS wait); one compare per slot into a scalar lane mask;
    // the scalar unit folds the masks into the three bits of the hit slot's number (at most one slot holds the
    // key), three v_cndmask turn them into the slot's byte offset, and only that slot's masks are read
    uint64_t kk[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS / 2; ++j) {
        const uint4 v = line[j];
        kk[2 * j] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        kk[2 * j + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    constexpr uint32_t SLOT_BYTES = 8u, MASK0 = 8u * SLOTS;  // a slot's masks: MASK0 + 8 * slot
    m0 = m1 = 0;
    if constexpr (SLOTS == 8) {
        // (ballot of a compare = v_cmp_eq_u64 with a scalar destination; inverse_ballot = the SGPR pair used as a
        // v_cndmask selector / exec mask: the compiler's lowering of `kk == key ? sl : hit` goes through VCC with
        // two VALU instructions and a wait state per slot)
        unsigned long long e[8];
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) e[sl] = __builtin_amdgcn_ballot_w64(kk[sl] == key);
        const unsigned long long b0 = e[1] | e[3] | e[5] | e[7], b1 = e[2] | e[3] | e[6] | e[7], b2 = e[4] | e[5] | e[6] | e[7];
        const unsigned long long any = b0 | b1 | b2 | e[0];
        const bool hit = __builtin_amdgcn_inverse_ballot_w64(any);
#if PG_ABLATE == 6  // (timing experiment: keys read and compared, the hit slot's mask word NOT read)
        if (hit) m0 = (uint32_t)b0 | 1u;
        return hit ? 1 : (kk[SLOTS - 1] == EMPTY_KEY ? 0 : -1);
#elif PG_ABLATE == 7  // (timing experiment: keys read, one compare instead of eight)
        m0 = (uint32_t)(kk[0] ^ kk[1] ^ kk[2] ^ kk[3] ^ kk[4] ^ kk[5] ^ kk[6] ^ kk[7]) | 1u;
        return (kk[0] ^ kk[3]) == key ? -1 : 1;
#endif
        if (hit) {
            const uint32_t off = (__builtin_amdgcn_inverse_ballot_w64(b0) ? SLOT_BYTES : 0u) | (__builtin_amdgcn_inverse_ballot_w64(b1) ? 2u * SLOT_BYTES : 0u) |
                                 (__builtin_amdgcn_inverse_ballot_w64(b2) ? 4u * SLOT_BYTES : 0u);
            if constexpr (TWO) {
                const uint2 mk = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint8_t *>(line) + off + MASK0);
                m0 = mk.x;
                m1 = mk.y;
            } else {
                m0 = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(line) + off + MASK0);
            }
        }
        return hit ? 1 : (kk[SLOTS - 1] == EMPTY_KEY ? 0 : -1);
    } else {
        int hit = -1;
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) hit = (kk[sl] == key) ? sl : hit;
        if (hit >= 0) {
            const uint2 mk = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint8_t *>(line) + (uint32_t)hit * SLOT_BYTES + MASK0);
            m0 = mk.x;
            if (TWO) m1 = mk.y;
        }
        return hit >= 0 ? 1 : (kk[SLOTS - 1] == EMPTY_KEY ? 0 : -1);
    }
}

// (a scan without control flow was within 0.5 %: profiles/r4e_ab_probe_scalar_cuts.txt)

// ---- byte-mask layout (up to 8 genomes: two halves of seven bare keys + seven mask bytes, pg_device.h) ----
// The line is staged as it is; a lane scans the half of its key: four ds_read_b128 bring the seven keys AND, in the eighth word,
// their mask bytes.  Seven compares into scalar lane masks, folded on the scalar unit into the three bits of the hit's slot number
// as in scan_line_lds; the hit's byte is cut out of the two mask dwords in registers — no second LDS read.
// the mask byte of slot b0 + 2 b1 + 4 b2 out of the half's eighth word {lo: the bytes of slots 0..3, hi: of slots 4..6}
__device__ __forceinline__ uint32_t bm_pick(uint32_t lo, uint32_t hi, bool b0, bool b1, bool b2) {
    const uint32_t sel = b2 ? hi : lo;
    const uint32_t sh = (b0 ? 8u : 0u) | (b1 ? 16u : 0u);
    return __builtin_amdgcn_ubfe(sel, sh, 8u);
}
// returns 1 = found, 0 = absent (half not full), -1 = absent from a full half
// FIRST: several slots may hold the key (k_insert_tile's snapshots, see scan_keys16_lds) — the LOWEST one counts; slot: its number within the half
template <bool FIRST = false>
__device__ __forceinline__ int scan_line_bm(const uint4 *line, uint64_t key, uint32_t &m0, uint32_t *slot = nullptr) {
    const uint4 *half = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(line) + half_offset_of_key(key));
    const uint4 v0 = half[0], v1 = half[1], v2 = half[2], v3 = half[3];
    const uint64_t kk[7] = {(uint64_t)v0.x | ((uint64_t)v0.y << 32), (uint64_t)v0.z | ((uint64_t)v0.w << 32), (uint64_t)v1.x | ((uint64_t)v1.y << 32),
                            (uint64_t)v1.z | ((uint64_t)v1.w << 32), (uint64_t)v2.x | ((uint64_t)v2.y << 32), (uint64_t)v2.z | ((uint64_t)v2.w << 32),
                            (uint64_t)v3.x | ((uint64_t)v3.y << 32)};
    unsigned long long e[7];
#pragma unroll
    for (int sl = 0; sl < 7; ++sl) e[sl] = __builtin_amdgcn_ballot_w64(kk[sl] == key);
    if constexpr (FIRST) {
        unsigned long long seen = e[0];
#pragma unroll
        for (int sl = 1; sl < 7; ++sl) {
            const unsigned long long m = e[sl];
            e[sl] = m & ~seen;
            seen |= m;
        }
    }
    const unsigned long long b0 = e[1] | e[3] | e[5], b1 = e[2] | e[3] | e[6], b2 = e[4] | e[5] | e[6];
    const bool hit = __builtin_amdgcn_inverse_ballot_w64(b0 | b1 | b2 | e[0]);
    m0 = 0;
    if (hit) {
        const bool h0 = __builtin_amdgcn_inverse_ballot_w64(b0), h1 = __builtin_amdgcn_inverse_ballot_w64(b1), h2 = __builtin_amdgcn_inverse_ballot_w64(b2);
        m0 = bm_pick(v3.z, v3.w, h0, h1, h2);
        if (slot) *slot = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u);
    }
    return hit ? 1 : (kk[6] == EMPTY_KEY ? 0 : -1);
}
// the half of one line straight from global memory (four 16-byte loads in flight)
__device__ __forceinline__ int scan_line_global_bm(const SubTable &st, uint32_t b, uint64_t key, uint32_t &m0) {
    const uint4 *half = reinterpret_cast<const uint4 *>(st.buckets + (uint64_t)b * 128u + half_offset_of_key(key));
    const uint4 v[4] = {half[0], half[1], half[2], half[3]};
    const uint64_t mb = (uint64_t)v[3].z | ((uint64_t)v[3].w << 32);  // the seven mask bytes
    m0 = 0;
    bool hit = false;
#pragma unroll
    for (int sl = 0; sl < 7; ++sl) {
        const uint64_t kk = (sl & 1) ? ((uint64_t)v[sl / 2].z | ((uint64_t)v[sl / 2].w << 32)) : ((uint64_t)v[sl / 2].x | ((uint64_t)v[sl / 2].y << 32));
        const bool h = kk == key;
        m0 = h ? (uint32_t)(mb >> (8 * sl)) & 0xFFu : m0;
        hit |= h;
    }
    const uint64_t last = (uint64_t)v[3].x | ((uint64_t)v[3].y << 32);
    return hit ? 1 : (last == EMPTY_KEY ? 0 : -1);
}

// one line straight from global memory: the 8 slot loads are issued together (one latency)
template <bool TWO, int SLOTS>
__device__ __forceinline__ int scan_line_global(const SubTable &st, uint32_t b, uint64_t key, uint32_t &m0, uint32_t &m1) {
    const uint4 *line = reinterpret_cast<const uint4 *>(st.buckets + (uint64_t)b * (16 * SLOTS));
    uint4 v[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) v[sl] = line[sl];
    m0 = m1 = 0;
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const uint64_t kk = (uint64_t)v[sl].x | ((uint64_t)v[sl].y << 32);
        const bool hit = (kk == key);
        m0 = hit ? v[sl].z : m0;
        if (TWO) m1 = hit ? v[sl].w : m1;
    }
    const uint64_t last = (uint64_t)v[SLOTS - 1].x | ((uint64_t)v[SLOTS - 1].y << 32);
    return (m0 | m1) ? 1 : (last == EMPTY_KEY ? 0 : -1);
}

// follow a key's probe sequence from its line number `level` (b, step) to the end
template <bool TWO, int SLOTS, bool BM = false>
__device__ __forceinline__ void lane_chase(const SubTable &st, uint64_t key, uint32_t level, uint32_t b, uint32_t step,
                                           uint32_t &m0, uint32_t &m1) {
    for (uint64_t n = 0; n < st.nbuckets + GROUP_CHAIN; ++n) {
        if constexpr (BM) {
            m1 = 0;
            if (scan_line_global_bm(st, b, key, m0) >= 0) return;
        } else if (scan_line_global<TWO, SLOTS>(st, b, key, m0, m1) >= 0) return;
        level = min(level + 1, GROUP_CHAIN + 1);
        advance_line(key, level, st.nbuckets, b, step);
    }
    m0 = m1 = 0;
}

// ---- split layout (more than 64 genomes: 16 bare keys per line, mask words in a second array) ----
// A hit is reported as (line, slot + 1) — slot1 == 0: absent — and the row is copied from the mask array afterwards.
// scan of a key line staged in LDS: 1 = found, 0 = absent (line not full), -1 = absent from a full line
// FIRST: several slots may hold the key (k_insert_tile's snapshots: a claim that is about to be retired, see
// wave_insert_batch) — report the lowest; otherwise at most one does
template <bool FIRST = false>
__device__ __forceinline__ int scan_keys16_lds(const uint4 *line, uint64_t key, uint32_t &slot1) {
    uint64_t kk[16];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint4 v = line[c];
        kk[2 * c] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        kk[2 * c + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    unsigned long long e[16];
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) e[sl] = __builtin_amdgcn_ballot_w64(kk[sl] == key);
    if constexpr (FIRST) {  // (scalar unit: a lane's match in a lower slot masks its later ones)
        unsigned long long seen = e[0];
#pragma unroll
        for (int sl = 1; sl < 16; ++sl) {
            const unsigned long long m = e[sl];
            e[sl] = m & ~seen;
            seen |= m;
        }
    }
    unsigned long long b[4] = {0, 0, 0, 0}, any = e[0];
#pragma unroll
    for (int sl = 1; sl < 16; ++sl) {
        any |= e[sl];
#pragma unroll
        for (int bit = 0; bit < 4; ++bit)
            if (sl & (1 << bit)) b[bit] |= e[sl];
    }
    const bool hit = __builtin_amdgcn_inverse_ballot_w64(any);
    slot1 = 0;
    if (hit)
        slot1 = 1u + ((__builtin_amdgcn_inverse_ballot_w64(b[0]) ? 1u : 0u) | (__builtin_amdgcn_inverse_ballot_w64(b[1]) ? 2u : 0u) |
                      (__builtin_amdgcn_inverse_ballot_w64(b[2]) ? 4u : 0u) | (__builtin_amdgcn_inverse_ballot_w64(b[3]) ? 8u : 0u));
    return hit ? 1 : (kk[15] == EMPTY_KEY ? 0 : -1);
}

// follow a key's probe sequence through key lines in global memory (16 key loads in flight per line)
__device__ __forceinline__ void lane_chase_wide(const SubTable &st, uint64_t key, uint32_t level, uint32_t b, uint32_t step,
                                                uint32_t &hline, uint32_t &slot1) {
    hline = slot1 = 0;
    for (uint64_t n = 0; n < st.nbuckets + GROUP_CHAIN; ++n) {
        const uint4 *line = reinterpret_cast<const uint4 *>(st.buckets + (uint64_t)b * (8u * SPLIT_KEYS));
        uint4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = line[c];
        uint32_t found = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (((uint64_t)v[c].x | ((uint64_t)v[c].y << 32)) == key) found = 2 * c + 1;
            if (((uint64_t)v[c].z | ((uint64_t)v[c].w << 32)) == key) found = 2 * c + 2;
        }
        if (found) {
            hline = b;
            slot1 = found;
            return;
        }
        if (((uint64_t)v[7].z | ((uint64_t)v[7].w << 32)) == EMPTY_KEY) return;  // line not full: absent
        level = min(level + 1, GROUP_CHAIN + 1);
        advance_line(key, level, st.nbuckets, b, step);
    }
}

// the row of a position: the W mask words of (line, slot1 - 1), or zeros (slot1 == 0); nbytes = ceil(N / 8).
// Rows and mask blocks are contiguous, so the copy goes in the widest pieces the width allows — one dwordx4 / x3 /
// x2 access per lane covers the wave's rows back to back (word-by-word stores at a 12- or 20-byte lane stride
// ran 2x slower); only 4-byte alignment is needed for them (gfx950 global memory takes unaligned wide accesses).
template <int NW>
struct __attribute__((packed, aligned(4))) WordsN {
    uint32_t w[NW];
};
template <int NW, bool NT = false>
__device__ __forceinline__ void copy_words(const uint32_t *src, uint8_t *dst, bool hit) {
    WordsN<NW> v;
#pragma unroll
    for (int i = 0; i < NW; ++i) v.w[i] = 0;
    if (hit) v = *reinterpret_cast<const WordsN<NW> *>(src);
    if constexpr (NW == 4 && NT) {  // (non-temporal, like the 8-byte rows of store_row)
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 q = {v.w[0], v.w[1], v.w[2], v.w[3]};
        __builtin_nontemporal_store(q, reinterpret_cast<u32x4 *>(dst));
    } else {
        *reinterpret_cast<WordsN<NW> *>(dst) = v;
    }
}
template <int NS>  // NS whole words and `tail` bytes of the next one: NS + 1 words in one load
__device__ __forceinline__ void copy_words_tail(const uint32_t *src, uint8_t *dst, bool hit, uint32_t tail) {
    WordsN<NS + 1> v;
#pragma unroll
    for (int i = 0; i <= NS; ++i) v.w[i] = 0;
    if (hit) v = *reinterpret_cast<const WordsN<NS + 1> *>(src);
    if constexpr (NS > 0) {
        WordsN<NS> o;
#pragma unroll
        for (int i = 0; i < NS; ++i) o.w[i] = v.w[i];
        *reinterpret_cast<WordsN<NS> *>(dst) = o;
    }
    if (NS > 0 && tail > 1) {  // (wave-uniform) the last 4 bytes of the row as one dword that overlaps the words before it — equal
                               // bytes — instead of 2 or 3 single bytes (15-byte rows: 13.6 ps per position, 12- and 16-byte rows 9.5-9.8)
        struct __attribute__((packed)) U32 { uint32_t v; };
        reinterpret_cast<U32 *>(dst + 4 * NS + tail - 4)->v = __builtin_amdgcn_alignbit(v.w[NS], v.w[NS > 0 ? NS - 1 : 0], 8u * tail);
    } else {
        for (uint32_t bb = 0; bb < tail; ++bb) dst[4 * NS + bb] = (uint8_t)(v.w[NS] >> (8 * bb));
    }
}
__device__ __forceinline__ void store_row_wide(const uint8_t *masks, uint32_t W, uint32_t nbytes, uint8_t *row, uint32_t hline,
                                               uint32_t slot1) {
    const bool hit = slot1 != 0;
    const uint32_t *mp = reinterpret_cast<const uint32_t *>(masks) + ((uint64_t)hline * SPLIT_KEYS + (slot1 - 1u)) * W;
    uint32_t d = 0;
    const uint32_t full = nbytes / 4;  // (wave-uniform loop bounds)
    const uint32_t tail = nbytes % 4;  // bytes of a last, partial word: fetched with the piece before it (one request)
    if (nbytes == 16) {  // (wave-uniform) the whole row in one store: non-temporal
        copy_words<4, true>(mp, row, hit);
        return;
    }
    for (; d + 4 <= full; d += 4) copy_words<4>(mp + d, row + 4 * d, hit);
    if (!tail) {
        if (full - d == 3) copy_words<3>(mp + d, row + 4 * d, hit);
        else if (full - d == 2) copy_words<2>(mp + d, row + 4 * d, hit);
        else if (full - d == 1) copy_words<1>(mp + d, row + 4 * d, hit);
    } else {
        if (full - d == 3) copy_words_tail<3>(mp + d, row + 4 * d, hit, tail);
        else if (full - d == 2) copy_words_tail<2>(mp + d, row + 4 * d, hit, tail);
        else if (full - d == 1) copy_words_tail<1>(mp + d, row + 4 * d, hit, tail);
        else copy_words_tail<0>(mp + d, row + 4 * d, hit, tail);
    }
}

// ---- inline layout (65..128 genomes, round 5): a line = S bare keys (S = 6 at W = 3 mask words, 5 at W = 4) followed by the slots'
// mask blocks; staged whole like a split-layout key line, but a hit's mask words come out of the SAME staged line ----
// scan of a staged line: 1 = found, 0 = absent (line not full), -1 = absent from a full line; slot1 = slot + 1 (0: absent).
// The hit's slot number stays on the vector unit (one compare + one select per key; from the last key down, so that the lowest
// match stays — k_insert_tile's snapshots may show a claim that is about to be retired).  Words 5.. of the line that hold mask
// bits (S = 5) are not compared.
__device__ __forceinline__ int scan_keys_inl(const uint4 *line, uint64_t key, uint32_t S, uint32_t &slot1) {
    uint64_t kk[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint4 v = line[c];
        kk[2 * c] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        kk[2 * c + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    const bool six = S >= 6u;  // (wave-uniform)
    slot1 = (six && kk[5] == key) ? 6u : 0u;
#pragma unroll
    for (int sl = 4; sl >= 0; --sl) slot1 = (kk[sl] == key) ? (uint32_t)(sl + 1) : slot1;
    const uint64_t last = six ? kk[5] : kk[4];
    return slot1 ? 1 : (last == EMPTY_KEY ? 0 : -1);
}
// the W (3 or 4) mask words of slot `slot` out of a staged line: four words from byte 8 S + 4 W slot on (W = 3: the fourth is the
// next slot's first word or the line's pad — rows of W = 3 tables are at most 12 bytes, it is never stored)
__device__ __forceinline__ void masks_inl(const uint4 *line, uint32_t S, uint32_t W, uint32_t slot, uint32_t (&w)[4]) {
    const WordsN<4> v = *reinterpret_cast<const WordsN<4> *>(reinterpret_cast<const uint8_t *>(line) + 8u * S + 4u * W * slot);
    w[0] = v.w[0], w[1] = v.w[1], w[2] = v.w[2], w[3] = v.w[3];
}
// a row of 9..16 bytes out of registers (zeros for an absent key): the widest pieces the width allows, as store_row_wide
template <int NS>
__device__ __forceinline__ void store_words_tail(const uint32_t (&v)[4], uint8_t *dst, uint32_t tail) {
    if (NS == 3 && tail == 0) {  // (wave-uniform) a 12-byte row is one store: non-temporal (profiles/r5m_ab_row_fuse.txt)
        typedef uint32_t u32x3 __attribute__((ext_vector_type(3), aligned(4)));
        u32x3 q = {v[0], v[1], v[2]};
        __builtin_nontemporal_store(q, reinterpret_cast<u32x3 *>(dst));
        return;
    }
    WordsN<NS> o;
#pragma unroll
    for (int i = 0; i < NS; ++i) o.w[i] = v[i];
    *reinterpret_cast<WordsN<NS> *>(dst) = o;
    if (tail > 1) {  // (wave-uniform) the row's last 4 bytes as one dword that overlaps the words before it — equal bytes
        struct __attribute__((packed)) U32 { uint32_t v; };
        reinterpret_cast<U32 *>(dst + 4 * NS + tail - 4)->v = __builtin_amdgcn_alignbit(v[NS & 3], v[NS - 1], 8u * tail);
    } else if (tail == 1) {
        dst[4 * NS] = (uint8_t)v[NS & 3];
    }
}
__device__ __forceinline__ void store_row_regs(uint8_t *row, uint32_t nbytes, const uint32_t (&w)[4]) {
    if (nbytes == 16) {  // (wave-uniform) one store covers the row: non-temporal, as store_row_wide
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 q = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(q, reinterpret_cast<u32x4 *>(row));
    } else if (nbytes >= 12) {
        store_words_tail<3>(w, row, nbytes - 12u);
    } else {
        store_words_tail<2>(w, row, nbytes - 8u);
    }
}
// A ragged row (9..11 or 13..15 bytes) as ONE store: the 12 or 16 bytes from the row's start on = the row and the first bytes of the
// NEXT row, which the next lane holds (one DPP shift of its first word) — overlapping stores of one instruction write equal bytes.
// A lane whose successor has no row in this batch writes zeros there: the next batch's own store, later in this wave's program
// order, puts them right — so not for the tile's last batch (the bytes behind its last row are another wave's), and not for the
// rows the overflow drain resolves (store_row_regs: exact).  Two stores per row at odd addresses cost the probe of 65 genomes
// 8 % against the one store of 12-byte rows (7.6 against 7.0 ps per position).
// The store is non-temporal (profiles/r5m_ab_row_fuse.txt).  Rows of three bytes (one unaligned dword) and of 5..7 bytes (one 8-byte
// store) are written the same way: see k_probe's row store.
// nxt: the first row word of the lane above (0 where that lane has no row), taken by the caller with every lane active
__device__ __forceinline__ void store_row_fused(uint8_t *row, uint32_t nbytes, const uint32_t (&w)[4], uint32_t nxt) {
    const uint32_t t = nbytes & 3u;  // (wave-uniform, 1..3) bytes of the row's last word
    const uint32_t keep = (1u << (8u * t)) - 1u;
    typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
    typedef uint32_t u32x3u __attribute__((ext_vector_type(3), aligned(1)));
    if (nbytes > 12u) {
        u32x4u q = {w[0], w[1], w[2], (w[3] & keep) | (nxt << (8u * t))};
        __builtin_nontemporal_store(q, reinterpret_cast<u32x4u *>(row));
    } else {
        u32x3u q = {w[0], w[1], (w[2] & keep) | (nxt << (8u * t))};
        __builtin_nontemporal_store(q, reinterpret_cast<u32x3u *>(row));
    }
}
// follow a key's probe sequence through inline-layout lines in global memory (all six key words of a line in flight together)
__device__ __forceinline__ void lane_chase_inl(const SubTable &st, uint64_t key, uint32_t level, uint32_t b, uint32_t step, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (uint64_t n = 0; n < st.nbuckets + GROUP_CHAIN; ++n) {
        const uint8_t *base = st.buckets + (uint64_t)b * 128u;
        const uint4 *line = reinterpret_cast<const uint4 *>(base);
        uint4 v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = line[c];
        const uint64_t kk[6] = {(uint64_t)v[0].x | ((uint64_t)v[0].y << 32), (uint64_t)v[0].z | ((uint64_t)v[0].w << 32),
                                (uint64_t)v[1].x | ((uint64_t)v[1].y << 32), (uint64_t)v[1].z | ((uint64_t)v[1].w << 32),
                                (uint64_t)v[2].x | ((uint64_t)v[2].y << 32), (uint64_t)v[2].z | ((uint64_t)v[2].w << 32)};
        uint32_t found = 0;
#pragma unroll
        for (int sl = 5; sl >= 0; --sl)
            if ((uint32_t)sl < st.slots && kk[sl] == key) found = (uint32_t)sl + 1u;
        if (found) {
            const uint32_t *mp = reinterpret_cast<const uint32_t *>(base + 8u * st.slots) + (found - 1u) * st.W;
#pragma unroll
            for (int i = 0; i < 4; ++i)  // (static indices: the words stay in registers)
                if ((uint32_t)i < st.W) w[i] = mp[i];
            return;
        }
        if ((st.slots >= 6u ? kk[5] : kk[4]) == EMPTY_KEY) return;  // line not full: absent
        level = min(level + 1, GROUP_CHAIN + 1);
        advance_line(key, level, st.nbuckets, b, step);
    }
}

// write the row bytes this sub-table owns: low nb0 bytes of m0 at column col0, low nb1 bytes of
// m1 at col0+4 (cpp/anchor.cpp:139-164).  ROWMODE 1: one-byte rows; 2: 8-byte rows (N = 64);
// 0: generic byte loop.
template <int ROWMODE>
__device__ __forceinline__ void store_row(uint8_t *row, uint32_t m0, uint32_t m1, const RowCols rc) {
    // Rows of 8 and of 16 bytes are written NON-TEMPORALLY: they are not read again before the statistics pass, and as
    // ordinary stores they push table lines out of the L2 (64 x 20 Mb k=21 8.1-8.4 -> 7.8 ms, k=31 7.22 -> 6.98,
    // 128 genomes 14.0-14.7 -> 13.1-13.9; profiles/r2_ab_nt_rows.txt).  Only where ONE store instruction covers the
    // row, so that a wave writes whole lines: one- and four-byte rows lose 3-5 % that way, rows of two 16-byte pieces
    // 25 % (256 genomes: 24.8 -> 32.2 ms — each piece leaves the L2 as a partial line); two- and four-byte rows lose
    // 13-15 % (profiles/r5m_ab_row_fuse.txt).
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    if (ROWMODE == 1) {
        row[0] = (uint8_t)m0;
    } else if (ROWMODE == 4) {  // four-byte rows (25..32 genomes): one aligned dword
        *reinterpret_cast<uint32_t *>(row) = m0;
    } else if (ROWMODE == 5) {  // two-byte rows (9..16 genomes)
        *reinterpret_cast<uint16_t *>(row) = (uint16_t)m0;
    } else if (ROWMODE == 6) {  // three-byte rows (17..24 genomes): two stores at byte alignment
        struct __attribute__((packed)) U16 { uint16_t v; };
        reinterpret_cast<U16 *>(row)->v = (uint16_t)m0;
        row[2] = (uint8_t)(m0 >> 16);
    } else if (ROWMODE == 2 || rc.words == 4) {  // (rc.words == 4: both words at an 8-byte aligned column: one store)
        u32x2 q = {m0, m1};
        uint8_t *p = row + (ROWMODE == 2 ? 0u : rc.col0);
        __builtin_nontemporal_store(q, reinterpret_cast<u32x2 *>(p));
    } else if  (rc.words == 1) {  // wave-uniform
        *reinterpret_cast<uint32_t *>(row + rc.col0) = m0;
        if (rc.nb1) *reinterpret_cast<uint32_t *>(row + rc.col0 + 4) = m1;
    } else if (rc.words == 2) {  // two-byte rows (9..16 genomes): one aligned 16-bit store
        *reinterpret_cast<uint16_t *>(row) = (uint16_t)m0;
    } else if (rc.words == 3) {  // rows of 3, 5, 6 or 7 bytes: two stores at byte alignment (gfx950 global
                                 // memory takes unaligned dword / short accesses), not one per byte
        struct __attribute__((packed)) U32 { uint32_t v; };
        struct __attribute__((packed)) U16 { uint16_t v; };
        const uint32_t nb = rc.nb0 + rc.nb1;  // wave-uniform
        if (nb == 3) {
            reinterpret_cast<U16 *>(row)->v = (uint16_t)m0;
            row[2] = (uint8_t)(m0 >> 16);
        } else {
            reinterpret_cast<U32 *>(row)->v = m0;
            if (nb == 5) row[4] = (uint8_t)m1;
            else if (nb == 6) reinterpret_cast<U16 *>(row + 4)->v = (uint16_t)m1;
            else reinterpret_cast<U32 *>(row + 3)->v = (m0 >> 24) | (m1 << 8);  // bytes 3..6 (byte 3 again)
        }
    } else {
        for (uint32_t bb = 0; bb < rc.nb0; ++bb) row[rc.col0 + bb] = (uint8_t)(m0 >> (8 * bb));
        for (uint32_t bb = 0; bb < rc.nb1; ++bb) row[rc.col0 + 4 + bb] = (uint8_t)(m1 >> (8 * bb));
    }
}

// value of lane-1 (lane 0 keeps its own): one DPP move (wave_shr:1) on the VALU instead of a
// ds_bpermute round trip through the LDS crossbar
__device__ __forceinline__ uint32_t lane_up1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
// lanes whose value differs from that of the lane below, as a lane mask: an xor whose first source is the DPP shift (a fast
// VOP2 instruction; gfx950 has no DPP form of the compares) and a compare with zero — a move, the shift and a compare
// before.  Lane 0 has no lane below: its bit is arbitrary — callers OR the mask with one that has bit 0 set, or ignore
// lane 0.  (s_nop 1: a DPP source written by the VALU instruction before needs two wait states.)
__device__ __forceinline__ unsigned long long differs_from_lane_below(uint32_t v) {
    uint32_t t;
    asm("s_nop 1\n\tv_xor_b32_dpp %0, %1, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "=&v"(t) : "v"(v));
    return __builtin_amdgcn_ballot_w64(t != 0u);
}
// Sliding minimum over the last W lanes (lanes below W-1 see shorter windows): m <- min(own, m of the lane below),
// W-1 times, each step ONE instruction — the DPP shift is the min's own source modifier; lane 0, which has no lane
// below, is left alone and keeps its m.  6 instructions for W = 7 where shuffle-doubling took 6 moves + 3 min +
// 3 selects.  (s_nop 1: a DPP source written by the previous VALU instruction needs two wait states; one asm
// block, so that the compiler does not pad every step once more)
#define PG_DPPMIN "s_nop 1\n\tv_min_u32_dpp %0, %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
template <int W>
__device__ __forceinline__ uint32_t sliding_min(uint32_t x) {
    uint32_t m = x;
    if constexpr (W == 2) asm(PG_DPPMIN : "+v"(m) : "v"(x));
    if constexpr (W == 3) asm(PG_DPPMIN PG_DPPMIN : "+v"(m) : "v"(x));
    if constexpr (W == 4) asm(PG_DPPMIN PG_DPPMIN PG_DPPMIN : "+v"(m) : "v"(x));
    if constexpr (W == 5) asm(PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN : "+v"(m) : "v"(x));
    if constexpr (W == 6) asm(PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN : "+v"(m) : "v"(x));
    if constexpr (W == 7) asm(PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN : "+v"(m) : "v"(x));
    if constexpr (W == 8) asm(PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN PG_DPPMIN : "+v"(m) : "v"(x));
    static_assert(W >= 1 && W <= 8, "minimizer window");
    return m;
}
#undef PG_DPPMIN
// ---- batches without halo lanes -----------------------------------------------------------------------------------
// A position's minimizer is the minimum over the W m-mers of its k-mer: its own (the last one) and the W - 1 before it,
// which the W - 1 lanes below own.  The first W - 1 lanes of a batch have too few lanes below them; round 1-4 made them
// HALO lanes — they only supplied m-mers, and a batch brought 64 - (W - 1) new positions (57 of 64 lanes at W = 7).
// Instead (van Herk's two halves of a window): the window of lane j < W - 1 = the last W - 1 - j m-mers before the batch
// (a suffix minimum over them) and the first j + 1 of this one (what the sliding minimum yields for a lane with fewer
// than W - 1 lanes below).  One ds_bpermute brings the W - 1 m-mer ranks before the NEXT batch's first position — they
// sit in consecutive lanes of this one — down to lanes 0 .. W - 2 (the carry; the other lanes hold ~0 once it is
// used); their suffix minima take three row-local DPP steps there (a window of eight, cut off where the ~0 begin),
// interleaved with the next batch's own sliding minimum, which takes them in with one v_min: up to 64 new positions
// per batch for about eight instructions.
// (wave priorities by phase of a batch, s_setprio, changed nothing: profiles/r4e_ab_setprio.txt)
// r[l] = min(x[l .. min(l + 7, last lane of l's row of 16)])
__device__ __forceinline__ uint32_t suffix_min8_row(uint32_t x) {
    uint32_t r = x;
    asm("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shl:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shl:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shl:4 row_mask:0xf bank_mask:0xf"
        : "+v"(r));
    return r;
}
// the sliding minimum of x AND, in place, the suffix minima of a second vector (the carry): two dependent chains
// interleaved (a DPP source written by a VALU instruction needs two wait states: the other chain's step is one of them)
// (the sliding step as min(m, m of the lane below) — a window of t + 1 from two windows of t — needs no third operand: the
// vector itself can then be the register the suffix chain works in; an input operand equal to a read-write one may be
// given the SAME register by the compiler, and was)
#define PG_F "v_min_u32_dpp %0, %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define PG_S(n) "v_min_u32_dpp %1, %1, %1 row_shl:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define PG_N0 "s_nop 0\n\t"
#define PG_N1 "s_nop 1\n\t"
template <int W>
__device__ __forceinline__ uint32_t sliding_min_suffix(uint32_t x, uint32_t &suffix) {
    uint32_t m = x, r = suffix;
    static_assert(W >= 2 && W <= 8, "minimizer window");
    if constexpr (W == 2) asm(PG_N1 PG_F PG_S(1) PG_N1 PG_S(2) PG_N1 PG_S(4) : "+v"(m), "+v"(r));
    if constexpr (W == 3) asm(PG_N1 PG_F PG_S(1) PG_N0 PG_F PG_S(2) PG_N1 PG_S(4) : "+v"(m), "+v"(r));
    if constexpr (W == 4) asm(PG_N1 PG_F PG_S(1) PG_N0 PG_F PG_S(2) PG_N0 PG_F PG_S(4) : "+v"(m), "+v"(r));
    if constexpr (W == 5) asm(PG_N1 PG_F PG_S(1) PG_N0 PG_F PG_S(2) PG_N0 PG_F PG_S(4) PG_N0 PG_F : "+v"(m), "+v"(r));
    if constexpr (W == 6) asm(PG_N1 PG_F PG_S(1) PG_N0 PG_F PG_S(2) PG_N0 PG_F PG_S(4) PG_N0 PG_F PG_N1 PG_F : "+v"(m), "+v"(r));
    if constexpr (W == 7) asm(PG_N1 PG_F PG_S(1) PG_N0 PG_F PG_S(2) PG_N0 PG_F PG_S(4) PG_N0 PG_F PG_N1 PG_F PG_N1 PG_F : "+v"(m), "+v"(r));
    if constexpr (W == 8) asm(PG_N1 PG_F PG_S(1) PG_N0 PG_F PG_S(2) PG_N0 PG_F PG_S(4) PG_N0 PG_F PG_N1 PG_F PG_N1 PG_F PG_N1 PG_F : "+v"(m), "+v"(r));
    suffix = r;
    return m;
}
#undef PG_F
#undef PG_S
#undef PG_N0
#undef PG_N1
// base + (set bits of `mask` at lanes <= this lane) - 1: for a lane whose own bit is set, its index among the set lanes
// (a queue slot, counted from the wave-uniform `base`); for any lane, the number of the last set lane at or below it (a
// run id, when the set lanes are the runs' first lanes).  Two VALU instructions: the shift of the mask by one lane —
// which turns mbcnt's "below this lane" into "at or below" — and the constant are scalar work, and the constant rides in
// on mbcnt's own addend.
__device__ __forceinline__ uint32_t lanes_le_index(unsigned long long mask, uint32_t base) {
    const unsigned long long m1 = mask >> 1;
    const uint32_t c = base + (uint32_t)(mask & 1ull) - 1u;
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, c));
}

// run ids: (set lanes of `lmask` at or below this lane) - 1 — lanes_le_index(lmask, 0) — with NO scalar instruction: mbcnt counts
// the set lanes BELOW (its addend -1 is an inline constant), and a lane's own bit comes in as the carry of v_addc_co_u32,
// whose carry-in operand is a lane mask in an SGPR pair
__device__ __forceinline__ uint32_t run_ids(unsigned long long lmask) {
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(lmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lmask, ~0u));
    uint32_t rid;
    unsigned long long carry_out;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(rid), "=s"(carry_out) : "v"(below), "s"(lmask));
    return rid;
}
// for a lane whose own bit of `mask` is set: base + its index among the set lanes = base + the set lanes BELOW it, which is
// what mbcnt counts as it is — none of lanes_le_index's scalar shifts (a scalar instruction costs k_probe's launch what a
// vector one does: profiles/r4e_probe_dummy_salu.txt)
__device__ __forceinline__ uint32_t set_lane_index(unsigned long long mask, uint32_t base) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, base));
}

// ROWMODE 3 — the genome-sharded mode's narrow tables (a block of up to 8 genomes): the probe emits the block's
// COMPACT BIT COLUMNS directly — per tile TILE_SLOTS x u64 per genome, bit l of word s = position 64 s + l — instead of one-byte
// rows that k_cols_extract would read back: the tile's columns are assembled in LDS (one ballot per genome and batch,
// shifted to the batch's place by the scalar unit; positions resolved by the overflow levels OR their bits in) and
// written once, 64 bytes per genome and tile.  (COLS_G, TILE_SLOTS: pg_kernels.h)
__device__ __forceinline__ void cols_or_position(unsigned long long *cols, uint32_t pl, uint32_t m0) {
    while (m0) {  // (rare path: a lane per resolved position, an LDS atomic per set bit)
        const uint32_t j = (uint32_t)__ffs((int)m0) - 1u;
        m0 &= m0 - 1u;
        atomicOr(&cols[(pl >> 6) * COLS_G + j], 1ull << (pl & 63u));
    }
}

// Overflow levels of a tile: dense 64-entry batches out of the wave's LDS queue, staged exactly
// like the main batches (neighbouring entries belong to the same group and share their next
// line); entries that overflow again are compacted in place for the next level.
// LEVELS: overflow levels worked off with staged lines; entries still unresolved after them chase their sequences lane
// by lane.  Two for many-genome tables (narrow windows, big groups: a third of the overflowing keys overflow again); ONE
// for the wide-window tables of up to 16 genomes, where the second staged level costs more than the few lanes it saves
// (+1.5 % at configs 1-2, tools/ab_one.sh; -1 % at 64 genomes).
template <bool TWO, int ROWMODE, int SLOTS, int MAXRUN, bool WIDE, int LEVELS, bool INL = false, bool BM = false>
__device__ __forceinline__ void drain_queue(const SubTable &st, uint32_t qn, const uint64_t *sw, const uint64_t *rw, uint32_t *q_grp,
                                            uint16_t *q_pl, uint32_t *lines_w, uint4 *buf,
                                            uint8_t *tile_rows, uint32_t nbytes, const RowCols rc, int lane) {
    // a queue entry is (group, position in the tile): SIX bytes of LDS.  The key is taken from the tile's sequence words
    // again, and the line and step of the entry's level are functions of the group, the key and the level (line_of_level,
    // pg_device.h) — worked out here, in the drain's dense batches.  (18 bytes per entry let the kernel run 26 waves per CU,
    // 10 bytes 32 with a queue of 192 entries; six bytes make that 320 entries in the same LDS.)
    const int k = (int)st.k;
    constexpr int LDS_LINE_U4 = SLOTS + 1;
    constexpr int STAGE_ITERS = (MAXRUN * SLOTS + 63) / 64;
    const uint8_t *chunk_base = st.buckets + (uint32_t)(lane % SLOTS) * 16u;
    const uint32_t lbytes = BM ? st.W * 128u : INL ? st.layout * 64u : st.slots * (WIDE ? 8u : 16u);  // (= 16 * SLOTS = 128, as a run-time scalar: see k_probe)
    static_assert(LEVELS >= 1, "k_probe's entries (group, position) get their line and step from level 1's staged batches");
    for (int level = 1; qn > 0; ++level) {
        __syncthreads();
        if (level > LEVELS) {
            // the few entries still unresolved (long chains) walk their sequences lane by lane:
            // 8 slot loads in flight per line, no staging overhead
            for (uint32_t e = lane; e < qn; e += 64) {
                uint32_t m0, m1;
                const uint64_t key = canonical_from_le(extract_bases(sw, q_pl[e]), k);
                uint32_t cl, cs;  // the line this level tries and the step of its sequence
                line_of_level(q_grp[e], key, (uint32_t)level, st.nbuckets, cl, cs);
                if constexpr (WIDE && INL) {
                    uint32_t rw4[4];
                    lane_chase_inl(st, key, (uint32_t)level, cl, cs, rw4);
                    if (rw4[0] | rw4[1] | rw4[2] | rw4[3]) store_row_regs(tile_rows + (uint64_t)q_pl[e] * nbytes, nbytes, rw4);
                } else if constexpr (WIDE) {
                    lane_chase_wide(st, key, (uint32_t)level, cl, cs, m0, m1);
                    if (m1) store_row_wide(st.masks, st.W, nbytes, tile_rows + (uint64_t)q_pl[e] * nbytes, m0, m1);
                } else {
                    lane_chase<TWO, SLOTS, BM>(st, key, (uint32_t)level, cl, cs, m0, m1);
                    if constexpr (ROWMODE == 3) cols_or_position(reinterpret_cast<unsigned long long *>(tile_rows), q_pl[e], m0);
                    else if (m0 | m1) store_row<ROWMODE>(tile_rows + (uint64_t)q_pl[e] * nbytes, m0, m1, rc);
                }
            }
            break;
        }
        uint32_t kept = 0;
        for (uint32_t i0 = 0; i0 < qn; i0 += 64) {
            const uint32_t e = i0 + lane;
            const bool act = e < qn;
            const uint32_t ec = act ? e : qn - 1;
            const uint32_t grp = q_grp[ec];
            const uint32_t pl = q_pl[ec];
            const uint64_t kmask = kmer_mask(k);
            const uint64_t X = extract_bases32(reinterpret_cast<const uint32_t *>(sw), pl) & kmask;
            const uint64_t key = canonical_from_xb(X, revcomp_window(rw, pl, kmask, PROBE_SEQ_BASES - (uint32_t)k), k);
            uint32_t line, step;
            if constexpr (LEVELS < (int)GROUP_CHAIN) {  // (the staged levels end before the group's chain does: none of the key's own hashing here)
                line = home_of_group(grp, st.nbuckets);
                step = step_of_group(grp, st.nbuckets);
                for (int i = 0; i < level; ++i) line = next_line(line, step, st.nbuckets);  // (wave-uniform: once or twice)
            } else {
                line_of_level(grp, key, (uint32_t)level, st.nbuckets, line, step);
            }
            const uint32_t prev_line = lane_up1(line);
            const bool leader = act && (lane == 0 || line != prev_line);
            const unsigned long long lmask = __builtin_amdgcn_ballot_w64(leader);
            const uint32_t rid = lanes_le_index(lmask, 0u);
            const uint32_t nruns = (uint32_t)__popcll(lmask);
            uint32_t m0 = 0, m1 = 0;
            [[maybe_unused]] uint32_t rw4[4] = {0, 0, 0, 0};  // (inline layout: the row's words)
            int rcode = 0;
            // (staging as in k_probe's main batches: the entries behind the last run repeat the first run's line, every lane
            // reads its entries at fixed places, one multiply-add per address)
            const uint32_t padline = lmask ? (uint32_t)__builtin_amdgcn_readlane((int)line, __builtin_ctzll(lmask)) : 0u;
            for (uint32_t r0 = 0; r0 < nruns; r0 += MAXRUN) {
                const uint32_t nl = min((uint32_t)MAXRUN, nruns - r0);
                if (lane < MAXRUN) lines_w[lane] = padline;
                if (leader && rid - r0 < nl) lines_w[rid - r0] = line;
                __syncthreads();
                uint4 v[STAGE_ITERS];
                uint32_t ln[STAGE_ITERS];
#pragma unroll
                for (int u = 0; u < STAGE_ITERS; ++u) ln[u] = lines_w[u * (64 / SLOTS) + lane / SLOTS];
#pragma unroll
                for (int u = 0; u < STAGE_ITERS; ++u) v[u] = *reinterpret_cast<const uint4 *>(chunk_base + (uint64_t)ln[u] * lbytes);
#pragma unroll
                for (int u = 0; u < STAGE_ITERS; ++u) {
                    const uint32_t idx = u * 64 + lane;
                    if constexpr (WIDE || BM) buf[(idx / SLOTS) * LDS_LINE_U4 + (idx % SLOTS)] = v[u];  // (bare keys: as they are)
                    else stage_chunk(buf + (idx / SLOTS) * LDS_LINE_U4, idx % SLOTS, SLOTS, v[u]);
                }
                __syncthreads();
                if (act && rid - r0 < nl) {
                    if constexpr (WIDE && INL) {
                        rcode = scan_keys_inl(buf + (rid - r0) * LDS_LINE_U4, key, st.slots, m1);
                        if (m1) masks_inl(buf + (rid - r0) * LDS_LINE_U4, st.slots, st.W, m1 - 1u, rw4);
                    } else if constexpr (WIDE) {
                        rcode = scan_keys16_lds(buf + (rid - r0) * LDS_LINE_U4, key, m1);
                        m0 = line;
                    } else if constexpr (BM) {
                        rcode = scan_line_bm(buf + (rid - r0) * LDS_LINE_U4, key, m0);
                    } else {
                        rcode = scan_line_lds<TWO, SLOTS>(buf + (rid - r0) * LDS_LINE_U4, key, m0, m1);
                    }
                }
                __syncthreads();
            }
            const bool again = act && rcode < 0;
            if constexpr (WIDE && INL) {
                if (act && m1) store_row_regs(tile_rows + (uint64_t)pl * nbytes, nbytes, rw4);
            } else if constexpr (WIDE) {
                if (act && m1) store_row_wide(st.masks, st.W, nbytes, tile_rows + (uint64_t)pl * nbytes, m0, m1);
            } else {
                if constexpr (ROWMODE == 3) {
                    if (act) cols_or_position(reinterpret_cast<unsigned long long *>(tile_rows), pl, m0);
                } else {
                    if (act && (m0 | m1)) store_row<ROWMODE>(tile_rows + (uint64_t)pl * nbytes, m0, m1, rc);
                }
            }
            const unsigned long long kmask2 = __builtin_amdgcn_ballot_w64(again);
            if (again) {  // in-place compaction: slot <= e, and this batch's reads are already done
                const uint32_t slot = set_lane_index(kmask2, kept);
                q_grp[slot] = grp;  // (the same two fields: the next level derives its own line)
                q_pl[slot] = (uint16_t)pl;
            }
            kept += (uint32_t)__popcll(kmask2);
            __syncthreads();
        }
        qn = kept;
    }
}

// ---------------------------------------------------------------------------
// Fused statistics (round 6; FuseArgs in pg_kernels.h): the END of a tile inside k_probe.  The statistics pass read every row
// again from HBM — a quarter of the step at 65-128 genomes, 102 GB at BASELINE configs[3] — although each wave has just
// written its tile's rows (at most 16 KB): here the wave reads them back while they are still in the L2 / Infinity Cache and
// leaves the tile's counters, 0.4-5 % of the row bytes, for k_tile_reduce to add up.  Nothing of this touches the batch loop:
// no register, no LDS byte and no instruction of it (the tile's descriptors are loaded again at the end, so that the loop
// keeps no more values alive than the unfused kernel's).  Extra VALU work at the tile's end is cheap where it matters: 48
// extra instructions per batch cost the probe of 65 / 128 genomes 0.6 %, of 27 / 64 genomes 9 % (profiles/r6b_elasticity.txt).
//   rows        16 per lane (row j * 64 + lane of the tile, j = 0..15), each ONE load of ceil(nbytes / 4) dwords at its byte
//               offset (gfx950 takes unaligned dword accesses), L1 bypassed (sc1: the L2 is where the wave's stores are)
//   histogram   popcount -> (bin of the row relative to the tile's first, popcount): one LDS add of 1 << 16 * (index & 1) to a
//               packed pair of u16 counters, four copies by lane & 3 (a tile has 1024 rows: no field overflows)
//   column sums sixteen rows per word through a Harley-Seal carry-save tree (15 adders: 45 instructions) into five bit
//               planes, transposed to byte counters and summed over the lanes by a halving exchange (k_epilogue's vflush)
//   bitmap.100  the tile's rows at multiples of 100 (eleven at most), copied byte by byte by the first lanes
// The reference does all of this in its scatter loop (cpp/anchor.cpp:156-183); the column sums are index.py:1051's.
// ---------------------------------------------------------------------------
#ifndef PG_FUSE_LOAD_SC1
#define PG_FUSE_LOAD_SC1 1  // 0: the row read-back with the default cache policy (experiment)
#endif
// NW (1..4) dwords from byte `off` of the tile's rows (any byte alignment: gfx950 takes unaligned dword accesses), as agent-scope
// loads of 8 and 4 bytes — sc1: served by the L2, where the wave's stores are, whatever the L1 holds — with the tile's base
// address in a scalar register pair.  (A buffer descriptor would do the same in one instruction for three or four words, but its
// four scalar registers do not survive in the wide instantiations, which are held to 80: the compiler then keeps it in vector
// registers and wraps every load in a readfirstlane loop.)
typedef const __attribute__((address_space(1))) uint8_t *GlobalBytes;  // (a pointer the compiler knows to be global memory: global_load with a scalar base, not flat_load)
template <int NW>
__device__ __forceinline__ void fuse_load_row(GlobalBytes base, uint32_t off, uint32_t (&w)[NW]) {
    GlobalBytes p = base + off;
#if PG_FUSE_LOAD_SC1
#pragma unroll
    for (int i = 0; i + 1 < NW; i += 2) {
        const unsigned long long v = __hip_atomic_load(reinterpret_cast<const __attribute__((address_space(1))) unsigned long long *>(p + 4 * i), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        w[i] = (uint32_t)v, w[i + 1] = (uint32_t)(v >> 32);
    }
    if constexpr (NW & 1)
        w[NW - 1] = __hip_atomic_load(reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(p + 4 * (NW - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    const WordsN<NW> v = *reinterpret_cast<const __attribute__((address_space(1))) WordsN<NW> *>(p);
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = v.w[i];
#endif
}
// the five bit planes of one row word (bit c of plane i = bit i of the number of the lane's 16 rows that hold column c) -> the
// tile's 32 column counters of that word, two u16 per output word: entry e (0..15) = columns e and e + 16
__device__ __forceinline__ void fuse_flush_word(const uint32_t (&pl)[5], uint32_t *out16, int lane) {
    uint32_t R[16];
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // byte b of v counts column 8 b + q (16 at most)
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) v |= ((pl[i] >> q) & 0x01010101u) << i;
        R[2 * q] = v & 0x00FF00FFu;
        R[2 * q + 1] = (v >> 8) & 0x00FF00FFu;
    }
    // 16 registers x 64 lanes -> one register per group of four lanes: a lane pair exchanges halves of its register file four times
    // (literal bounds: with the halving written as a loop the compiler indexes R dynamically — a chain of 16 selects per access)
#define PG_XCHG(HALF, BIT)                                                  \
    {                                                                       \
        const bool up = (lane & BIT) != 0;                                  \
        _Pragma("unroll") for (int i = 0; i < HALF; ++i) {                  \
            const uint32_t send = up ? R[i] : R[i + HALF];                  \
            const uint32_t keep = up ? R[i + HALF] : R[i];                  \
            R[i] = keep + (uint32_t)__shfl_xor((int)send, BIT);             \
        }                                                                   \
    }
    PG_XCHG(8, 32)
    PG_XCHG(4, 16)
    PG_XCHG(2, 8)
    PG_XCHG(1, 4)
#undef PG_XCHG
    R[0] += (uint32_t)__shfl_xor((int)R[0], 2);
    R[0] += (uint32_t)__shfl_xor((int)R[0], 1);
    if ((lane & 3) == 0) {  // this lane holds register lane >> 2 = 2 q + odd: columns q + 8 odd (low half) and + 16 (high half)
        const uint32_t idx = (uint32_t)lane >> 2;
        out16[(idx >> 1) + ((idx & 1u) ? 8u : 0u)] = R[0];
    }
}
// One pass over the tile's rows for NWP (1 or 2) of their words, from byte `woff` of the row on: the lane's 16 rows in four
// groups of four (two groups' loads in flight), their popcounts added to `pcs` (one byte per row, four rows per register: a row
// of three or four words takes two passes — the registers of ONE pass of two words are what fits beside the 64 of eight waves per
// SIMD) and, in the row's LAST pass, counted into the histogram; the words' column sums through the carry-save tree and out.
template <int NWP, bool LASTPASS>
__device__ __forceinline__ void tile_statistics_pass(uint32_t *Hc, GlobalBytes rs, uint32_t npos, uint32_t nbytes, uint32_t woff,
                                                     uint32_t keep_last, uint32_t split, uint32_t N, uint32_t (&pcs)[4], uint32_t *cs_out, int lane) {
    const uint32_t N1 = N + 1u;
    uint32_t ones[NWP], twos[NWP], fours[NWP], eights[NWP], sixteens[NWP], hold4[NWP], hold8[NWP];
#pragma unroll
    for (int w = 0; w < NWP; ++w) ones[w] = twos[w] = fours[w] = eights[w] = sixteens[w] = hold4[w] = hold8[w] = 0;
    uint32_t nx[4][NWP];
    auto request = [&](int g, uint32_t (&dst)[4][NWP]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = (uint32_t)(4 * g + i) * 64u + (uint32_t)lane;
            fuse_load_row<NWP>(rs, min(r, npos - 1u) * nbytes + woff, dst[i]);  // (rows behind the tile's last: that one again, masked out below)
        }
    };
    request(0, nx);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        uint32_t rw[4][NWP];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int w = 0; w < NWP; ++w) rw[i][w] = nx[i][w];
        if (g < 3) request(g + 1, nx);
        uint32_t pc4 = pcs[g];  // the four rows' popcounts so far, a byte each
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = (uint32_t)(4 * g + i) * 64u + (uint32_t)lane;
            // (validity and the bin as arithmetic, not as lane masks: sixteen rows' masks alive at once are 32 scalar registers the
            // wide instantiations do not have)
            const uint32_t vmask = (uint32_t)((int32_t)(r - npos) >> 31);  // all ones for a row of the tile (r < npos <= 1024)
            if (LASTPASS) rw[i][NWP - 1] &= keep_last;  // (the row's last word holds bytes of the next row)
            uint32_t pc = 0;
#pragma unroll
            for (int w = 0; w < NWP; ++w) {
                rw[i][w] &= vmask;
                pc += (uint32_t)__popc(rw[i][w]);
            }
            if (LASTPASS) {
                pc = min(pc + ((pc4 >> (8 * i)) & 0xFFu), N);  // (junk bits beyond ngenomes: the reference indexes out of bounds there; our rows have none)
                const uint32_t idx = pc + (N1 & (uint32_t)((int32_t)(split - 1u - r) >> 31));  // + N + 1 for a row of the tile's second bin (r >= split)
                atomicAdd(&Hc[idx], vmask & 1u);
            } else {
                pc4 += pc << (8 * i);  // (at most 64 per pass)
            }
        }
        if (!LASTPASS) pcs[g] = pc4;
#pragma unroll
        for (int w = 0; w < NWP; ++w) {  // four rows into the planes: three carry-save adders, the carries of weight 4 and 8 held back in turn
            uint32_t u = ones[w] ^ rw[0][w];
            const uint32_t c2a = (ones[w] & rw[0][w]) | (u & rw[1][w]);
            ones[w] = u ^ rw[1][w];
            u = ones[w] ^ rw[2][w];
            const uint32_t c2b = (ones[w] & rw[2][w]) | (u & rw[3][w]);
            ones[w] = u ^ rw[3][w];
            u = twos[w] ^ c2a;
            const uint32_t c4 = (twos[w] & c2a) | (u & c2b);
            twos[w] = u ^ c2b;
            if ((g & 1) == 0) {
                hold4[w] = c4;
            } else {
                u = fours[w] ^ hold4[w];
                const uint32_t c8 = (fours[w] & hold4[w]) | (u & c4);
                fours[w] = u ^ c4;
                if (g == 1) {
                    hold8[w] = c8;
                } else {
                    u = eights[w] ^ hold8[w];
                    sixteens[w] = (eights[w] & hold8[w]) | (u & c8);
                    eights[w] = u ^ c8;
                }
            }
        }
    }
#pragma unroll
    for (int w = 0; w < NWP; ++w) {
        const uint32_t pl[5] = {ones[w], twos[w], fours[w], eights[w], sixteens[w]};
        fuse_flush_word(pl, cs_out + 16 * w, lane);
    }
}

template <int NW>
__device__ __forceinline__ void tile_statistics(uint32_t *H, const uint8_t *tile_rows, uint32_t npos, uint32_t nbytes, const AnchorDesc &a,
                                                uint32_t tile_start, uint32_t tile, const FuseArgs &fo, int lane) {
    const uint32_t N = fo.ngenomes, N1 = N + 1u, hw = fo.hw;
    const uint32_t nh = 2u * N1;  // histogram counters of a tile: (bin 0 / 1) x (popcount 0..N), four copies of them in LDS
#ifdef PG_PHASE_TIMING  // (slots 11..15 of the phase counters: wait for the stores, zero + 1-in-100 request, rows (first pass), rows (second pass) + 1-in-100 stores, histogram out)
    uint32_t tph[5] = {0, 0, 0, 0, 0}, tph_t = (uint32_t)__builtin_readcyclecounter();
#define PG_TPH(i) { const uint32_t n_ = (uint32_t)__builtin_readcyclecounter(); tph[i] += n_ - tph_t; tph_t = n_; }
#else
#define PG_TPH(i)
#endif
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every row store of this wave has been acknowledged by the L2
    __syncthreads();                     // (the probe's LDS buffers are dead from here on)
    PG_TPH(0)
    // (the base through readfirstlane: the tile's address is wave-uniform, but the compiler cannot see it)
    const uint64_t base = reinterpret_cast<uint64_t>(tile_rows);
    GlobalBytes rs = reinterpret_cast<GlobalBytes>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base));
    // bitmap.100: rows whose position in the contig is a multiple of 100 (cpp/anchor.cpp:169-177), eleven at most: requested now,
    // stored behind the rows' passes (a round trip to the L2 that nothing waits for)
    const uint32_t r100 = (100u - tile_start % 100u) % 100u + 100u * (uint32_t)lane;
    const bool want100 = fo.out100 != nullptr && r100 < npos;
    uint32_t w100[NW];
    fuse_load_row<NW>(rs, min(r100, npos - 1u) * nbytes, w100);
    for (uint32_t i = lane; i < 4u * nh; i += 64) H[i] = 0;
    // rows [0, split) of the tile lie in its first bin, the others in the next one (bins are at least a tile long)
    const uint64_t bin_end = ((uint64_t)(tile_start / a.binlen) + 1u) * a.binlen;
    const uint32_t split = (uint32_t)min((uint64_t)npos, bin_end - tile_start);
    const uint32_t keep = (nbytes & 3u) ? ((1u << (8u * (nbytes & 3u))) - 1u) : ~0u;  // bytes of the row in its last word
    uint32_t *const Hc = H + ((uint32_t)lane & 3u) * nh;
    uint32_t *cs_out = fo.tile_cs + (uint64_t)tile * fo.csw;
    uint32_t pcs[4] = {0, 0, 0, 0};
    __syncthreads();
    PG_TPH(1)
    if constexpr (NW <= 2) {
        tile_statistics_pass<NW, true>(Hc, rs, npos, nbytes, 0u, keep, split, N, pcs, cs_out, lane);
        PG_TPH(2)
    } else {
        tile_statistics_pass<2, false>(Hc, rs, npos, nbytes, 0u, ~0u, split, N, pcs, cs_out, lane);
        PG_TPH(2)
        tile_statistics_pass<NW - 2, true>(Hc, rs, npos, nbytes, 8u, keep, split, N, pcs, cs_out + 32, lane);
    }
    if (want100) {
        uint8_t *dst = fo.out100 + a.out100_off + (uint64_t)((tile_start + r100) / 100u) * nbytes;
#pragma unroll
        for (int i = 0; i < NW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if ((uint32_t)(4 * i + b) < nbytes) dst[4 * i + b] = (uint8_t)(w100[i] >> (8 * b));
    }
    __syncthreads();
    PG_TPH(3)
    uint32_t *th = fo.tile_hist + (uint64_t)tile * hw;
    for (uint32_t i = lane; i < hw; i += 64) {  // two counters per word (a tile has 1024 rows: a u16 holds any count)
        const uint32_t lo = H[2u * i] + H[nh + 2u * i] + H[2u * nh + 2u * i] + H[3u * nh + 2u * i];
        const uint32_t hi = H[2u * i + 1u] + H[nh + 2u * i + 1u] + H[2u * nh + 2u * i + 1u] + H[3u * nh + 2u * i + 1u];
        th[i] = lo | (hi << 16);
    }
    PG_TPH(4)
#ifdef PG_PHASE_TIMING
    if (lane == 0)
        for (int i = 0; i < 5; ++i) atomicAdd(&pg_phase_cycles[(blockIdx.x & 1023u) * 16u + 11 + i], (unsigned long long)tph[i]);
#endif
#undef PG_TPH
}

// M64: m-mers longer than 16 bases.  WIDE: split layout (SLOTS = 8 then counts the 16-byte chunks of a key line: the
// staging geometry is the same, a line holds 16 bare keys; m0 / m1 carry the hit's line and slot + 1)
// (probe_pipelined: the instantiations that run the skewed batch order, see the end of the kernel; they are held to the 64
// registers of 8 waves per SIMD — the only spill that costs them sits around the queue-full call, a cold path)
// (the skewed order runs for the one-word rows of 1..4 bytes and for two-word slots, every window; not for generic one-word rows
// nor for the split and inline layouts: profiles/r4_ab_early_fetch.txt, r4e_ab_wide_skewed_order.txt, r5i_inline_layout.txt.  The
// inline-layout probe is held to the 64 registers of 8 waves per SIMD all the same.)
template <bool TWO, int ROWMODE, int SLOTS, bool WIDE>
constexpr bool probe_pipelined = SLOTS == 8 && !WIDE && ROWMODE != 3 && (ROWMODE == 1 || ROWMODE >= 4 || TWO);
// The scalar registers count too: a SIMD's 800 SGPRs admit floor(800 / (ceil(sgpr / 16) * 16 + 16)) waves — 8 up to 80, 7 up to
// 96, 6 up to 112 (MI355X_MICROARCH.md) — whatever the compiler's own occupancy figure says.  Left alone the generic-row and
// split-layout instantiations took 92 and 105 (their lane masks live on the scalar unit): 7 and 6 waves.  Held to 80, a dozen
// masks move to vector lanes and the ninth to 63rd genome gain 3-6 % (27 x 40 Mb 140 -> 148 G k-mers/s).
// FUSE: the tile ends with its statistics (tile_statistics above; `fo` says where they go)
// BM: the byte-mask layout (SLOTS = 8 counts the 16-byte chunks of a line, as for WIDE; TWO false; ROWMODE 1 — pipelined, held to
// 8 waves like the 8-slot one-byte probe — or 3, whose column words in LDS admit 6 waves per SIMD whatever the registers)
template <int W_C, bool TWO, int ROWMODE, int SLOTS, bool M64, bool WIDE = false, bool INL = false, bool FUSE = false, bool BM = false>
__global__ __launch_bounds__(64, ((probe_pipelined<TWO, ROWMODE, SLOTS, WIDE> || INL || FUSE) ? 8 : 1))
__attribute__((amdgpu_num_sgpr(80))) void k_probe(const SubTable st, const uint64_t *__restrict__ seqw,
                                              const uint32_t *__restrict__ nmw, const uint32_t *__restrict__ has_n,
                                              const SeqDesc *__restrict__ sd, const AnchorDesc *__restrict__ ad,
                                              const uint32_t *__restrict__ tile_contig,
                                              const uint32_t *__restrict__ sched, uint32_t tile_base,
                                              uint8_t *__restrict__ out1, uint32_t nbytes, const RowCols rc, const FuseArgs fo) {
    // A staged line occupies 16*SLOTS + 16 bytes of LDS: the pad keeps the lanes' ds_read_b128 of
    // "their" lines off a common bank group (a power-of-two stride would be a 32-way conflict)
    constexpr int LDS_LINE_U4 = SLOTS + 1;
    // lines staged per step: 16, whatever the window — a batch ends in front of its 17th run (CUT below; 24 lines for the
    // 6-m-mer window lost to the smaller LDS footprint: profiles/r4b_ab_w6_maxrun.txt)
    constexpr int MAXRUN = PROBE_MAXRUN;
    constexpr int STAGE_ITERS = (MAXRUN * SLOTS + 63) / 64;  // 16-byte loads per lane per staging step
    // ONE block of LDS, carved up by hand, the tile's sequence words FIRST: the two-dword window reads of every batch
    // (ds_read2_b32, whose offsets reach 1020 bytes) then address them with an immediate instead of an add per window
    // (left to itself the compiler put the staging buffer first and the sequence words at 4.2-4.6 KB).
    constexpr int BUF_U4 = ((STAGE_ITERS * 64 + SLOTS - 1) / SLOTS) * LDS_LINE_U4;  // room for every staged chunk slot
    constexpr int OFF_RW = PROBE_SEQW * 8, OFF_NW = OFF_RW + (PROBE_SEQW + 1) * 8, OFF_LW = OFF_NW + PROBE_SEQW * 4;
    constexpr int QCAP = PROBE_QCAP;
    constexpr int OFF_BUF = (OFF_LW + MAXRUN * 4 + 15) & ~15, OFF_QG = OFF_BUF + BUF_U4 * 16;
    constexpr int OFF_QP = OFF_QG + QCAP * 4, LDS_BYTES = OFF_QP + QCAP * 2;
    static_assert(OFF_LW <= 1020 || PROBE_TILE > 1024, "the sequence words must stay within reach of ds_read2_b32's offsets");
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    uint64_t *const sw = reinterpret_cast<uint64_t *>(lds);
    uint64_t *const rw = reinterpret_cast<uint64_t *>(lds + OFF_RW);
    uint32_t *const nw = reinterpret_cast<uint32_t *>(lds + OFF_NW);
    uint32_t(*const lines_w)[MAXRUN] = reinterpret_cast<uint32_t(*)[MAXRUN]>(lds + OFF_LW);
    uint4(*const buf)[BUF_U4] = reinterpret_cast<uint4(*)[BUF_U4]>(lds + OFF_BUF);
    uint32_t *const q_grp = reinterpret_cast<uint32_t *>(lds + OFF_QG);  // overflow queue of the tile (position order): the entry's group
    uint16_t *const q_pl = reinterpret_cast<uint16_t *>(lds + OFF_QP);   // and position within the tile (the key is re-derived from sw)
    PG_PH_DECL
    const int lane = threadIdx.x;
    const int k = (int)st.k;
    // (a minimizer table has 20 <= k <= 32, minimizer_length: the low word of the k-mer mask is all ones there, and the
    // compiler drops its ANDs once it knows)
    if constexpr (W_C != 0) __builtin_assume(k >= 20 && k <= 32);
    // tiles run in launch order unless the result carries a schedule (co-scheduled anchor genomes:
    // homologous regions of all genomes next to each other, so that table lines are shared in L2)
    // (tile_base: the launch covers a contig range of the result; a schedule is a permutation within such ranges)
    const uint32_t tile = sched ? sched[blockIdx.x + tile_base] : blockIdx.x + tile_base;
    const uint32_t c = tile_contig[tile];
    const AnchorDesc a = ad[c];
    const SeqDesc s = sd[c];
    const uint32_t tile_start = (tile - a.tile0) * PROBE_TILE;
    const uint32_t npos = min((uint32_t)PROBE_TILE, a.nkmers - tile_start);
    const bool hasn = has_n[c] != 0;

    // packed bases of the tile (+ halo), the only sequence traffic: 0.25 B per position
    for (int i = lane; i < PROBE_SEQW; i += 64) {
        const uint64_t wi = (uint64_t)(tile_start >> 5) + i;
        const uint64_t wv = wi < s.nwords ? seqw[s.seq_off + wi] : 0ull;
        sw[i] = wv;
        rw[PROBE_SEQW - 1 - i] = pair_reverse64(~wv);
        nw[i] = (hasn && wi < s.nwords) ? nmw[s.seq_off + wi] : 0u;
    }
    if (lane == 0) rw[PROBE_SEQW] = 0;  // (a window's three dwords may reach one word past the end)
    __syncthreads();  // single wave: compiles to a wave-level wait, not an s_barrier

    // (minimizer tables: k >= 20, the mask's low word is all ones — spelt out, the compiler drops the ANDs with it: two per
    // position)
    const uint64_t kmask = W_C ? (((uint64_t)(k == 32 ? ~0u : ((1u << (2 * k - 32)) - 1u)) << 32) | 0xFFFFFFFFull) : kmer_mask(k);
    const uint32_t rcb = PROBE_SEQ_BASES - (uint32_t)k;
    constexpr int HALO = W_C ? W_C - 1 : 0;  // m-mers of a window that lanes below its own supply
    constexpr bool CARRY = W_C >= 2;  // the first lanes' missing m-mers carried over from the batch before (sliding_min_suffix)
    // CUT: a batch ends in front of its (MAXRUN + 1)-th run — the next batch starts there — so that ONE staging step takes
    // every batch: at w = 7 a quarter of the 58-position batches met more than 16 lines and paid a second, unhidden fetch
    // (not in direct mode, k < 20: every position is a run of its own there, and a batch of 16 positions would run the front
    // end four times where four staging steps share one)
    constexpr bool CUT = W_C != 0;
    const uint32_t m = W_C ? (uint32_t)k - W_C + 1 : 0;
    const uint64_t mm64 = (m >= 32) ? ~0ull : ((1ull << (2 * (m ? m : 1))) - 1);
    // (columns mode: `out1` is the block's column buffer, `nbytes` its width in genomes; the "rows" of the tile are
    // the LDS words the columns are assembled in)
    __shared__ unsigned long long cols[ROWMODE == 3 ? TILE_SLOTS * COLS_G : 1];
    if constexpr (ROWMODE == 3) {
        for (uint32_t i = lane; i < TILE_SLOTS * COLS_G; i += 64) cols[i] = 0;
        __syncthreads();
    }
#if PG_ABLATE == 9 || PG_ABLATE == 10  // (timing experiment, wrong rows: every tile writes into a window of 256 tiles' rows — the L2 takes the stores, HBM sees none)
    uint8_t *tile_rows = out1 + (uint64_t)(blockIdx.x & 255u) * PROBE_TILE * nbytes;
#else
    uint8_t *tile_rows = ROWMODE == 3 ? reinterpret_cast<uint8_t *>(cols) : out1 + a.out_off + (uint64_t)tile_start * nbytes;
#endif
    uint32_t qn = 0;  // wave-uniform: overflow entries of this tile so far

    const uint8_t *chunk_base = st.buckets + (uint32_t)(lane % SLOTS) * 16u;  // this lane's 16-byte chunk of line 0
    const uint32_t lbytes = BM ? st.W * 128u : INL ? st.layout * 64u : st.slots * (WIDE ? 8u : 16u);  // bytes per line (= 16 * SLOTS = 128), as a run-time scalar (inline layout: LAYOUT_INLINE * 64; byte-mask: W = 1)

    // A batch in three parts, so that the front end of batch i + 1 can run while the table lines of batch i are on
    // their way: the fetch is the longest wait of a batch — a couple of thousand cycles behind a busy
    // texture-address unit and a TLB that misses on a quarter of these random lines — and the next batch's keys,
    // minimizers and runs need nothing from it.
    struct Front {  // what the front end of a batch leaves behind: no table access so far
        uint64_t key;
        uint32_t grp, line, rid, nruns, padline;
        uint32_t adv;                            // positions the batch covers: the next one starts that many further on (wave-uniform)
        uint32_t ln[STAGE_ITERS];                // the lines this lane fetches a chunk of in the first staging step
        unsigned long long rmask, amask, lmask;  // lanes with a position / active (no N in the window) / first of a run
    };
    // ---- the carry of a batch that starts at position b0 of the tile (the tile's first, or one the tail loop starts
    // again): lane j < HALO gets the rank of m-mer b0 + j (the m-mers before m-mer b0 + HALO, lane 0's own); the other
    // lanes' values are not used.  An m-mer straight from the staged sequence words: forward strand from sw, reverse
    // complement from rw — the values front() cuts out of X and B.
    auto carry_at = [&](const uint32_t b0) __attribute__((always_inline)) {
        uint32_t y = ~0u;
        if constexpr (CARRY) {
            const uint32_t q = b0 + (uint32_t)min(lane, HALO - 1);  // m-mer number = its first base in the tile
            const uint64_t fa = extract_bases32(reinterpret_cast<const uint32_t *>(sw), q) & mm64;
            const uint64_t fr = extract_bases32(reinterpret_cast<const uint32_t *>(rw), PROBE_SEQ_BASES - q - m) & mm64;
            const uint32_t h = M64 ? mmer_rank(fa < fr ? fa : fr) : mz_order(min((uint32_t)fa, (uint32_t)fr));
            y = h;
        }
        return y;
    };
    uint32_t carry = ~0u;  // (CARRY) what the next front() takes in (lanes 0 .. HALO - 1): written by carry_at or by the front() before
    // ---- keys: lane = position b0 + lane; it also owns m-mer number b0 + lane + HALO ----
    auto front = [&](const uint32_t b0) __attribute__((always_inline)) {
        Front f;
        const int32_t pl = (int32_t)(b0 + lane);
        // (a ballot straight off the compare stays a scalar mask)
        f.rmask = __builtin_amdgcn_ballot_w64(pl < (int32_t)npos);
        const uint32_t pq = (uint32_t)pl;
        const uint64_t X = extract_bases32(reinterpret_cast<const uint32_t *>(sw), pq) & kmask;
        const uint64_t B = revcomp_window(rw, pq, kmask, rcb);
        f.key = ~(X > B ? X : B) & kmask;  // (canonical_from_xb with this kernel's mask)
        f.amask = f.rmask;
        if (hasn) f.amask &= __builtin_amdgcn_ballot_w64(extract_nmask(nw, pq, k) == 0);
        [[maybe_unused]] uint32_t own = 0;
        if (W_C) {
            // m-mer number b0 + lane + HALO is the LAST m-mer of this lane's own k-mer: forward strand from X, reverse
            // complement from B — no second pass over the sequence words
            constexpr uint32_t off = (uint32_t)HALO;  // m-mer's offset inside the k-mer
            if constexpr (!M64) {  // m-mers of up to 32 bits: one funnel shift each, no 64-bit arithmetic
                const uint32_t mm32 = (uint32_t)mm64;
                const uint32_t fa = __builtin_amdgcn_alignbit((uint32_t)(X >> 32), (uint32_t)X, 2 * off) & mm32;
                const uint32_t fr = __builtin_amdgcn_alignbit((uint32_t)(B >> 32), (uint32_t)B, 2 * (HALO - off)) & mm32;
                f.grp = mz_order(min(fa, fr));  // (= mmer_rank: its fold of the high half is the identity here)
            } else {
                const uint64_t fa = (X >> (2 * off)) & mm64;
                const uint64_t fr = (B >> (2 * (HALO - off))) & mm64;
                f.grp = mmer_rank(fa < fr ? fa : fr);
            }
#ifdef PG_DUMMY_VALU
            {   // (experiment: PG_DUMMY_VALU extra VALU instructions per batch, nothing else changed)
                uint32_t dm = f.grp;
#pragma unroll
                for (int i = 0; i < PG_DUMMY_VALU; ++i) asm volatile("v_alignbit_b32 %0, %0, %1, 3" : "+v"(dm) : "v"((uint32_t)lane));
                if (dm == 0x12345u && lane == 77) out1[0] = 1;
            }
#endif
            // sliding minimum over lanes [lane-W_C+1, lane]: m <- min(own rank, m of the lane below), W_C-1 times
            // (the first lanes of the wave see shorter windows: the carry supplies the m-mers before them)
            if constexpr (CARRY) {
                own = f.grp;  // (this lane's own m-mer rank: the next batch's carry is cut out of these below)
                uint32_t suffix = __builtin_amdgcn_inverse_ballot_w64((1ull << HALO) - 1ull) ? carry : ~0u;
                f.grp = sliding_min_suffix<W_C >= 2 ? W_C : 2>(f.grp, suffix);
                f.grp = min(f.grp, suffix);
            } else {
                f.grp = sliding_min<W_C ? W_C : 1>(f.grp);
            }
        } else {
            f.grp = group_of_key(f.key);
        }
        // ---- runs of equal home line among the active lanes (lane masks on the scalar unit: a run starts at an active
        // lane whose predecessor is inactive or on another line; lane 0 has no predecessor — the shift leaves its bit clear)
        f.line = home_of_group(f.grp, st.nbuckets);
        f.lmask = f.amask & (~(f.amask << 1) | differs_from_lane_below(f.line));
        f.rid = run_ids(f.lmask);  // run id of an active lane
        uint32_t lanes_kept = 64u;
        if constexpr (CUT) {
            // the lanes of the first MAXRUN runs — a prefix of the wave: run ids do not fall from lane to lane; the lanes
            // in front of the first run count -1 — stay; the others' positions are the next batch's
            const unsigned long long keep = __builtin_amdgcn_sicmp((int32_t)f.rid, MAXRUN, 40 /* signed < */);
            f.amask &= keep;
            f.rmask &= keep;
            f.lmask &= keep;
            lanes_kept = (uint32_t)__popcll(keep);  // (>= MAXRUN when anything is cut: the batch always advances)
        }
        f.adv = lanes_kept;
        if constexpr (CARRY) {
            // the next batch's carry: the HALO m-mer ranks in front of its first position's own = lanes lanes_kept - HALO
            // .. lanes_kept - 1 of this batch (not needed before the next front(): the LDS crossbar's latency is hidden)
            // (lanes 0 .. HALO - 1, the only ones whose result is used, read lanes below 64: no wrap to take care of)
            carry = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((uint32_t)lane << 2) + ((lanes_kept - HALO) << 2)), (int)own);
        }
        f.nruns = (uint32_t)__popcll(f.lmask);
        // (a batch without runs: s_ff1 of an empty mask is -1, v_readlane takes it modulo 64 — lane 63's line, a line of the table
        // like any other, fetched and scanned by no lane: no test for the empty mask)
        // (the instruction itself, not __builtin_ctzll: ctz of 0 is undefined to the COMPILER — it may fold anything — while
        // s_ff1_i32_b64 is defined by the ISA to return -1; __ffsll - 1 is defined too and costs two scalar instructions more)
        int first_run;
        asm("s_ff1_i32_b64 %0, %1" : "=s"(first_run) : "s"(f.lmask));
        f.padline = (uint32_t)__builtin_amdgcn_readlane((int)f.line, first_run & 63);  // (wave-uniform)
#if PG_ABLATE == 3  // (timing experiment: keys, minimizers and runs only — no table access)
        if (f.line != 0xDEADBEEFu) f.nruns = 0;
#endif
        // The first staging step's line numbers go through lines_w HERE — one per run, padded with the first run's
        // (see issue) — and every lane reads back the ones it will fetch a chunk of: two LDS round trips that would
        // stand between "the chunks of the batch before are staged" and this batch's fetch; the read is in flight
        // while the caller does something else (the skewed order: the whole staging of the batch before).
        const bool leader = __builtin_amdgcn_inverse_ballot_w64(f.lmask);
        if (lane < MAXRUN) lines_w[0][lane] = f.padline;
        if (leader && f.rid < (uint32_t)MAXRUN) lines_w[0][f.rid] = f.line;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < STAGE_ITERS; ++it) f.ln[it] = lines_w[0][it * (64 / SLOTS) + lane / SLOTS];
        return f;
    };
    // ---- the fetch of a staging step: runs r0 .. r0 + MAXRUN - 1 of the batch, MAXRUN lines = MAXRUN * SLOTS chunks of 16
    // bytes, coalesced, all loads of the step in flight.  The step's line numbers go through lines_w, one per run; the
    // entries behind the last run repeat the first run's line (the same address again inside one load: no second
    // fetch), so that a lane reads its entries at fixed places — no clamp of the entry's number, one LDS instruction for
    // all of a lane's entries.  Loads are unconditional: any predicate makes the compiler sink each load into its own
    // branch and wait for it there.  A lane always fetches chunk lane % SLOTS of a line: its address = the lane's own
    // base + line x line bytes, one multiply-add (the line bytes come from the table's descriptor, a scalar the
    // compiler cannot turn into a 64-bit shift and a 64-bit add).
    struct Lines {  // the step's 16-byte chunks on their way into this lane's registers
        uint4 v[STAGE_ITERS];
    };
    auto issue = [&](const Front &f, const uint32_t r0) __attribute__((always_inline)) {
        Lines L;
        uint32_t ln[STAGE_ITERS];
        if (r0 != 0u) {  // (the first step's line numbers are the front end's: f.ln)
            const uint32_t nl = min((uint32_t)MAXRUN, f.nruns - r0);  // (0 for a batch without runs: r0 is 0 then)
            const bool leader = __builtin_amdgcn_inverse_ballot_w64(f.lmask);
            if (lane < MAXRUN) lines_w[0][lane] = f.padline;
            if (leader && f.rid - r0 < nl) lines_w[0][f.rid - r0] = f.line;
            __syncthreads();
        }
#pragma unroll
        for (int it = 0; it < STAGE_ITERS; ++it) {
            if (r0 != 0u) ln[it] = lines_w[0][it * (64 / SLOTS) + lane / SLOTS];
            else ln[it] = f.ln[it];
#if PG_ABLATE == 1  // (timing experiment, wrong rows: every fetch a cache hit — the lines of one 64 KB window)
            ln[it] &= 511u;
#endif
        }
#pragma unroll
        for (int it = 0; it < STAGE_ITERS; ++it) L.v[it] = *reinterpret_cast<const uint4 *>(chunk_base + (uint64_t)ln[it] * lbytes);
        return L;
    };
    // ---- the rest of the batch: its lines into LDS, every lane scans its own; overflow entries; the rows ----
    auto back = [&](const Front &f, const Lines &L, const uint32_t b0, auto &&after_staging) __attribute__((always_inline)) {
        const bool act = __builtin_amdgcn_inverse_ballot_w64(f.amask), inrange = __builtin_amdgcn_inverse_ballot_w64(f.rmask);
        const int32_t pl = (int32_t)(b0 + lane);
        uint32_t m0 = 0, m1 = 0;
        [[maybe_unused]] uint32_t rw4[4] = {0, 0, 0, 0};  // (inline layout: the row's words, zeros for an absent key)
        int rcode = 0;
        // a staging step's chunks into LDS (wave-uniform placement: chunk idx of the step -> line idx / SLOTS, slot
        // idx % SLOTS), then every lane of the step's runs scans its own line
        auto stage = [&](const Lines &S) __attribute__((always_inline)) {
            // (chunk it * 64 + lane of the step: line it * (64 / SLOTS) + lane / SLOTS, slot lane % SLOTS — one address per
            // lane, the iterations at constant offsets from it)
            uint4 *const mine = buf[0] + ((uint32_t)lane / SLOTS) * LDS_LINE_U4;
#pragma unroll
            for (int it = 0; it < STAGE_ITERS; ++it) {
                if constexpr (WIDE || BM) mine[it * (64 / SLOTS) * LDS_LINE_U4 + ((uint32_t)lane % SLOTS)] = S.v[it];  // (bare keys: as they are)
                else stage_chunk(mine + it * (64 / SLOTS) * LDS_LINE_U4, (uint32_t)lane % SLOTS, SLOTS, S.v[it]);
            }
            __syncthreads();
        };
        auto scan = [&](const uint32_t r0) __attribute__((always_inline)) {
            const uint32_t nl = min((uint32_t)MAXRUN, f.nruns - r0);
#if PG_ABLATE == 5  // (timing experiment: lines fetched and staged, no slot scan: every lane "hits" with one LDS word)
            if (act && f.rid - r0 < nl) {
                rcode = 1;
                m0 = m1 = reinterpret_cast<const uint32_t *>(buf[0] + (f.rid - r0) * LDS_LINE_U4)[2];
            }
#else
            if (act && f.rid - r0 < nl) {
                if constexpr (WIDE && INL) {
                    rcode = scan_keys_inl(buf[0] + (f.rid - r0) * LDS_LINE_U4, f.key, st.slots, m1);
                    if (m1) masks_inl(buf[0] + (f.rid - r0) * LDS_LINE_U4, st.slots, st.W, m1 - 1u, rw4);
                } else if constexpr (WIDE) {
                    rcode = scan_keys16_lds(buf[0] + (f.rid - r0) * LDS_LINE_U4, f.key, m1);
                    m0 = f.line;
                } else if constexpr (BM) {
                    rcode = scan_line_bm(buf[0] + (f.rid - r0) * LDS_LINE_U4, f.key, m0);
                } else {
                    rcode = scan_line_lds<TWO, SLOTS>(buf[0] + (f.rid - r0) * LDS_LINE_U4, f.key, m0, m1);
                }
            }
#endif
            __syncthreads();
        };
        // The batch's lines are waited for HERE, on every path (a batch without runs has none in flight).  Left to the
        // compiler, the wait sits inside the branch below, the chunks count as possibly still on their way where the
        // paths meet, and the first instruction that re-uses one of their registers — an address of the NEXT fetch,
        // issued right behind this batch's row store — gets a vmcnt(0) that waits for that store to be acknowledged.
        PG_PH(1)
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), nothing else
        PG_PH(2)
        // (a batch without runs — a stretch of N — is not singled out: its lines_w hold line 0 throughout (padline), which is fetched,
        // staged and scanned by no lane; three wave-uniform tests and their branches per batch were 10 scalar instructions:
        // profiles/r4e_ab_probe_scalar_cuts.txt)
        stage(L);
        PG_PH(3)
        after_staging();  // (the chunks' registers are free from here on: the skewed order starts the NEXT batch's fetch now)
        PG_PH(4)
        scan(0u);
        PG_PH(5)
        if constexpr (!CUT)
        for (uint32_t r0 = MAXRUN; r0 < f.nruns; r0 += MAXRUN) {  // (a batch with more than MAXRUN lines: a quarter of the batches at w = 7)
            const Lines X = issue(f, r0);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            stage(X);
            scan(r0);
        }
        // ---- overflow: absent from a full line -> queue entry for the next line of its sequence ----
        // (sicmp = the compare as a lane mask, predicate 40 = signed less-than: a ballot of `rcode < 0` is sunk into the
        // blocks rcode comes from and its bool rebuilt here through 0 / 1)
        const unsigned long long omask = f.amask & __builtin_amdgcn_sicmp(rcode, 0, 40);
        const bool ovf = __builtin_amdgcn_inverse_ballot_w64(omask);
        if (omask) {
            // (the entry carries the GROUP and the position, nothing else: the line and step of every later level — the
            // multiplies and the wrap — are worked out by the drain's dense batches (drain_queue), not here for the few
            // overflowing lanes of every batch; a GROUP_CHAIN == 1 tuning build, whose level 1 is the key's own sequence,
            // is served by the same entry: line_of_level takes the key, which the drain cuts out of the sequence words)
            // (the queue always has room for a whole batch: the batch loop leaves for an early drain before it could not)
            const uint32_t slot = set_lane_index(omask, qn);
            if (ovf) {
                q_grp[slot] = f.grp;
                q_pl[slot] = (uint16_t)pl;
            }
            qn += (uint32_t)__popcll(omask);
        }
        PG_PH(10)
        // (32-bit offset from the tile's uniform base: one store with a scalar base address)
        if constexpr (WIDE && INL) {
            // (ragged rows: one store per row — not in the tile's last batch, see store_row_fused; positions without a row hold zeros)
            const bool fuse = (nbytes & 3u) != 0u && b0 + (uint32_t)__popcll(f.rmask) < npos;  // (wave-uniform)
            if (fuse) {
                const uint32_t mine = inrange ? rw4[0] : 0u;
                const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);  // (lane 63: 0)
                if (inrange) store_row_fused(tile_rows + (uint64_t)(uint32_t)pl * nbytes, nbytes, rw4, nxt);
            } else if (inrange) {
                store_row_regs(tile_rows + (uint64_t)(uint32_t)pl * nbytes, nbytes, rw4);
            }
        } else if constexpr (WIDE) {
#if PG_ABLATE == 2  // (timing experiment: no mask gather, no row store)
            if (inrange && m0 == 0xDEADBEEFu && m1 == 77u)
#elif PG_ABLATE == 8 || PG_ABLATE == 10  // (timing experiment, wrong rows: the row store without a DIVERGENT mask gather — every hit copies slot 0 of line 0's block)
            if (m1) m0 = 0, m1 = 1;
            if (inrange)
#else
            // (rows of 13..15 bytes, W = 4: the hit's four mask words into registers and ONE 16-byte store per row, as the inline
            // layout's ragged rows — store_row_fused; not in the tile's last batch)
            if (st.W == 4u && (nbytes & 3u) != 0u && b0 + (uint32_t)__popcll(f.rmask) < npos) {  // (wave-uniform)
                uint32_t v4[4] = {0, 0, 0, 0};
                if (inrange && m1) {
                    const WordsN<4> g = *reinterpret_cast<const WordsN<4> *>(reinterpret_cast<const uint32_t *>(st.masks) + ((uint64_t)m0 * SPLIT_KEYS + (m1 - 1u)) * 4u);
                    v4[0] = g.w[0], v4[1] = g.w[1], v4[2] = g.w[2], v4[3] = g.w[3];
                }
                const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v4[0], 0x130 /* wave_shl:1 */, 0xf, 0xf, true);  // (lanes without a row hold 0)
                if (inrange) store_row_fused(tile_rows + (uint64_t)(uint32_t)pl * nbytes, nbytes, v4, nxt);
            } else if (inrange)
#endif
                store_row_wide(st.masks, st.W, nbytes, tile_rows + (uint64_t)(uint32_t)pl * nbytes, m0, m1);
        } else if constexpr (ROWMODE == 3) {
            const uint32_t w0 = b0 >> 6, sh = b0 & 63u;
            for (uint32_t j = 0; j < rc.col0; ++j) {  // (uniform) one ballot per genome of the block
                const unsigned long long shifted = __ballot(inrange && ((m0 >> j) & 1u));  // bit i = position b0 + i
                if (lane == 0 && shifted) {
                    cols[w0 * COLS_G + j] |= shifted << sh;
                    if (sh && (shifted >> (64u - sh))) cols[(w0 + 1) * COLS_G + j] |= shifted >> (64u - sh);
                }
            }
        } else {
            if (ROWMODE == 6 && b0 + (uint32_t)__popcll(f.rmask) < npos) {  // (wave-uniform; ROWMODE a constant)
                // (three-byte rows as ONE unaligned dword per row — the row and the next lane's first byte — as the
                // 5..7-byte rows; not in the tile's last batch)
                const uint32_t mine = inrange ? m0 : 0u;
                const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
                struct __attribute__((packed)) U32 { uint32_t v; };
                if (inrange) reinterpret_cast<U32 *>(tile_rows + (uint32_t)pl * 3u)->v = (m0 & 0xFFFFFFu) | (nxt << 24);
            } else if constexpr (ROWMODE == 6) {
                // (the tile's last batch) Three-byte rows as ALIGNED dwords: a u16 and a u8 per lane at odd addresses cost the launch a third
                // of its time (20 x 40 Mb: 6.7 ps per position against 5.1 with the four-byte rows of 27 genomes).
                // The batch's rows are 3 x 58 consecutive bytes; the aligned dword that starts inside a lane's row
                // holds the row's last 3 - j bytes and the next lane's first j + 1 (j = 0..2 by the row's address
                // mod 4; a row that starts at byte 1 of a dword starts none) — the next lane's mask comes over one DPP
                // shift, and ~43 lanes write whole dwords.  The lane without a successor in the batch (lane 63, or the
                // tile's last position) and the batch's first position, whose leading bytes no lane of this batch
                // covers, write their own three bytes as before; stores that overlap write equal bytes.
                const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m0, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
                const uint32_t o4 = (uint32_t)reinterpret_cast<uintptr_t>(tile_rows) & 3u;  // (a tile starts at a multiple of 512 rows)
                const uint32_t j = ((uint32_t)pl - o4) & 3u;
                const uint32_t lo = (nxt << 24) | (m0 & 0xFFFFFFu);
                const uint32_t dw = __builtin_amdgcn_alignbit(nxt >> 8, lo, 8u * j);
                const unsigned long long nextin = f.rmask >> 1;
                const unsigned long long dmask = f.rmask & nextin & __builtin_amdgcn_ballot_w64(j != 3u);
                const unsigned long long fmask = f.rmask & (1ull | ~nextin);
                uint8_t *row = tile_rows + (uint32_t)pl * 3u;
                if (__builtin_amdgcn_inverse_ballot_w64(dmask)) *reinterpret_cast<uint32_t *>(row + j) = dw;
                if (__builtin_amdgcn_inverse_ballot_w64(fmask)) store_row<ROWMODE>(row, m0, m1, rc);
            } else
#if PG_ABLATE == 2  // (timing experiment: no row store unless a value no mask has turns up)
            if (inrange && m0 == 0xDEADBEEFu)
#else
            // (rows of 5..7 bytes, 33..56 genomes: ONE 8-byte store per row — the row and the first bytes of the next lane's, as
            // store_row_fused does for the wider ragged rows; not in the tile's last batch)
            if (ROWMODE == 0 && TWO && rc.words == 3u && nbytes >= 5u && b0 + (uint32_t)__popcll(f.rmask) < npos) {  // (wave-uniform)
                const uint32_t mine = inrange ? m0 : 0u;
                const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
                if (inrange) {
                    typedef uint32_t u32x2u __attribute__((ext_vector_type(2), aligned(1)));
                    const uint32_t t8 = 8u * (nbytes - 4u);  // bits of the row in its second word (8, 16 or 24)
                    u32x2u q = {m0, (m1 & ((1u << t8) - 1u)) | (nxt << t8)};
                    *reinterpret_cast<u32x2u *>(tile_rows + (uint32_t)pl * nbytes) = q;  // (non-temporal: 56 genomes +3 %, 40 genomes mixed — plain)
                }
            } else if (inrange)
#endif
                store_row<ROWMODE>(tile_rows + (ROWMODE == 1 ? (uint32_t)pl : ROWMODE == 4 ? (uint32_t)pl * 4u : ROWMODE == 5 ? (uint32_t)pl * 2u : ROWMODE == 6 ? (uint32_t)pl * 3u : (uint32_t)pl * nbytes), m0, m1, rc);
        }
        PG_PH(6)
    };
    // The skewed order — front end of batch i + 1 between the fetch of batch i and its use — keeps the fetched chunks
    // and two batches' keys in registers at once: it pays where that still fits 64 registers (8 waves per SIMD: this
    // kernel's speed goes with its occupancy — 7 waves cost 7 %, 5 waves 28 %), i.e. for the one-byte rows of up to 8
    // genomes (configs[1]: 4.31 -> 4.17 ms); the wider instantiations spill there and keep the plain order.
    constexpr bool PIPE = probe_pipelined<TWO, ROWMODE, SLOTS, WIDE>;
    constexpr int LEVELS = (W_C >= 6 && !TWO && !WIDE && PROBE_STAGED_LEVELS > 1) ? 1 : PROBE_STAGED_LEVELS;  // (W_C >= 6: the wide-window tables of up to 16 genomes)
    // The batch loop runs until the tile is through OR the overflow queue could not take another full batch (tiles inside
    // a repeat family: most of their keys sit outside their home lines): the queue is drained then and the loop goes on
    // where it stopped.  So no batch ever meets a full queue — the lane-by-lane chase that served it was a function
    // call inside the loop, whose clobbered registers the allocator answered with spills on the hot path.
    static_assert(QCAP >= 128, "an early drain must leave room for a batch");
    constexpr uint32_t QROOM = QCAP - 64;  // entries the queue may hold when a batch starts
    // (The hot loop stands on its own: what it keeps in registers is dead when it ends.  The tail — a plain batch loop
    // around the one drain — only ever runs batches for the tiles whose queue filled up.)
    uint32_t b0 = 0;
    if constexpr (PIPE) {
        // The skewed order — front end of batch i + 1 between the fetch of batch i and its use — keeps the fetched chunks
        // and two batches' keys in registers at once: it pays where that still fits 64 registers (8 waves per SIMD: this
        // kernel's speed goes with its occupancy — 7 waves cost 7 %, 5 waves 28 %)
        Lines L;
#pragma unroll
        for (int it = 0; it < STAGE_ITERS; ++it) L.v[it] = make_uint4(0, 0, 0, 0);
        PG_PH(0)
        carry = carry_at(0u);
        Front cur = front(0u);
        L = issue(cur, 0u);
        for (;;) {
            PG_PH(7)
            const uint32_t b1 = b0 + cur.adv;
            const bool more = b1 < npos;  // (wave-uniform)
            Front nxt = cur;
            __builtin_amdgcn_sched_barrier(0);  // (the parts stay apart: interleaved by the scheduler they keep both batches' temporaries alive)
            if (more) nxt = front(b1);  // while the lines of `cur` are on their way
            __builtin_amdgcn_sched_barrier(0);
            // the next batch's fetch goes out as soon as this batch's chunks have left their registers for LDS: it is in
            // flight during this batch's slot scan, row store and overflow entries AND the front end after next
            back(cur, L, b0, [&]() __attribute__((always_inline)) {
                if (more) L = issue(nxt, 0u);
            });
            __builtin_amdgcn_sched_barrier(0);
            b0 = b1;
            if (!more || qn > QROOM) break;  // (rare way out with a fetch in flight: nobody reads it; the tail starts the batch again)
            cur = nxt;
        }
    } else {
        {
            carry = carry_at(0u);
            const Front f = front(0u);
            const Lines L = issue(f, 0u);  // (also for a batch without runs — a stretch of N: line 0 is fetched and ignored)
            back(f, L, 0u, [] {});
            b0 = f.adv;
        }
        while (b0 < npos && qn <= QROOM) {
            const Front f = front(b0);
            const Lines L = issue(f, 0u);
            back(f, L, b0, [] {});
            b0 += f.adv;
        }
    }
    PG_PH(7)
    for (;;) {
        drain_queue<TWO, ROWMODE, SLOTS, MAXRUN, WIDE, LEVELS, INL, BM>(st, qn, sw, rw, q_grp, q_pl, lines_w[0], buf[0], tile_rows, nbytes, rc, lane);
        qn = 0;
        if (b0 >= npos) break;
        __syncthreads();
        carry = carry_at(b0);  // (the hot loop may have left with the front end of a batch it did not finish)
        while (b0 < npos && qn <= QROOM) {
            const Front f = front(b0);
            const Lines L = issue(f, 0u);
            back(f, L, b0, [] {});
            b0 += f.adv;
        }
    }
    PG_PH(8)
    PG_PH_FLUSH
    if constexpr (FUSE) {
        static_assert(ROWMODE != 1 && ROWMODE != 3 && LDS_BYTES >= 4 * 4 * 2 * 129, "fused statistics: rows of 2..16 bytes; four copies of 2 x 129 histogram counters in LDS");
        // Everything about the tile is looked up AGAIN (through pointers the compiler cannot identify with the ones the kernel
        // began with): kept alive across the batch loop these values would cost it scalar registers it does not have.
        const AnchorDesc *ad2 = ad;
        const uint32_t *tc2 = tile_contig, *sched2 = sched;
        asm volatile("" : "+s"(ad2), "+s"(tc2), "+s"(sched2));
        const uint32_t tile2 = sched2 ? sched2[blockIdx.x + tile_base] : blockIdx.x + tile_base;
        const AnchorDesc a2 = ad2[tc2[tile2]];
        if (a2.binlen >= (uint32_t)PROBE_TILE) {  // (wave-uniform) contigs with shorter bins are the statistics pass's (launched over their tiles only)
            const uint32_t ts2 = (tile2 - a2.tile0) * PROBE_TILE;
            const uint32_t np2 = min((uint32_t)PROBE_TILE, a2.nkmers - ts2);
            const uint8_t *rows2 = out1 + a2.out_off + (uint64_t)ts2 * nbytes;
            uint32_t *H = reinterpret_cast<uint32_t *>(lds);
            if constexpr (WIDE) {
                if (nbytes <= 12u) tile_statistics<3>(H, rows2, np2, nbytes, a2, ts2, tile2, fo, lane);
                else tile_statistics<4>(H, rows2, np2, nbytes, a2, ts2, tile2, fo, lane);
            } else {
                tile_statistics<TWO ? 2 : 1>(H, rows2, np2, nbytes, a2, ts2, tile2, fo, lane);
            }
        }
    }
    if constexpr (ROWMODE == 3) {
        // the tile's columns: TILE_SLOTS slots x `width` (= nbytes) genomes, slot-major — what k_cols_extract would have written
        __syncthreads();
        const uint32_t width = nbytes, trel = tile - tile_base;
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(out1) + (uint64_t)trel * TILE_SLOTS * width;
        for (uint32_t i = lane; i < TILE_SLOTS * width; i += 64) dst[i] = cols[(i / width) * COLS_G + i % width];
    }
}

// ---------------------------------------------------------------------------
// k-mer set construction, wave-cooperative (replaces one thread per k-mer with a per-thread minimizer loop and eight
// volatile key loads each): the SAME front end as k_probe — one wave per tile of 512 positions, per 64-lane batch
// canonical keys, minimizer by the sliding DPP minimum, runs of equal home line, the batch's lines staged into LDS
// with coalesced 128-byte fetches — then every lane scans its line's snapshot:
//   key found (every later genome's common case: 85-99 % of its k-mers exist already)  ->  OR the genome's bit into
//       the slot's mask word (a plain store when the snapshot shows the bit missing: see lane_insert_grp's note on
//       the one-writer invariant) or, in counting mode, atomicAdd
//   key absent in the snapshot  ->  (position, group) goes to the wave's LDS queue; the queue is worked off densely,
//       64 entries at a time, by the CAS-claiming insert (wave_insert_batch: lane_insert_grp's protocol — claims race
//       correctly against other waves — with one compare-and-swap per address and round; the group id is handed over)
// counters[0] += newly claimed keys; counters[1] = overflow flag (a probe sequence exceeded max_probe lines).
// ---------------------------------------------------------------------------
constexpr int INSERT_QCAP = 256;

// The claiming insert for a batch of 64 queue entries, wave-cooperative.  The protocol is lane_insert_grp's (a key may
// be claimed in a slot only by someone who has seen every earlier slot of its sequence hold OTHER keys; slots never
// revert), but the lanes of a run — neighbouring queue entries of one minimizer group walk the same lines in step —
// no longer each throw their own compare-and-swap at the run's next free slot: per round only the FIRST of the lanes
// that aim at an address issues the CAS, and what the slot holds afterwards (its own key if it won, else the key it
// found there) is handed to the others, who compare and move on.  A device-scope CAS costs far more than anything
// else here (3.2 of them per new key were 11 of the first genome's 13 ms at config 2); now about one per new key.
// A line is read with 8 relaxed atomic loads in flight together (volatile loads are waited for one by one).
// r: 0 = existed, 1 = newly claimed, -1 = gave up after max_probe lines.
// CLAIM = false (update-only builds, pg_table_update_seqset): a key the table does not hold is left out — the walk ends at
// the first line that is not full, nothing is claimed.
template <bool COUNT, bool CLAIM = true>
__device__ __forceinline__ int wave_insert_batch(const SubTable &st, bool valid, uint64_t key, uint32_t grp, int w, uint32_t bits,
                                                 uint32_t max_probe, int lane) {
    // (byte-mask layout: the walk sees the key's HALF of every line — seven keys at `hoff`, slots numbered 0..6 within it; lanes of a
    // run whose keys live in different halves aim at different addresses and form groups of their own below)
    const bool bm = st.layout == LAYOUT_BYTEMASK;
    const uint32_t kstride = key_stride(st), slots = bm ? BM_HALF_KEYS : st.slots, hoff = bm ? half_offset_of_key(key) : 0u;
    auto slot_key = [&](uint32_t line, uint32_t sl) __attribute__((always_inline)) {
        return reinterpret_cast<unsigned long long *>(st.buckets + (uint64_t)line * line_bytes(st) + hoff + kstride * sl);
    };
    uint32_t b = home_of_group(grp, st.nbuckets), step = step_of_group(grp, st.nbuckets), probes = 0;
    int s = -1;  // slot to try next in line b; -1: the line has not been read yet; slots: the line is full
    bool done = !valid, fresh = false;  // fresh: the line has just been read, s is its first empty slot
    int r = 0;
    auto shfl64 = [](uint64_t v, int src) __attribute__((always_inline)) {
        return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32);
    };
    auto resolve = [&](uint32_t sl, bool claimed) __attribute__((always_inline)) {
        if (bm) {  // (never a counting table: pg_api.hip)
            mask_byte_or<false>(st.buckets + (uint64_t)b * 128u + hoff + BM_MASK0 + sl, bits, claimed);
            r = claimed ? 1 : 0;
            done = true;
            return;
        }
        uint32_t *mp = mask_ptr(st, b, sl, (uint32_t)w);
        if (COUNT) {
            if (*mp < 0xFFFFFF00u) atomicAdd(mp, bits);  // saturates far above any -ci threshold
        } else if (claimed) {
            *reinterpret_cast<volatile uint32_t *>(mp) = bits;  // a fresh slot's mask words are zero (lane_insert_grp's note on racing writers applies)
        } else {
            const uint32_t cur = *mp;
            if ((cur & bits) != bits) *reinterpret_cast<volatile uint32_t *>(mp) = cur | bits;
        }
        r = claimed ? 1 : 0;
        done = true;
    };
    while (__ballot(!done)) {
        if (!done && s >= (int)slots) {  // on to the next line of the sequence
            if (++probes >= max_probe) {
                done = true;
                r = -1;
            } else {
                advance_line(key, probes, st.nbuckets, b, step);
                s = -1;
            }
        }
        if (!done && s < 0) {  // read the line: the key itself, or the first empty slot (lines fill front to back)
            uint8_t *base = st.buckets + (uint64_t)b * line_bytes(st) + hoff;
            int hit = -1, fr = -1;
            for (uint32_t s0 = 0; s0 < slots; s0 += 8) {
                uint64_t kk[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    kk[i] = __hip_atomic_load(reinterpret_cast<unsigned long long *>(base + kstride * (s0 + i)), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
                    if (s0 + (uint32_t)i >= slots) kk[i] = TOMB_KEY;  // (inline layout: mask words behind the line's 5 or 6 keys — neither a key nor empty)
                }
                int h8 = -1, f8 = -1;
#pragma unroll
                for (int i = 7; i >= 0; --i) {
                    h8 = (kk[i] == key) ? i : h8;
                    f8 = (kk[i] == EMPTY_KEY) ? i : f8;
                }
                if (hit < 0 && h8 >= 0) hit = (int)s0 + h8;
                if (fr < 0 && f8 >= 0) fr = (int)s0 + f8;
            }
            if (hit >= 0) resolve((uint32_t)hit, false);
            else if (!CLAIM && fr >= 0) done = true;  // not in a line that is not full: the table does not hold it
            else {
                s = fr >= 0 ? fr : (int)slots;
                fresh = true;
            }
        }
        if constexpr (!CLAIM) continue;  // (s is -1 or slots here: read the next line, or finished)
        // The lanes of a run that have just read their line claim DISTINCT slots in one round: first empty slot + rank
        // in the run.  A claim made this way has not yet seen the slots below it; it sees them right after — every slot
        // of the run's range is occupied once the round is over, and what each holds comes back with its lane's CAS —
        // and if a LOWER one turns out to hold the same key (an equal key further up in the run, or another wave's
        // claim that landed in between), the claim is retired (TOMB_KEY) and the key counts as found below.  Two
        // racing claims of one key in one line always see each other from the higher slot (its range reaches down to
        // what was the first empty slot when it read the line, and the lower claim was not there yet or it would
        // have been found), so exactly the lower copy survives.  Not in counting mode: a count added to a copy that
        // is retired afterwards would be lost.
        if (!COUNT) {
            const bool sp = !done && fresh && s < (int)slots;
            const unsigned long long spmask = __ballot(sp);
            if (spmask) {
                const uint64_t gaddr = sp ? reinterpret_cast<uint64_t>(slot_key(b, (uint32_t)s)) : 0;  // (line, first empty slot)
                const uint64_t gprev = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)gaddr, 1) | ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(gaddr >> 32), 1) << 32);
                const bool gl = sp && (lane == 0 || gprev != gaddr);
                const unsigned long long glmask = __ballot(gl);
                const unsigned long long below = glmask & ((2ull << lane) - 1ull);
                const int g0 = below ? 63 - __builtin_clzll(below) : lane;  // first lane of this lane's group
                const unsigned long long ends = (glmask | ~spmask) & ~((2ull << g0) - 1ull);
                const int gend = ends ? __builtin_ctzll(ends) : 64;
                const uint32_t mm = sp ? min((uint32_t)(gend - g0), slots - (uint32_t)s) : 0u;  // slots the group goes for
                const int t = s + (lane - g0);
                const bool part = sp && t < (int)slots;
                uint64_t content = 0;
                bool won = false;
                if (part) {
                    const unsigned long long cur = atomicCAS(slot_key(b, (uint32_t)t), (unsigned long long)EMPTY_KEY, (unsigned long long)key);
                    won = cur == EMPTY_KEY;
                    content = won ? key : cur;
                }
                int pos = -1;  // lowest slot of the group's range that holds this lane's key
                for (uint32_t i = 0; i < slots; ++i) {  // (wave-uniform trip count)
                    const uint64_t c = shfl64(content, min(g0 + (int)i, 63));
                    if (i < mm && pos < 0 && c == key) pos = s + (int)i;
                }
                if (sp) {
                    if (pos >= 0) {
                        const bool mine = part && won && pos == t;
                        if (part && won && pos != t) *reinterpret_cast<volatile unsigned long long *>(slot_key(b, (uint32_t)t)) = TOMB_KEY;
                        resolve((uint32_t)pos, mine);
                    } else {
                        s += (int)mm;  // other keys all the way: on behind them, one slot per round from here
                    }
                }
            }
        }
        fresh = false;
        // one compare-and-swap round among the lanes that have a slot to try
        const bool want = !done && s >= 0 && s < (int)slots;
        unsigned long long *kp = want ? slot_key(b, (uint32_t)s) : nullptr;
        const uint64_t addr = reinterpret_cast<uint64_t>(kp);
        const uint64_t prev = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)addr, 1) | ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(addr >> 32), 1) << 32);
        const bool leader = want && (lane == 0 || prev != addr);  // (a lane without a slot to try carries address 0)
        uint64_t content = 0;
        bool won = false;
        if (leader) {
            const unsigned long long cur = atomicCAS(kp, (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            won = cur == EMPTY_KEY;
            content = won ? key : cur;
        }
        const unsigned long long lmask = __builtin_amdgcn_ballot_w64(leader);
        if (__ballot(want)) {
            const unsigned long long below = lmask & ((2ull << lane) - 1ull);
            const int mine = below ? 63 - __builtin_clzll(below) : lane;  // the leader this lane follows
            const uint64_t got = (uint64_t)(uint32_t)__shfl((int)(uint32_t)content, mine) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(content >> 32), mine) << 32);
            if (want) {
                if (got == key) resolve((uint32_t)s, leader && won);
                else ++s;
            }
        }
    }
    return r;
}

template <int W_C, bool M64>
__global__ __launch_bounds__(64) void k_insert_tile(const SubTable st, int w, uint32_t bits, uint32_t count_mode,
                                                    const uint64_t *__restrict__ seqw, const uint32_t *__restrict__ nmw,
                                                    const uint32_t *__restrict__ has_n, const SeqDesc *__restrict__ sd,
                                                    const uint32_t *__restrict__ tile0, uint32_t ncontigs,
                                                    unsigned long long *__restrict__ counters, uint32_t max_probe) {
    constexpr int SLOTS = 8;  // 16-byte chunks of a 128-byte line (8 slots, or 16 bare keys in the split layout)
    constexpr int LDS_LINE_U4 = SLOTS + 1;
    constexpr int STAGE_ITERS = (PROBE_MAXRUN * SLOTS + 63) / 64;
    __shared__ uint64_t sw[PROBE_SEQW];
    __shared__ uint64_t rw[PROBE_SEQW + 1];
    __shared__ uint32_t nw[PROBE_SEQW];
    __shared__ uint32_t lines_w[PROBE_MAXRUN];
    __shared__ uint4 buf[((STAGE_ITERS * 64 + SLOTS - 1) / SLOTS) * LDS_LINE_U4];
    __shared__ uint32_t q_grp[INSERT_QCAP];
    __shared__ uint16_t q_pl[INSERT_QCAP];
    const int lane = threadIdx.x;
    const int k = (int)st.k;
    const bool split = st.layout == LAYOUT_SPLIT;  // (uniform)
    const bool update_only = (count_mode & 2u) != 0;  // pg_table_update_seqset: bits for keys already there, no new keys
    count_mode &= 1u;
    const uint32_t tile = blockIdx.x;
    uint32_t c = 0;  // contig of the tile: last c with tile0[c] <= tile (uniform binary search)
    {
        uint32_t lo = 0, hi = ncontigs;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tile0[mid] <= tile) lo = mid;
            else hi = mid;
        }
        c = lo;
    }
    const SeqDesc s = sd[c];
    const uint32_t nkmers = (uint32_t)(s.len - (uint64_t)k + 1);
    const uint32_t tile_start = (tile - tile0[c]) * PROBE_TILE;
    const uint32_t npos = min((uint32_t)PROBE_TILE, nkmers - tile_start);
    const bool hasn = has_n[c] != 0;
    for (int i = lane; i < PROBE_SEQW; i += 64) {
        const uint64_t wi = (uint64_t)(tile_start >> 5) + i;
        const uint64_t wv = wi < s.nwords ? seqw[s.seq_off + wi] : 0ull;
        sw[i] = wv;
        rw[PROBE_SEQW - 1 - i] = pair_reverse64(~wv);
        nw[i] = (hasn && wi < s.nwords) ? nmw[s.seq_off + wi] : 0u;
    }
    if (lane == 0) rw[PROBE_SEQW] = 0;  // (a window's three dwords may reach one word past the end)
    __syncthreads();
    const uint64_t kmask = W_C ? (((uint64_t)(k == 32 ? ~0u : ((1u << (2 * k - 32)) - 1u)) << 32) | 0xFFFFFFFFull) : kmer_mask(k);  // (as in k_probe)
    const uint32_t rcb = PROBE_SEQ_BASES - (uint32_t)k;
    constexpr int HALO = W_C ? W_C - 1 : 0;
    constexpr int STRIDE = 64 - HALO;
    const uint32_t m = W_C ? (uint32_t)k - W_C + 1 : 0;
    const uint64_t mm64 = (m >= 32) ? ~0ull : ((1ull << (2 * (m ? m : 1))) - 1);
    uint32_t qn = 0, claimed = 0;  // (wave-uniform)
    bool overflowed = false;

    auto drain = [&]() {  // the queued (absent) keys through the claiming insert, 64 at a time
        __syncthreads();
        for (uint32_t e0 = 0; e0 < qn; e0 += 64) {
            const uint32_t e = e0 + lane;
            const bool valid = e < qn;
            const uint32_t ec = valid ? e : qn - 1;
            const uint64_t key = canonical_from_le(extract_bases32(reinterpret_cast<const uint32_t *>(sw), q_pl[ec]), k);
            const int r = update_only ? wave_insert_batch<false, false>(st, valid, key, q_grp[ec], w, bits, max_probe, lane)
                          : count_mode ? wave_insert_batch<true>(st, valid, key, q_grp[ec], w, bits, max_probe, lane)
                                       : wave_insert_batch<false>(st, valid, key, q_grp[ec], w, bits, max_probe, lane);
            overflowed |= __ballot(r < 0) != 0;
            claimed += (uint32_t)__popcll(__ballot(r > 0));
        }
        qn = 0;
        __syncthreads();
    };

    uint32_t adv = STRIDE;  // positions the batch covers (k_probe's CUT: a batch ends in front of its (PROBE_MAXRUN + 1)-th run)
    for (uint32_t b = 0; b < npos; b += adv) {
        const int32_t pl = (int32_t)(b + lane) - HALO;
        const bool inrange = pl >= (int32_t)b && pl < (int32_t)npos;
        const uint32_t pq = (uint32_t)max(pl, 0);
        const uint64_t X = extract_bases32(reinterpret_cast<const uint32_t *>(sw), pq) & kmask;
        const uint64_t B = revcomp_window(rw, pq, kmask, rcb);
        const uint64_t key = ~(X > B ? X : B) & kmask;
        bool act = inrange;
        if (hasn) act = act && (extract_nmask(nw, pq, k) == 0);
        uint32_t grp;
        if (W_C) {
            const uint32_t off = (uint32_t)(pl + HALO) - pq;
            if constexpr (!M64) {
                const uint32_t mm32 = (uint32_t)mm64;
                const uint32_t fa = __builtin_amdgcn_alignbit((uint32_t)(X >> 32), (uint32_t)X, 2 * off) & mm32;
                const uint32_t fr = __builtin_amdgcn_alignbit((uint32_t)(B >> 32), (uint32_t)B, 2 * (HALO - off)) & mm32;
                grp = mz_order(min(fa, fr));
            } else {
                const uint64_t fa = (X >> (2 * off)) & mm64;
                const uint64_t fr = (B >> (2 * (HALO - off))) & mm64;
                grp = mmer_rank(fa < fr ? fa : fr);
            }
            grp = sliding_min<W_C ? W_C : 1>(grp);
        } else {
            grp = group_of_key(key);
        }
        const uint32_t line = home_of_group(grp, st.nbuckets);
        const uint32_t prev_line = lane_up1(line);
        unsigned long long amask = __builtin_amdgcn_ballot_w64(act);  // (run starts by lane-mask arithmetic on the scalar unit, as in k_probe)
        unsigned long long lmask = amask & (~(amask << 1) | __builtin_amdgcn_ballot_w64(line != prev_line));
        const uint32_t rid = lanes_le_index(lmask, 0u);
        if constexpr (W_C != 0) {  // one staging step per batch: the lanes behind the PROBE_MAXRUN-th run are the next batch's
            const unsigned long long keep = __builtin_amdgcn_sicmp((int32_t)rid, PROBE_MAXRUN, 40 /* signed < */);
            amask &= keep;
            lmask &= keep;
            act = __builtin_amdgcn_inverse_ballot_w64(amask);
            adv = (uint32_t)__popcll(keep) - HALO;
        }
        const bool leader = __builtin_amdgcn_inverse_ballot_w64(lmask);
        const uint32_t nruns = (uint32_t)__popcll(lmask);
        bool found = false, full = true;  // full: the staged home line had no empty slot (or was not reached)
        for (uint32_t r0 = 0; r0 < nruns; r0 += PROBE_MAXRUN) {
            const uint32_t nl = min((uint32_t)PROBE_MAXRUN, nruns - r0);
            if (leader && rid - r0 < nl) lines_w[rid - r0] = line;
            __syncthreads();
            uint4 v[STAGE_ITERS];
#pragma unroll
            for (int it = 0; it < STAGE_ITERS; ++it) {
                const uint32_t ls = min((uint32_t)(it * (64 / SLOTS) + lane / SLOTS), nl - 1u);
                v[it] = *reinterpret_cast<const uint4 *>(st.buckets + (((uint64_t)lines_w[ls] * 128u) | ((lane % SLOTS) * 16u)));
            }
#pragma unroll
            for (int it = 0; it < STAGE_ITERS; ++it) {
                const uint32_t idx = it * 64 + lane;
                buf[(idx / SLOTS) * LDS_LINE_U4 + (idx % SLOTS)] = v[it];
            }
            __syncthreads();
            if (act && rid - r0 < nl) {
                const uint4 *ln = buf + (rid - r0) * LDS_LINE_U4;
                uint32_t *mp = nullptr;
                uint32_t cur = 0;
                if (st.layout == LAYOUT_INLINE) {  // (uniform)
                    uint32_t slot1;
                    full = scan_keys_inl(ln, key, st.slots, slot1) < 0;
                    if (slot1) {
                        found = true;
                        mp = mask_ptr(st, line, slot1 - 1u, (uint32_t)w);
                        cur = *reinterpret_cast<const volatile uint32_t *>(mp);
                    }
                } else if (split) {
                    uint32_t slot1;
                    full = scan_keys16_lds<true>(ln, key, slot1) < 0;
                    if (slot1) {
                        found = true;
                        mp = reinterpret_cast<uint32_t *>(st.masks) + ((uint64_t)line * SPLIT_KEYS + (slot1 - 1u)) * st.W + (uint32_t)w;
                        cur = *reinterpret_cast<const volatile uint32_t *>(mp);
                    }
                } else if (st.layout == LAYOUT_BYTEMASK) {  // (uniform) the key's half of the snapshot; the genome's bit goes into the slot's mask BYTE
                    uint32_t mb, slot = 0;
                    const int rcode = scan_line_bm<true>(ln, key, mb, &slot);
                    full = rcode < 0;
                    found = rcode > 0;
                    // (found with the bit missing: a byte store — never the dword, whose other bytes are other slots'; every writer of
                    // this byte during the launch ORs in the same bits.  mp stays null: byte-mask tables never count)
                    if (found && (mb & bits) != bits)
                        *reinterpret_cast<volatile uint8_t *>(st.buckets + (uint64_t)line * 128u + half_offset_of_key(key) + BM_MASK0 + slot) = (uint8_t)(mb | bits);
                } else {
                    uint32_t m0, m1;
                    // (the slot's byte offset is what is needed here: scan the keys like scan_line_lds does)
                    uint64_t kk[8];
#pragma unroll
                    for (int sl = 0; sl < 8; ++sl) kk[sl] = *reinterpret_cast<const uint64_t *>(ln + sl);
                    unsigned long long e[8];
#pragma unroll
                    for (int sl = 0; sl < 8; ++sl) e[sl] = __builtin_amdgcn_ballot_w64(kk[sl] == key);
                    {  // a snapshot taken during this launch may show a key twice (a claim about to be retired, see
                       // wave_insert_batch): the LOWEST slot counts — a lane's match there masks its later ones (scalar unit)
                        unsigned long long seen = e[0];
#pragma unroll
                        for (int sl = 1; sl < 8; ++sl) {
                            const unsigned long long m = e[sl];
                            e[sl] = m & ~seen;
                            seen |= m;
                        }
                    }
                    const unsigned long long b0 = e[1] | e[3] | e[5] | e[7], b1 = e[2] | e[3] | e[6] | e[7], b2 = e[4] | e[5] | e[6] | e[7];
                    full = kk[7] != EMPTY_KEY;
                    (void)m0;
                    (void)m1;
                    if (__builtin_amdgcn_inverse_ballot_w64(b0 | b1 | b2 | e[0])) {
                        found = true;
                        const uint32_t off = (__builtin_amdgcn_inverse_ballot_w64(b0) ? 16u : 0u) | (__builtin_amdgcn_inverse_ballot_w64(b1) ? 32u : 0u) |
                                             (__builtin_amdgcn_inverse_ballot_w64(b2) ? 64u : 0u);
                        cur = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(ln) + off + 8 + 4 * w);
                        mp = reinterpret_cast<uint32_t *>(st.buckets + (uint64_t)line * 128u + off + 8 + 4 * w);
                    }
                }
                if (found && mp) {
                    if (count_mode) {
                        if (cur < 0xFFFFFF00u) atomicAdd(mp, bits);
                    } else if ((cur & bits) != bits) {
                        *reinterpret_cast<volatile uint32_t *>(mp) = cur | bits;
                    }
                }
            }
            __syncthreads();
        }
        // absent from the snapshot of its line (or the line was not reached): queue for the claiming insert
        // (update-only: a key missing from a home line that is not full is not in the table — lines fill front to back)
        const bool todo = act && !found && (!update_only || full);
        const unsigned long long tmask = __builtin_amdgcn_ballot_w64(todo);
        if (tmask) {
            if (qn + 64 > (uint32_t)INSERT_QCAP) drain();
            if (todo) {
                const uint32_t slot = lanes_le_index(tmask, qn);
                q_grp[slot] = grp;
                q_pl[slot] = (uint16_t)pl;
            }
            qn += (uint32_t)__popcll(tmask);
        }
    }
    if (qn) drain();
    if (lane == 0) {
        if (claimed) atomicAdd(&counters[0], (unsigned long long)claimed);
        if (overflowed) atomicOr(reinterpret_cast<unsigned int *>(&counters[1]), 1u);
    }
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
template <int W_C, bool TWO, int ROWMODE, int SLOTS>
static hipError_t probe_t(hipStream_t s, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw,
                          const uint32_t *has_n, const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig,
                          const uint32_t *sched, uint32_t tile_base, uint8_t *out1, uint32_t nbytes, const RowCols &rc, const FuseArgs *fuse) {
    const bool m64 = W_C && st.m > 16;
    if constexpr (SLOTS == 8 && ROWMODE != 1 && ROWMODE != 3) {  // (the fused instantiations: rows of 2..8 bytes, 8-slot lines)
        if (fuse) {
            if (m64)
                hipLaunchKernelGGL((k_probe<W_C, TWO, ROWMODE, SLOTS, true, false, false, true>), dim3(ntiles), dim3(64), 0, s, st, seqw, nmw, has_n, sd, ad,
                                   tile_contig, sched, tile_base, out1, nbytes, rc, *fuse);
            else
                hipLaunchKernelGGL((k_probe<W_C, TWO, ROWMODE, SLOTS, false, false, false, true>), dim3(ntiles), dim3(64), 0, s, st, seqw, nmw, has_n, sd, ad,
                                   tile_contig, sched, tile_base, out1, nbytes, rc, *fuse);
            return hipGetLastError();
        }
    }
    if (fuse) return hipErrorInvalidValue;  // (launch_anchor only asks for what is instantiated)
    const FuseArgs none = {nullptr, nullptr, nullptr, 0, 0, 0};
    if (m64)
        hipLaunchKernelGGL((k_probe<W_C, TWO, ROWMODE, SLOTS, true>), dim3(ntiles), dim3(64), 0, s, st, seqw, nmw, has_n, sd, ad,
                           tile_contig, sched, tile_base, out1, nbytes, rc, none);
    else
        hipLaunchKernelGGL((k_probe<W_C, TWO, ROWMODE, SLOTS, false>), dim3(ntiles), dim3(64), 0, s, st, seqw, nmw, has_n, sd, ad,
                           tile_contig, sched, tile_base, out1, nbytes, rc, none);
    return hipGetLastError();
}

template <int W_C>
static hipError_t probe_w(hipStream_t s, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw,
                          const uint32_t *has_n, const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig,
                          const uint32_t *sched, uint32_t tile_base, uint8_t *out1, uint32_t nbytes, const RowCols &rc, int rowmode,
                          const FuseArgs *fuse = nullptr) {
#define PG_A s, ntiles, st, seqw, nmw, has_n, sd, ad, tile_contig, sched, tile_base, out1, nbytes, rc, fuse
#define PG_K s, st, seqw, nmw, has_n, sd, ad, tile_contig, sched, tile_base, out1, nbytes, rc
    const FuseArgs none = {nullptr, nullptr, nullptr, 0, 0, 0};
    const bool m64 = W_C && st.m > 16;
    if (st.layout == LAYOUT_INLINE || st.layout == LAYOUT_SPLIT) {
        // more than 64 genomes: keys and their mask blocks in one line (inline, 65..96 genomes), or key lines + mask array (split)
        const bool inl = st.layout == LAYOUT_INLINE;
        if (fuse && (nbytes > 16u || !PG_FUSE_WIDE)) return hipErrorInvalidValue;
        if (inl) {
            if (fuse) {
#if PG_FUSE_WIDE
                if (m64) hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, true, true, true, true>), dim3(ntiles), dim3(64), 0, PG_K, *fuse);
                else hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, false, true, true, true>), dim3(ntiles), dim3(64), 0, PG_K, *fuse);
#endif
            } else {
                if (m64) hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, true, true, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
                else hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, false, true, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
            }
        } else {
            if (fuse) {
#if PG_FUSE_WIDE
                if (m64) hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, true, true, false, true>), dim3(ntiles), dim3(64), 0, PG_K, *fuse);
                else hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, false, true, false, true>), dim3(ntiles), dim3(64), 0, PG_K, *fuse);
#endif
            } else {
                if (m64) hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, true, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
                else hipLaunchKernelGGL((k_probe<W_C, false, 0, 8, false, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
            }
        }
        return hipGetLastError();
    }
    if (st.layout == LAYOUT_BYTEMASK) {  // up to 8 genomes: one-byte rows, or the sharded mode's bit columns — nothing else occurs
        if (fuse || (rowmode != 1 && rowmode != 3)) return hipErrorInvalidValue;
        if (rowmode == 1) {
            if (m64) hipLaunchKernelGGL((k_probe<W_C, false, 1, 8, true, false, false, false, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
            else hipLaunchKernelGGL((k_probe<W_C, false, 1, 8, false, false, false, false, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
        } else {
            if (m64) hipLaunchKernelGGL((k_probe<W_C, false, 3, 8, true, false, false, false, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
            else hipLaunchKernelGGL((k_probe<W_C, false, 3, 8, false, false, false, false, true>), dim3(ntiles), dim3(64), 0, PG_K, none);
        }
        return hipGetLastError();
    }
    if (st.slots == 16) {
        if (st.W == 2) {
            if (rowmode == 2) return probe_t<W_C, true, 2, 16>(PG_A);
            return probe_t<W_C, true, 0, 16>(PG_A);
        }
        if (rowmode == 1) return probe_t<W_C, false, 1, 16>(PG_A);
        return probe_t<W_C, false, 0, 16>(PG_A);
    }
    if (st.W == 2) {
        if (rowmode == 2) return probe_t<W_C, true, 2, 8>(PG_A);
        return probe_t<W_C, true, 0, 8>(PG_A);
    }
    if (rowmode == 3) return probe_t<W_C, false, 3, 8>(PG_A);
    if (rowmode == 1) return probe_t<W_C, false, 1, 8>(PG_A);
    if (rowmode == 4) return probe_t<W_C, false, 4, 8>(PG_A);
    if (rowmode == 5) return probe_t<W_C, false, 5, 8>(PG_A);
    if (rowmode == 6) return probe_t<W_C, false, 6, 8>(PG_A);
    return probe_t<W_C, false, 0, 8>(PG_A);
#undef PG_A
#undef PG_K
}

template <int W_C>
static hipError_t insert_tiles_w(hipStream_t s, uint32_t ntiles, const SubTable &st, int w, uint32_t bits, uint32_t count_mode,
                                 const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd,
                                 const uint32_t *tile0, uint32_t ncontigs, unsigned long long *counters, uint32_t max_probe) {
    if (W_C && st.m > 16)
        hipLaunchKernelGGL((k_insert_tile<W_C, true>), dim3(ntiles), dim3(64), 0, s, st, w, bits, count_mode, seqw, nmw, has_n, sd,
                           tile0, ncontigs, counters, max_probe);
    else
        hipLaunchKernelGGL((k_insert_tile<W_C, false>), dim3(ntiles), dim3(64), 0, s, st, w, bits, count_mode, seqw, nmw, has_n, sd,
                           tile0, ncontigs, counters, max_probe);
    return hipGetLastError();
}

// the parts' entry points: the windows a unit instantiates (see the top of the file)
#define PG_PROBE_ARGS hipStream_t s, uint32_t w, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, \
                      const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig, const uint32_t *sched, uint32_t tile_base, uint8_t *out1,          \
                      uint32_t nbytes, const RowCols &rc, int rowmode, const FuseArgs *fuse
#define PG_PROBE_CASE(W) case W: return probe_w<W>(s, ntiles, st, seqw, nmw, has_n, sd, ad, tile_contig, sched, tile_base, out1, nbytes, rc, rowmode, fuse);
#define PG_INSERT_ARGS hipStream_t s, uint32_t win, uint32_t ntiles, const SubTable &st, int w, uint32_t bits, uint32_t count_mode, const uint64_t *seqw, \
                       const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd, const uint32_t *tile0, uint32_t ncontigs,                          \
                       unsigned long long *counters, uint32_t max_probe
#define PG_INSERT_CASE(W) case W: return insert_tiles_w<W>(s, ntiles, st, w, bits, count_mode, seqw, nmw, has_n, sd, tile0, ncontigs, counters, max_probe);
// (each unit is a code object of its own, loaded by the HIP runtime when the first of its kernels is asked for: preload_anchor_kernels asks)
#if PG_HAS_PART(1)
hipError_t preload_part1() {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_insert_tile<6, false>));
}
#endif
#if PG_HAS_PART(2)
hipError_t preload_part2() {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_insert_tile<7, false>));
}
#endif
#if PG_HAS_PART(0)
hipError_t probe_part0(PG_PROBE_ARGS) {
    switch (w) { PG_PROBE_CASE(0) PG_PROBE_CASE(3) PG_PROBE_CASE(4) default: return hipErrorInvalidValue; }
}
hipError_t insert_part0(PG_INSERT_ARGS) {
    switch (win) { PG_INSERT_CASE(0) PG_INSERT_CASE(3) PG_INSERT_CASE(4) default: return hipErrorInvalidValue; }
}
#endif
#if PG_HAS_PART(1)
hipError_t probe_part1(PG_PROBE_ARGS) {
    switch (w) { PG_PROBE_CASE(5) PG_PROBE_CASE(6) default: return hipErrorInvalidValue; }
}
hipError_t insert_part1(PG_INSERT_ARGS) {
    switch (win) { PG_INSERT_CASE(5) PG_INSERT_CASE(6) default: return hipErrorInvalidValue; }
}
#endif
#if PG_HAS_PART(2)
hipError_t probe_part2(PG_PROBE_ARGS) {
    switch (w) { PG_PROBE_CASE(7) PG_PROBE_CASE(8) default: return hipErrorInvalidValue; }
}
hipError_t insert_part2(PG_INSERT_ARGS) {
    switch (win) { PG_INSERT_CASE(7) PG_INSERT_CASE(8) default: return hipErrorInvalidValue; }
}
#endif
#undef PG_PROBE_ARGS
#undef PG_PROBE_CASE
#undef PG_INSERT_ARGS
#undef PG_INSERT_CASE

#if PG_MAIN_PART  // ======== the launchers: part 0 (or the one unit) only ========
// the kernel's compile-time window must be the one the table was built with: the part that instantiates it
static hipError_t probe_window(hipStream_t s, uint32_t w, uint32_t ntiles, const SubTable &st, const uint64_t *seqw, const uint32_t *nmw,
                               const uint32_t *has_n, const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig, const uint32_t *sched,
                               uint32_t tile_base, uint8_t *out1, uint32_t nbytes, const RowCols &rc, int rowmode, const FuseArgs *fuse) {
    auto *part = (w == 0 || w == 3 || w == 4) ? probe_part0 : (w == 5 || w == 6) ? probe_part1 : (w == 7 || w == 8) ? probe_part2 : nullptr;
    if (!part) return hipErrorInvalidValue;
    return part(s, w, ntiles, st, seqw, nmw, has_n, sd, ad, tile_contig, sched, tile_base, out1, nbytes, rc, rowmode, fuse);
}

static int row_mode(uint32_t nbytes, const RowCols &rc) {
    if (nbytes == 1) return 1;
    if (nbytes == 8 && rc.col0 == 0 && rc.nb0 == 4 && rc.nb1 == 4) return 2;
    if (nbytes == 4 && rc.col0 == 0 && rc.nb0 == 4 && rc.nb1 == 0) return 4;
    if (nbytes == 2 && rc.col0 == 0 && rc.nb1 == 0) return 5;
    if (nbytes == 3 && rc.col0 == 0 && rc.nb1 == 0) return 6;
    return 0;
}

// columns_width != 0: the genome-sharded mode's narrow tables (up to 8 genomes, 8-slot or byte-mask lines) emit the block's bit
// columns (`columns_width` genomes wide) into `out1` instead of rows
hipError_t launch_anchor(hipStream_t s, const TableDesc &T, const uint64_t *seqw, const uint32_t *nmw,
                         const uint32_t *has_n, const SeqDesc *sd, const AnchorDesc *ad, const uint32_t *tile_contig,
                         const uint32_t *sched, uint32_t tile_base, uint32_t ntiles, uint8_t *out1, uint64_t out1_bytes,
                         uint32_t columns_width, const FuseArgs *fuse) {
    if (ntiles == 0) return hipSuccess;
    const uint32_t nbytes = (T.ngenomes + 7) / 8;
    hipError_t e = hipSuccess;
    (void)out1_bytes;
    // fused statistics: one sub-table writes whole rows of 2..16 bytes, 8-slot / inline / split lines (pg_api.hip asks only then)
    if (fuse && (columns_width || T.nsub != 1 || !fuse_rows_ok(nbytes) || fuse->ngenomes != T.ngenomes ||
                 (T.sub[0].layout == LAYOUT_SLOTS && T.sub[0].slots != 8)))
        return hipErrorInvalidValue;
    if (columns_width) {
        const SubTable &st = T.sub[0];
        if (T.nsub != 1 || !((st.layout == LAYOUT_SLOTS && st.slots == 8) || st.layout == LAYOUT_BYTEMASK) || st.W != 1 || T.ngenomes > (uint32_t)COLS_G ||
            columns_width > (uint32_t)COLS_G || columns_width < T.ngenomes)
            return hipErrorInvalidValue;
        RowCols rc;
        rc.col0 = T.ngenomes;  // (genomes of the block)
        rc.nb0 = rc.nb1 = rc.words = 0;
        const uint32_t w = st.m ? st.k - st.m + 1 : 0;
        return probe_window(s, w, ntiles, st, seqw, nmw, has_n, sd, ad, tile_contig, sched, tile_base, out1, columns_width, rc, 3, nullptr);
    }
    for (uint32_t si = 0; si < T.nsub; ++si) {
        const SubTable &st = T.sub[si];
        RowCols rc;  // every sub-table writes all bytes of the columns it owns, so rows need no zero fill
        rc.col0 = 4 * st.word0;
        rc.nb0 = min(4u, nbytes - rc.col0);
        rc.nb1 = (st.W == 2 && nbytes > rc.col0 + 4) ? min(4u, nbytes - rc.col0 - 4) : 0;
        rc.words = (nbytes % 4 == 0 && rc.nb0 == 4 && (rc.nb1 == 0 || rc.nb1 == 4)) ? 1u : (nbytes == 2 ? 2u : 0u);
        if (T.nsub == 1 && (nbytes == 3 || (nbytes >= 5 && nbytes <= 7))) rc.words = 3u;
        if (rc.words == 1 && rc.nb1 == 4 && rc.col0 % 8 == 0 && nbytes % 8 == 0) rc.words = 4u;  // (one 8-byte store per row: -9 % probe time at N=128)
        const int rm = (T.nsub == 1) ? row_mode(nbytes, rc) : 0;
        const uint32_t w = st.m ? st.k - st.m + 1 : 0;
        e = probe_window(s, w, ntiles, st, seqw, nmw, has_n, sd, ad, tile_contig, sched, tile_base, out1, nbytes, rc, rm, fuse);
        if (e != hipSuccess) return e;
    }
    return e;
}

#ifdef PG_PHASE_TIMING
}  // namespace pg
extern "C" int pg_debug_phase_cycles(unsigned long long *out16, int reset) {
    hipDeviceSynchronize();
    static unsigned long long all[1024 * 16];
    if (hipMemcpyFromSymbol(all, HIP_SYMBOL(pg::pg_phase_cycles), sizeof all) != hipSuccess) return -1;
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    for (int b = 0; b < 1024; ++b)
        for (int i = 0; i < 16; ++i) out16[i] += all[b * 16 + i];
    if (reset) {
        for (auto &x : all) x = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(pg::pg_phase_cycles), all, sizeof all) != hipSuccess) return -1;
    }
    return 0;
}
namespace pg {
#endif
hipError_t preload_anchor_kernels() {  // (any kernel of this unit loads its code object; the other parts' load with their first launch)
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_insert_tile<4, false>));
    if (e == hipSuccess) e = preload_part1();
    if (e == hipSuccess) e = preload_part2();
    return e;
}

// every k-mer of the contigs described by sd / tile0 (tile0[c] = first tile of contig c; tile0[ncontigs] = ntiles)
hipError_t launch_insert_tiles(hipStream_t s, const SubTable &st, int w, uint32_t bits, int count_mode, const uint64_t *seqw,
                               const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd, const uint32_t *tile0,
                               uint32_t ncontigs, uint32_t ntiles, unsigned long long *counters, uint32_t max_probe) {
    if (ntiles == 0) return hipSuccess;
    const uint32_t win = st.m ? st.k - st.m + 1 : 0;
    auto *part = (win == 0 || win == 3 || win == 4) ? insert_part0 : (win == 5 || win == 6) ? insert_part1 : (win == 7 || win == 8) ? insert_part2 : nullptr;
    if (!part) return hipErrorInvalidValue;
    return part(s, win, ntiles, st, w, bits, (uint32_t)count_mode, seqw, nmw, has_n, sd, tile0, ncontigs, counters, max_probe);
}
#endif  // PG_MAIN_PART

}  // namespace pg
