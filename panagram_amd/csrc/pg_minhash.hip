// pg_minhash.hip — MinHash sketches of packed samples ON THE GPU (gfx950): the candidates of a bottom-s sketch.
//
// Replaces `mash sketch -s 10000` of the reference's workflow (panagram/workflow/Snakefile:124-149; mash's defaults
// k = 21, seed 42).  Per k-mer position of a packed seqset (the (contig, job) decomposition of k_sketch_set):
//   validity     the k bits of the "not ACGT" plane (extract_nmask)
//   canonical    X = LE window of the forward strand, B = that of its reverse complement (revcomp_le).  The first-base-
//                most-significant values are ~B (forward) and ~X (reverse complement), so the forward string is the
//                lexicographically smaller one iff ~B <= ~X; the canonical string's LE window is then X, else B
//   bytes        the 21 upper-case ASCII bytes in registers: codes spread to one per byte, looked up in "ACGT" by
//                v_perm_b32 (4 bytes per instruction)
//   hash         MurmurHash3_x64_128 over them (one 16-byte block, a 5-byte tail, the two fmix64), h1 kept
//   candidate    h1 <= limit: appended to a buffer, one atomic per wave (ballot + mbcnt); slots past `cap` are counted,
//                not written — count > cap is the overflow the host reruns with a larger buffer
// The host (pg_api.hip: pg_minhash_add_seqset) sorts and deduplicates the candidates and keeps the s smallest.  Each
// job also counts its ACGT bases (the p-value's sample length).
#include "pg_kernels.h"

namespace pg {

constexpr int MH_K = MINHASH_K;
constexpr uint64_t MH_C1 = 0x87c37b91114253d5ull, MH_C2 = 0x4cf5ad432745937full;

__device__ __forceinline__ uint64_t mh_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t mh_fmix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// 8 codes (2 bits each, first in the low bits) -> their 8 ASCII bytes, first in the low byte
__device__ __forceinline__ uint64_t mh_ascii8(uint32_t c) {
    uint32_t t = (c | (c << 8)) & 0x00ff00ffu;  // byte 0: codes 0-3, byte 2: codes 4-7
    t = (t | (t << 4)) & 0x0f0f0f0fu;          // byte m: code 2m (bits 0-1), code 2m + 1 (bits 2-3)
    constexpr uint32_t ACGT = 0x54474341u;     // 'A' 'C' 'G' 'T' in bytes 0..3 (both perm sources: selectors 0-7 all hit it)
    const uint32_t ev = __builtin_amdgcn_perm(ACGT, ACGT, t & 0x03030303u);         // bytes of codes 0, 2, 4, 6
    const uint32_t od = __builtin_amdgcn_perm(ACGT, ACGT, (t >> 2) & 0x03030303u);  // bytes of codes 1, 3, 5, 7
    const uint32_t lo = __builtin_amdgcn_perm(od, ev, 0x05010400u);                 // ev0 od0 ev1 od1
    const uint32_t hi = __builtin_amdgcn_perm(od, ev, 0x07030602u);                 // ev2 od2 ev3 od3
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// h1 of MurmurHash3_x64_128(seed) over the 21 ASCII bytes of the k-mer whose LE window (first base in bits 0-1) is L
__device__ __forceinline__ uint64_t mh_hash21(uint64_t L, uint64_t seed) {
    const uint64_t b0 = mh_ascii8((uint32_t)L & 0xffffu);                    // bytes 0-7
    const uint64_t b1 = mh_ascii8((uint32_t)L >> 16);                        // bytes 8-15
    const uint64_t b2 = mh_ascii8((uint32_t)(L >> 32)) & 0xffffffffffull;    // bytes 16-20 (the tail)
    uint64_t h1 = seed, h2 = seed;
    uint64_t k1 = mh_rotl(b0 * MH_C1, 31) * MH_C2;
    h1 ^= k1;
    h1 = mh_rotl(h1, 27) + h2;
    h1 = h1 * 5 + 0x52dce729u;
    uint64_t k2 = mh_rotl(b1 * MH_C2, 33) * MH_C1;
    h2 ^= k2;
    h2 = mh_rotl(h2, 31) + h1;
    h2 = h2 * 5 + 0x38495ab5u;
    h1 ^= mh_rotl(b2 * MH_C1, 31) * MH_C2;  // (a tail of 5 bytes: k1 only)
    h1 ^= (uint64_t)MH_K;
    h2 ^= (uint64_t)MH_K;
    h1 += h2;
    h2 += h1;
    return mh_fmix64(h1) + mh_fmix64(h2);
}

// job j = bases [y * MINHASH_JOB, (y + 1) * MINHASH_JOB) of contig x: the k-mers starting there, and its ACGT bases
__global__ __launch_bounds__(256) void k_minhash(const SeqDesc *__restrict__ sd, const uint2 *__restrict__ jobs,
                                                 const uint64_t *__restrict__ seqw_all, const uint32_t *__restrict__ nmw_all,
                                                 const uint32_t *__restrict__ has_n, uint64_t limit, uint64_t seed,
                                                 uint64_t *__restrict__ cand, uint64_t cap, unsigned long long *count,
                                                 unsigned long long *bases) {
    const uint2 job = jobs[blockIdx.x];
    const SeqDesc d = sd[job.x];
    const uint64_t b0 = (uint64_t)job.y * MINHASH_JOB, b1 = min(d.len, b0 + MINHASH_JOB);
    const uint64_t p1 = d.len >= (uint64_t)MH_K ? min(b1, d.len - MH_K + 1) : b0;
    const uint64_t *seqw = seqw_all + d.seq_off;
    const uint32_t *nmw = nmw_all + d.seq_off;
    const bool hasn = has_n[job.x] != 0;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));

    // ACGT bases of [b0, b1): a "not ACGT" word per 32 (b0 is a multiple of 32)
    uint32_t acgt = 0;
    if (!hasn) {
        acgt = threadIdx.x == 0 ? (uint32_t)(b1 - b0) : 0u;
    } else {
        for (uint64_t w = (b0 >> 5) + threadIdx.x; (w << 5) < b1; w += 256) {
            const uint32_t nb = (uint32_t)min<uint64_t>(32, b1 - (w << 5));
            const uint32_t lm = nb == 32 ? ~0u : ((1u << nb) - 1u);
            acgt += nb - (uint32_t)__popc(nmw[w] & lm);
        }
    }
    for (int off = 32; off > 0; off >>= 1) acgt += __shfl_xor(acgt, off);
    if (lane == 0 && acgt) atomicAdd(bases, (unsigned long long)acgt);

    const uint64_t km = (1ull << (2 * MH_K)) - 1;
    for (uint64_t q = b0; q < p1; q += 256) {  // (bounds uniform over the block: every lane reaches the ballot)
        const uint64_t p = q + threadIdx.x;
        bool take = false;
        uint64_t h = 0;
        if (p < p1 && !(hasn && extract_nmask(nmw, p, MH_K))) {
            const uint64_t X = extract_bases(seqw, p) & km;
            const uint64_t B = revcomp_le(X, MH_K);
            const uint64_t L = (~B & km) <= (~X & km) ? X : B;
            h = mh_hash21(L, seed);
            take = h <= limit;
        }
        const uint64_t bal = __ballot(take);
        if (bal == 0) continue;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)bal) - 1u;
        unsigned long long slot0 = 0;
        if (lane == leader) slot0 = atomicAdd(count, (unsigned long long)__popcll(bal));
        slot0 = __shfl(slot0, (int)leader);
        if (take) {
            const uint64_t slot = slot0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (slot < cap) cand[slot] = h;
        }
    }
}

hipError_t launch_minhash(hipStream_t st, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                          const uint32_t *nmw, const uint32_t *has_n, uint64_t limit, uint32_t seed, uint64_t *cand, uint64_t cap,
                          unsigned long long *count, unsigned long long *bases) {
    if (njobs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_minhash, dim3(njobs), dim3(256), 0, st, sd, jobs, seqw, nmw, has_n, limit, (uint64_t)seed, cand, cap,
                       count, bases);
    return hipGetLastError();
}

}  // namespace pg
