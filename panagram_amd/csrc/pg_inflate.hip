// pg_inflate.hip — BGZF blocks inflated ON THE GPU (gfx950): the read side of pg_deflate.hip.
//
// Replaces, for a bitmap.<step>.gz read back into HBM, the block-by-block host inflate of Bio.bgzf
// (the reference's BgzfReader, index.py:615-651, 827-845).  k_bgzf_inflate: one workgroup = ONE wave = one BGZF block.
//   - full RFC 1951: stored, fixed- and dynamic-Huffman blocks, any number of them per member, matches up to 32 KiB back,
//     the empty EOF member; whatever wrote the block (zlib at any level / strategy, the row-aware host encoder, k_row_deflate)
//   - the bit reader and the Huffman decode are wave-uniform (every lane holds the same state; the words come in through
//     scalar-uniform loads); the lanes write match copies and stored runs in parallel
//   - the block's whole output (ISIZE <= 65536) lives in LDS: the match window needs no memory ordering beyond the wave's
//     own in-order LDS traffic; two workgroups fit a CU's 160 KiB
//   - decode tables in LDS, built by the wave from the code lengths (ballots give every symbol its canonical rank): a
//     first-level table of LL_BITS / D_BITS bits, longer codes through the canonical count / symbol walk
//   - CRC-32 of the output with pg_deflate.hip's tables (68-byte chunks, slicing by four, shifted into place by the
//     chunk-count tables), checked together with ISIZE
//   - the finished bytes go out through the caller's segment map (PaySeg: payload offset -> device offset), so that a
//     block that straddles two contigs of a padded row buffer lands in both; bytes outside the map are dropped
// Every input byte is untrusted: reads stay inside the block's deflate bytes (the word loads are clamped to the buffer and
// the consumed bit count is checked before anything read is acted on: a stream cut short fails as INF_E_INPUT, whatever
// the bits behind it say), writes inside ISIZE; a malformed block sets its status word (INF_E_*) and its workgroup stops.
#include "pg_kernels.h"

namespace pg {

constexpr int INF_THREADS = 64;
constexpr uint32_t INF_OUT = 65536;
constexpr int LL_BITS = 10, D_BITS = 8;

__constant__ uint16_t INF_LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t INF_LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t INF_DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t INF_DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t INF_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the wave's bit reader over the block's deflate bytes: a 64-bit buffer refilled a word at a time
struct BitIn {
    const uint32_t *w;
    uint64_t nwords;  // words of the whole buffer (loads past it read 0)
    uint64_t wi;      // next word to load
    uint64_t buf;
    uint32_t nb;      // valid bits in buf
    uint64_t used, limit;  // bits consumed / bits the block has
    __device__ __forceinline__ void refill() {
        while (nb <= 32) {
            const uint64_t i = wi++;
            const uint32_t v = i < nwords ? w[i] : 0u;
            buf |= (uint64_t)uni(v) << nb;
            nb += 32;
        }
    }
    __device__ __forceinline__ uint32_t peek() const { return (uint32_t)buf; }
    __device__ __forceinline__ void drop(uint32_t n) {
        buf >>= n;
        nb -= n;
        used += n;
    }
    __device__ __forceinline__ uint32_t bits(uint32_t n) {  // n <= 16; the caller has refilled
        const uint32_t v = (uint32_t)buf & ((1u << n) - 1u);
        drop(n);
        return v;
    }
    __device__ __forceinline__ bool over() const { return used > limit; }
};

// one canonical Huffman code in LDS: count[len], symbols sorted by (len, symbol), the first-level table
struct Code {
    uint16_t *count;  // [16]
    uint16_t *sym;    // [n]
    uint16_t *lut;    // [1 << lbits]: (symbol << 4) | len, 0 = longer code (or none)
    int lbits;
};

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, int n) { return __builtin_bitreverse32(v) >> (32 - n); }

// code lengths len[0..n) (LDS) -> the tables of C.  0: complete; 1: incomplete; -1: over-subscribed
__device__ int build_code(const uint8_t *len, int n, Code C) {
    const int lane = threadIdx.x;
    if (lane < 16) C.count[lane] = 0;
    for (int i = lane; i < (1 << C.lbits); i += INF_THREADS) C.lut[i] = 0;
    // per length: how many symbols, and every symbol's rank among those of its length (ballots over chunks of 64)
    uint32_t cnt[16];
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int c0 = 0; c0 < n; c0 += INF_THREADS) {
        const int s = c0 + lane;
        const int L = s < n ? len[s] : 0;
        for (int l = 1; l < 16; ++l) {
            const uint64_t m = __ballot(s < n && L == l);
            cnt[l] += (uint32_t)__popcll(m);
        }
    }
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return -1;
    }
    // canonical codes (RFC 1951 3.2.2): the first code of length l = (first code of l-1 + count of l-1) << 1
    uint32_t first_code[16], first_idx[16];
    {
        uint32_t nc = 0, idx = 0;
        for (int l = 1; l < 16; ++l) {
            nc = l == 1 ? 0u : (nc + cnt[l - 1]) << 1;
            first_code[l] = nc;
            first_idx[l] = idx;
            idx += cnt[l];
        }
    }
    __syncthreads();
    if (lane < 16) C.count[lane] = (uint16_t)(lane ? cnt[lane] : 0);
    uint32_t seen[16];
    for (int l = 0; l < 16; ++l) seen[l] = 0;
    for (int c0 = 0; c0 < n; c0 += INF_THREADS) {
        const int s = c0 + lane;
        const int L = s < n ? len[s] : 0;
        uint32_t rank = 0, base_i = 0, base_c = 0;
        for (int l = 1; l < 16; ++l) {
            const uint64_t m = __ballot(s < n && L == l);
            if (L == l) {
                rank = seen[l] + (uint32_t)__popcll(m & below);
                base_i = first_idx[l];
                base_c = first_code[l];
            }
            seen[l] += (uint32_t)__popcll(m);
        }
        if (s < n && L) {
            C.sym[base_i + rank] = (uint16_t)s;
            if (L <= C.lbits) {
                const uint32_t r = rev_bits(base_c + rank, L);
                const uint16_t e = (uint16_t)((s << 4) | L);
                for (uint32_t j = r; j < (1u << C.lbits); j += (1u << L)) C.lut[j] = e;
            }
        }
    }
    __syncthreads();
    return left > 0 ? 1 : 0;
}

// one symbol (the caller has refilled: >= 32 bits in the buffer); -1: no such code
__device__ __forceinline__ int decode(BitIn &in, const Code &C) {
    const uint32_t v = in.peek();
    const uint32_t e = uni(C.lut[v & ((1u << C.lbits) - 1u)]);
    if (e & 15u) {
        in.drop(e & 15u);
        return (int)(e >> 4);
    }
    // longer than the table: the canonical walk (codes are MSB-first inside the LSB-first stream)
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((v >> (l - 1)) & 1u);
        const int count = (int)uni(C.count[l]);
        if (code - count < first) {
            in.drop((uint32_t)l);
            return (int)uni(C.sym[index + (code - first)]);
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

__global__ __launch_bounds__(INF_THREADS) void k_bgzf_inflate(const uint32_t *__restrict__ comp, uint64_t comp_words,
                                                             const InflBlock *__restrict__ blocks, const PaySeg *__restrict__ segs,
                                                             uint32_t nseg, uint8_t *__restrict__ dst,
                                                             const uint32_t *__restrict__ crc_tabs, uint32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t out[INF_OUT];
    __shared__ uint32_t S[1024];  // CRC-32, slicing by four (pg_deflate.hip's tables)
    __shared__ uint16_t ll_lut[1 << LL_BITS], d_lut[1 << D_BITS];
    __shared__ uint16_t ll_cnt[16], d_cnt[16], ll_sym[288], d_sym[32];
    __shared__ uint8_t lens[288 + 32];
    const int lane = threadIdx.x;
    const InflBlock B = blocks[blockIdx.x];
    for (int i = lane; i < 1024; i += INF_THREADS) S[i] = crc_tabs[i];
    const uint32_t isize = uni(B.isize);
    auto fail = [&](uint32_t code) {
        if (lane == 0) status[blockIdx.x] = code;
    };
    if (isize > INF_OUT || B.csize < B.hlen + 8u + 2u) {
        fail(INF_E_HEADER);
        return;
    }
    // the deflate bytes: [coff + hlen, coff + csize - 8)
    BitIn in;
    const uint64_t d0 = B.coff + B.hlen;
    in.w = comp;
    in.nwords = comp_words;
    in.wi = d0 >> 2;
    in.buf = 0;
    in.nb = 0;
    in.used = 0;
    in.limit = 8ull * (B.csize - B.hlen - 8u);
    in.refill();
    in.buf >>= 8 * (d0 & 3);
    in.nb -= 8 * (uint32_t)(d0 & 3);
    in.refill();
    Code LL{ll_cnt, ll_sym, ll_lut, LL_BITS}, D{d_cnt, d_sym, d_lut, D_BITS};
    uint32_t pos = 0;  // bytes written to out
    uint32_t last = 0;
    do {
        in.refill();
        last = in.bits(1);
        const uint32_t type = in.bits(2);
        if (in.over()) {  // (a block header behind the data: the stream was cut short)
            fail(INF_E_INPUT);
            return;
        }
        if (type == 0) {  // stored: to the byte boundary, LEN, NLEN, the bytes
            in.drop((8u - (uint32_t)(in.used & 7u)) & 7u);
            in.refill();
            const uint32_t L = in.bits(16), NL = in.bits(16);
            if ((L ^ 0xFFFFu) != NL) {
                fail(INF_E_STORED);
                return;
            }
            if (in.over() || in.used + 8ull * L > in.limit) {
                fail(INF_E_INPUT);
                return;
            }
            if (pos + L > isize) {
                fail(INF_E_OVERRUN);
                return;
            }
            // in.nb is a multiple of 8: the buffered bytes first, then straight from memory
            uint32_t i = 0;
            while (i < L && in.nb) {
                if (lane == 0) out[pos + i] = (uint8_t)in.buf;
                in.drop(8);
                ++i;
            }
            const uint64_t byte0 = d0 + in.used / 8;  // byte of the stream at the reader's position
            const uint8_t *cb = reinterpret_cast<const uint8_t *>(comp);
            for (uint32_t j = i + lane; j < L; j += INF_THREADS) out[pos + j] = cb[byte0 + (j - i)];
            const uint64_t bitpos = 8ull * (byte0 + (L - i));  // realign the reader behind the run
            in.used += 8ull * (L - i);
            in.wi = bitpos >> 5;
            in.buf = 0;
            in.nb = 0;
            in.refill();
            in.buf >>= bitpos & 31;
            in.nb -= (uint32_t)(bitpos & 31);
            pos += L;
            continue;
        }
        if (type == 3) {
            fail(INF_E_TYPE);
            return;
        }
        int nlen, ndist;
        if (type == 1) {  // fixed code (RFC 1951 3.2.6)
            for (int s = lane; s < 288 + 32; s += INF_THREADS)
                lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            nlen = 288;
            ndist = 32;  // (30 and 31 take part in the code, never in the data)
            __syncthreads();
        } else {  // dynamic: HLIT, HDIST, HCLEN, the code-length code, the two codes' lengths
            in.refill();
            nlen = (int)in.bits(5) + 257;
            ndist = (int)in.bits(5) + 1;
            const int ncl = (int)in.bits(4) + 4;
            if (in.over()) {
                fail(INF_E_INPUT);
                return;
            }
            if (nlen > 286 || ndist > 30) {
                fail(INF_E_CODES);
                return;
            }
            __shared__ uint8_t cl[19];
            if (lane < 19) cl[lane] = 0;
            __syncthreads();
            for (int i = 0; i < ncl; ++i) {
                in.refill();
                const uint32_t v = in.bits(3);
                if (lane == 0) cl[INF_CL_ORDER[i]] = (uint8_t)v;
            }
            __syncthreads();
            if (in.over()) {
                fail(INF_E_INPUT);
                return;
            }
            Code CL{ll_cnt, ll_sym, ll_lut, 7};
            if (build_code(cl, 19, CL) != 0) {  // the code-length code must be complete
                fail(INF_E_CODES);
                return;
            }
            int i = 0;
            while (i < nlen + ndist) {
                in.refill();
                const int s = decode(in, CL);
                if (s < 0 || in.over()) {
                    fail(s < 0 ? INF_E_SYMBOL : INF_E_INPUT);
                    return;
                }
                if (s < 16) {
                    if (lane == 0) lens[i] = (uint8_t)s;
                    ++i;
                    continue;
                }
                uint32_t rep, v = 0;
                if (s == 16) {
                    if (i == 0) {
                        fail(INF_E_CODES);
                        return;
                    }
                    __syncthreads();
                    v = uni(lens[i - 1]);
                    rep = 3 + in.bits(2);
                } else if (s == 17) {
                    rep = 3 + in.bits(3);
                } else {
                    rep = 11 + in.bits(7);
                }
                if (in.over()) {
                    fail(INF_E_INPUT);
                    return;
                }
                if (i + (int)rep > nlen + ndist) {
                    fail(INF_E_CODES);
                    return;
                }
                for (uint32_t j = lane; j < rep; j += INF_THREADS) lens[i + j] = (uint8_t)v;
                i += (int)rep;
            }
            if (in.over()) {
                fail(INF_E_INPUT);
                return;
            }
            __syncthreads();
            if (lens[256] == 0) {  // no end-of-block code
                fail(INF_E_CODES);
                return;
            }
        }
        // an incomplete code is only allowed when no code is longer than one bit: none, or a single one (puff / zlib)
        auto loose = [&](const Code &C) {
            uint32_t longer = 0;
            for (int l = 2; l < 16; ++l) longer += C.count[l];
            return longer != 0;
        };
        int r = build_code(lens, nlen, LL);
        if (r < 0 || (r > 0 && loose(LL))) {
            fail(INF_E_CODES);
            return;
        }
        r = build_code(lens + nlen, ndist, D);
        if (r < 0 || (r > 0 && loose(D))) {
            fail(INF_E_CODES);
            return;
        }
        // the block's symbols
        for (;;) {
            in.refill();
            const int s = decode(in, LL);
            if (s < 0) {
                fail(INF_E_SYMBOL);
                return;
            }
            if (s < 256) {
                if (in.over()) {
                    fail(INF_E_INPUT);
                    return;
                }
                if (pos >= isize) {
                    fail(INF_E_OVERRUN);
                    return;
                }
                if (lane == 0) out[pos] = (uint8_t)s;
                ++pos;
            } else if (s == 256) {
                break;
            } else {
                const int ls = s - 257;
                if (ls >= 29) {
                    fail(in.over() ? INF_E_INPUT : INF_E_SYMBOL);
                    return;
                }
                const uint32_t len = INF_LEN_BASE[ls] + in.bits(INF_LEN_EXTRA[ls]);
                in.refill();
                const int ds = decode(in, D);
                if (ds < 0 || ds >= 30) {
                    fail(in.over() ? INF_E_INPUT : INF_E_SYMBOL);
                    return;
                }
                const uint32_t dist = INF_DIST_BASE[ds] + in.bits(INF_DIST_EXTRA[ds]);
                if (in.over()) {
                    fail(INF_E_INPUT);
                    return;
                }
                if (dist > pos) {
                    fail(INF_E_DISTANCE);
                    return;
                }
                if (pos + len > isize) {
                    fail(INF_E_OVERRUN);
                    return;
                }
                // lane j writes out[pos + j] from out[pos - dist + (j mod dist)]: every source byte was written by an
                // earlier symbol, so a copy that overlaps its own output (dist < len: a periodic pattern) needs no steps
                const uint32_t src = pos - dist;
                if (dist >= len) {
                    for (uint32_t j = lane; j < len; j += INF_THREADS) out[pos + j] = out[src + j];
                } else if (dist == 1) {
                    const uint8_t b = out[src];
                    for (uint32_t j = lane; j < len; j += INF_THREADS) out[pos + j] = b;
                } else {
                    for (uint32_t j = lane; j < len; j += INF_THREADS) out[pos + j] = out[src + j % dist];
                }
                pos += len;
            }
        }
        if (in.over()) {
            fail(INF_E_INPUT);
            return;
        }
    } while (!last);
    __syncthreads();
    if (pos != isize) {
        fail(INF_E_ISIZE);
        return;
    }
    // the footer: CRC32, ISIZE (byte-aligned behind the deflate data; read bytewise, it need not be word-aligned)
    const uint8_t *cb = reinterpret_cast<const uint8_t *>(comp);
    const uint64_t ft = B.coff + B.csize - 8;
    const uint32_t f_crc = (uint32_t)cb[ft] | ((uint32_t)cb[ft + 1] << 8) | ((uint32_t)cb[ft + 2] << 16) | ((uint32_t)cb[ft + 3] << 24);
    const uint32_t f_isize = (uint32_t)cb[ft + 4] | ((uint32_t)cb[ft + 5] << 8) | ((uint32_t)cb[ft + 6] << 16) | ((uint32_t)cb[ft + 7] << 24);
    if (f_isize != isize) {
        fail(INF_E_ISIZE);
        return;
    }
    // CRC-32 of out[0, pos): 68-byte chunks, chunk t's register (chunk 0 from 0xFFFFFFFF, the others from 0) shifted by
    // the F - 1 - t chunks behind it (crc_tabs[1024 + 1024 j ..]: 2^j chunks of zero bytes) and XOR-ed; the tail bytewise
    const uint32_t F = pos / DF_CHUNK_BYTES;
    uint32_t acc = 0;
    for (uint32_t t = lane; t < F; t += INF_THREADS) {
        uint32_t c = t == 0 ? 0xFFFFFFFFu : 0u;
        const uint32_t *wv = reinterpret_cast<const uint32_t *>(out + t * DF_CHUNK_BYTES);
        for (uint32_t q = 0; q < DF_CHUNK_BYTES / 4; ++q) {
            const uint32_t x = c ^ wv[q];
            c = S[768 + (x & 255u)] ^ S[512 + ((x >> 8) & 255u)] ^ S[256 + ((x >> 16) & 255u)] ^ S[x >> 24];
        }
        const uint32_t e = F - 1 - t;
        for (uint32_t j = 0; j < DF_CRC_LEVELS; ++j)
            if ((e >> j) & 1u) {
                const uint32_t *T = crc_tabs + 1024 + 1024 * j;
                c = T[c & 255u] ^ T[256 + ((c >> 8) & 255u)] ^ T[512 + ((c >> 16) & 255u)] ^ T[768 + (c >> 24)];
            }
        acc ^= c;
    }
    for (int o = 32; o > 0; o >>= 1) acc ^= (uint32_t)__shfl_xor((int)acc, o);
    uint32_t crc = F ? acc : 0xFFFFFFFFu;
    for (uint32_t z = F * DF_CHUNK_BYTES; z < pos; ++z) crc = S[(crc ^ out[z]) & 255u] ^ (crc >> 8);
    crc ^= 0xFFFFFFFFu;
    if (uni(crc) != f_crc) {
        fail(INF_E_CRC);
        return;
    }
    // out -> the device buffer through the segment map: [lo, hi) of the payload, segment by segment
    const uint64_t lo = B.roff, hi = B.roff + pos;
    if (pos == 0 || nseg == 0 || hi <= segs[0].lstart || lo >= segs[nseg].lstart) return;
    uint32_t a = 0, b = nseg;  // the segment holding max(lo, segs[0].lstart)
    while (b - a > 1) {
        const uint32_t m = (a + b) >> 1;
        if (segs[m].lstart <= lo) a = m;
        else b = m;
    }
    for (uint32_t s = a; s < nseg && segs[s].lstart < hi; ++s) {
        const uint64_t x0 = max(lo, segs[s].lstart), x1 = min(hi, segs[s + 1].lstart);
        if (x0 >= x1) continue;
        uint8_t *d = dst + segs[s].doff + (x0 - segs[s].lstart);
        const uint8_t *o = out + (x0 - lo);
        const uint32_t n = (uint32_t)(x1 - x0);
        // bytes up to the destination's first dword, whole dwords, the tail
        const uint32_t head = min(n, (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u));
        if ((uint32_t)lane < head) d[lane] = o[lane];
        const uint32_t nw = (n - head) / 4;
        uint32_t *dw = reinterpret_cast<uint32_t *>(d + head);
        const uint8_t *ow = o + head;
        for (uint32_t i = lane; i < nw; i += INF_THREADS) {
            const uint8_t *p = ow + 4 * i;
            dw[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        const uint32_t done = head + 4 * nw;
        if ((uint32_t)lane < n - done) d[done + lane] = o[done + lane];
    }
}

hipError_t launch_bgzf_inflate(hipStream_t st, const uint32_t *comp, uint64_t comp_words, const InflBlock *blocks, uint32_t nblocks,
                               const PaySeg *segs, uint32_t nseg, uint8_t *dst, const uint32_t *crc_tabs, uint32_t *status) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(nblocks), dim3(INF_THREADS), 0, st, comp, comp_words, blocks, segs, nseg, dst, crc_tabs,
                       status);
    return hipGetLastError();
}

}  // namespace pg
