// pg_fastq.hip — FASTQ text to the ASCII of ONE contig ON THE GPU (gfx950): the sequence lines of all complete records joined by a
// single 'N', so that no k-mer window spans two reads and every kernel that streams a sequence set runs on reads without a
// descriptor per read.  pg_seqset_load_dev packs the ASCII (k_pack); nothing here packs.
//
// Definitions (tests/place_ref.py: fastq_model is the same in Python):
//   line      the bytes up to and including a line feed; line number = the line feeds before a byte.  Only the line count decides
//             what a line is: line 4 r is record r's header, 4 r + 1 its sequence, 4 r + 2 its separator, 4 r + 3 its qualities
//             (which may begin with '@' or '+').  Four-line FASTQ only: a sequence wrapped over several lines is not supported.
//   complete  L line feeds in the text make nreads = L / 4 complete records; consumed = the offset just past line feed 4 nreads.
//             The bytes from there on (a torn record) contribute nothing and are not checked.
//   output    the bytes of every complete record's sequence line without its line feed and without a '\r' right before it, one
//             'N' between two records — also around an empty sequence line.  len = those bytes + nreads - 1 (0 without a record).
//   malformed a complete record whose header line does not begin with '@' or whose separator line does not begin with '+' (an
//             empty line begins with neither).
//
// The text is cut into tiles of FASTQ_TILE bytes, one block of 256 threads per tile, 16 bytes per thread (one aligned load).  A
// byte's line number modulo 4 depends on all the text before it, so:
//   k_fastq_scan     per tile the line feeds, and for each of the four line numbers modulo 4 its first byte may have (its PHASE):
//                    the bytes it will put out, the malformed lines and the tile-local line number of the first of them.
//   k_fastq_offsets  one block: the scan of the tiles' line feeds gives every tile its phase, which picks one of its four counts;
//                    their scan gives the tile's first output byte.  Also L, and the first malformed line below line 4 nreads.
//   k_fastq_join     per tile again: every thread finds its bytes' line numbers and output positions from the tile's two bases
//                    and two scans inside the block, and stores its output bytes.  The line feed that ends the last complete
//                    record stores {len, consumed} instead of a separator.
// No tile waits for another, there is no global atomic, every write to HBM is a vector store.  The text buffer is readable, and
// zero, up to the next multiple of FASTQ_TILE past its last byte and 16 bytes beyond.
#include "pg_kernels.h"

namespace pg {

static_assert(FASTQ_TILE == 256 * 16, "a tile is 16 bytes for each of 256 threads");
static_assert(sizeof(FastqTileSum) == 64, "four 16-byte stores");

struct FastqBytes {
    uint32_t d[4];    // the 16 bytes
    uint32_t act;     // bit j: byte j lies inside the text
    uint32_t lf;      // bit j: byte j is a line feed
    uint32_t start;   // bit j: byte j is the first of a line
    uint32_t crlf;    // bit j: byte j is a '\r' right before a line feed
    __device__ __forceinline__ uint32_t at(uint32_t j) const { return (d[j >> 2] >> (8 * (j & 3))) & 0xFFu; }
};

__device__ __forceinline__ FastqBytes fastq_load16(const uint8_t *__restrict__ text, uint64_t nbytes, uint64_t a0) {
    FastqBytes b;
    const uint4 q = *reinterpret_cast<const uint4 *>(text + a0);
    b.d[0] = q.x; b.d[1] = q.y; b.d[2] = q.z; b.d[3] = q.w;
    const uint32_t prev = a0 ? text[a0 - 1] : 0x0Au;  // (offset 0 begins a line)
    const uint32_t next = text[a0 + 16];              // (inside the padded buffer; 0 past the text)
    b.act = b.lf = b.crlf = 0;
    uint32_t cr = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t c = b.at(j);
        if (a0 + j < nbytes) b.act |= 1u << j;
        if (c == 0x0Au) b.lf |= 1u << j;
        if (c == 0x0Du) cr |= 1u << j;
    }
    b.lf &= b.act;
    b.start = ((b.lf << 1) | (prev == 0x0Au ? 1u : 0u)) & b.act;
    b.crlf = cr & ((b.lf >> 1) | (next == 0x0Au && a0 + 16 < nbytes ? 1u << 15 : 0u)) & b.act;
    return b;
}

// the exclusive prefix of v over the block's 256 threads (wsum: 4 words of LDS, free to be written); total: the block's sum
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= (uint32_t)o) incl += up;
    }
    __syncthreads();  // (the words' readers of the scan before this one are through)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    return before + incl - v;
}

__global__ __launch_bounds__(256) void k_fastq_scan(const uint8_t *__restrict__ text, uint64_t nbytes, FastqTileSum *__restrict__ sums) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t red[4][8];
    __shared__ uint32_t firstbad[2][4];  // [header rule, separator rule][line class]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 8) firstbad[tid >> 2][tid & 3] = 0xFFFFFFFFu;
    const FastqBytes b = fastq_load16(text, nbytes, (uint64_t)blockIdx.x * FASTQ_TILE + 16ull * tid);
    uint32_t nlf;
    const uint32_t l0 = block_exclusive((uint32_t)__popc(b.lf), wsum, nlf);  // (its barriers order the marks above too)
    // per line class (tile-local line number & 3), 8 bits each: the bytes that go out if the class is the sequence line's, the
    // line feeds, the lines that do not begin with '@', and with '+'
    uint32_t cnt = 0, lfs = 0, noat = 0, noplus = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        if (!((b.act >> j) & 1u)) continue;
        const uint32_t line = l0 + (uint32_t)__popc(b.lf & ((1u << j) - 1u)), sh = 8 * (line & 3u);
        if ((b.lf >> j) & 1u)
            lfs += 1u << sh;
        else if (!((b.crlf >> j) & 1u))
            cnt += 1u << sh;
        if ((b.start >> j) & 1u) {
            const uint32_t c = b.at(j);
            if (c != 0x40u) {
                noat += 1u << sh;
                atomicMin(&firstbad[0][line & 3u], line);
            }
            if (c != 0x2Bu) {
                noplus += 1u << sh;
                atomicMin(&firstbad[1][line & 3u], line);
            }
        }
    }
    // the sums: every 8-bit field (at most 16 per thread) widened to 16 bits (at most 4096 per tile)
    uint32_t v[8] = {cnt & 0x00FF00FFu, (cnt >> 8) & 0x00FF00FFu, lfs & 0x00FF00FFu, (lfs >> 8) & 0x00FF00FFu,
                     noat & 0x00FF00FFu, (noat >> 8) & 0x00FF00FFu, noplus & 0x00FF00FFu, (noplus >> 8) & 0x00FF00FFu};
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[i] += (uint32_t)__shfl_xor((int)v[i], o);
        if (lane == 0) red[wave][i] = v[i];
    }
    __syncthreads();
    if (tid < 4) {
        const uint32_t ph = tid;  // the line number & 3 of the tile's first byte
        auto field = [&](uint32_t i, uint32_t cls) {  // class cls of counter i (0 cnt, 1 lfs, 2 noat, 3 noplus)
            const uint32_t w = 2 * i + (cls & 1u);
            return ((red[0][w] + red[1][w] + red[2][w] + red[3][w]) >> (16 * (cls >> 1))) & 0xFFFFu;
        };
        // a line of true number n has tile-local class (n - ph) & 3
        const uint32_t c0 = (0u - ph) & 3u, c1 = (1u - ph) & 3u, c2 = (2u - ph) & 3u, c3 = (3u - ph) & 3u;
        const uint32_t out = field(0, c1) + field(1, c3), nbad = field(2, c0) + field(3, c2);
        const uint32_t fb = min(firstbad[0][c0], firstbad[1][c2]);
        uint32_t *s = reinterpret_cast<uint32_t *>(sums + blockIdx.x);
        // (16 words: nlf, out[4], nbad[4], firstbad[4], pad[3] — thread ph stores its three, thread 0 the count of line feeds)
        s[1 + ph] = out;
        s[5 + ph] = nbad;
        s[9 + ph] = fb;
        if (ph == 0) s[0] = nlf;
    }
}

// one block of 256 threads over all tiles: thread i takes tiles [i * per, (i + 1) * per)
__global__ __launch_bounds__(256) void k_fastq_offsets(const FastqTileSum *__restrict__ sums, uint32_t ntiles, ulonglong2 *__restrict__ bases,
                                                       uint64_t *__restrict__ summary) {
    __shared__ uint64_t part[256];
    __shared__ uint64_t total_s;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + 255) / 256;
    const uint64_t t0 = min((uint64_t)tid * per, (uint64_t)ntiles), t1 = min(t0 + per, (uint64_t)ntiles);
    auto exclusive = [&](uint64_t v, uint64_t &total) {  // over the 256 threads, thread 0 adding them up (256 additions per scan)
        __syncthreads();
        part[tid] = v;
        __syncthreads();
        if (tid == 0) {
            uint64_t run = 0;
            for (uint32_t i = 0; i < 256; ++i) {
                const uint64_t x = part[i];
                part[i] = run;
                run += x;
            }
            total_s = run;
        }
        __syncthreads();
        total = total_s;
        return part[tid];
    };
    uint64_t mine = 0, L = 0, total_out = 0;
    for (uint64_t t = t0; t < t1; ++t) mine += sums[t].nlf;
    const uint64_t lf0 = exclusive(mine, L);
    const uint64_t limit = L & ~3ull;  // lines below it belong to complete records
    mine = 0;
    uint64_t lf = lf0;
    for (uint64_t t = t0; t < t1; ++t) {
        mine += sums[t].out[lf & 3u];
        lf += sums[t].nlf;
    }
    uint64_t ob = exclusive(mine, total_out);
    lf = lf0;
    uint64_t bad = ~0ull;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint32_t ph = (uint32_t)(lf & 3u);
        bases[t] = make_ulonglong2(ob, lf);
        if (bad == ~0ull && sums[t].nbad[ph] && lf + sums[t].firstbad[ph] < limit) bad = lf + sums[t].firstbad[ph];
        ob += sums[t].out[ph];
        lf += sums[t].nlf;
    }
    __syncthreads();
    part[tid] = bad;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t i = 0; i < 256; ++i) bad = min(bad, part[i]);
        summary[0] = L;
        summary[1] = bad;
        summary[2] = total_out;
    }
}

__global__ __launch_bounds__(256) void k_fastq_join(const uint8_t *__restrict__ text, uint64_t nbytes, const ulonglong2 *__restrict__ bases,
                                                    uint64_t limit, uint8_t *__restrict__ out, uint64_t out_cap, uint64_t *__restrict__ fin) {
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t a0 = (uint64_t)blockIdx.x * FASTQ_TILE + 16ull * tid;
    const ulonglong2 tb = bases[blockIdx.x];
    if (tb.y >= limit) return;  // (block-uniform: the whole tile lies behind the last complete record)
    const FastqBytes b = fastq_load16(text, nbytes, a0);
    uint32_t total;
    const uint64_t l0 = tb.y + block_exclusive((uint32_t)__popc(b.lf), wsum, total);
    uint32_t emit = 0;  // bit j: byte j puts a byte out (a sequence byte, or 'N' for the line feed that ends a record)
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        if (!((b.act >> j) & 1u)) continue;
        const uint64_t line = l0 + (uint32_t)__popc(b.lf & ((1u << j) - 1u));
        if (line >= limit) continue;
        const bool is_lf = (b.lf >> j) & 1u;
        if ((line & 3u) == 1u ? !is_lf && !((b.crlf >> j) & 1u) : (line & 3u) == 3u && is_lf) emit |= 1u << j;
    }
    uint64_t pos = tb.x + block_exclusive((uint32_t)__popc(emit), wsum, total);
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        if (!((emit >> j) & 1u)) continue;
        if ((b.lf >> j) & 1u) {
            const uint64_t line = l0 + (uint32_t)__popc(b.lf & ((1u << j) - 1u));
            if (line + 1 == limit) {  // the end of the last complete record: no separator behind it
                fin[0] = pos;
                fin[1] = a0 + j + 1;
            } else if (pos < out_cap) {
                out[pos] = 0x4Eu;
            }
        } else if (pos < out_cap) {
            out[pos] = (uint8_t)b.at(j);
        }
        ++pos;
    }
}

hipError_t launch_fastq_scan(hipStream_t st, const uint8_t *text, uint64_t nbytes, uint32_t ntiles, FastqTileSum *sums, ulonglong2 *bases,
                             uint64_t *summary) {
    if (ntiles == 0) return hipSuccess;
    if (!text || !sums || !bases || !summary || (uint64_t)ntiles * FASTQ_TILE < nbytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fastq_scan, dim3(ntiles), dim3(256), 0, st, text, nbytes, sums);
    hipLaunchKernelGGL(k_fastq_offsets, dim3(1), dim3(256), 0, st, sums, ntiles, bases, summary);
    return hipGetLastError();
}

hipError_t launch_fastq_join(hipStream_t st, const uint8_t *text, uint64_t nbytes, uint32_t ntiles, const ulonglong2 *bases, uint64_t limit,
                             uint8_t *out, uint64_t out_cap, uint64_t *fin) {
    if (ntiles == 0 || limit == 0) return hipSuccess;
    if (!text || !bases || !out || !fin || (uint64_t)ntiles * FASTQ_TILE < nbytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fastq_join, dim3(ntiles), dim3(256), 0, st, text, nbytes, bases, limit, out, out_cap, fin);
    return hipGetLastError();
}

}  // namespace pg
