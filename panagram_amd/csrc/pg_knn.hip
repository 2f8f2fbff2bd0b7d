// pg_knn.hip — exact k nearest neighbours among the rows of a dense float32 matrix ON THE GPU (gfx950), under squared
// Euclidean distance: the neighbour graph behind the viewer's UMAP files (panagram/index.py:1131-1137: run_umap hands the
// bins x genomes pair-count matrix of a chromosome, or of the whole genome, to umap.UMAP, whose first step this is).
//
// X is n x D, row-major.  The rows are cut into SEGMENTS (the chromosomes of an anchor): a row searches only the rows of its
// own segment, itself included.  The host cuts every segment into TILES of up to blockDim.x query rows; a block takes one
// tile, a thread one query row, and the block streams the segment's rows — the candidates — through LDS in ascending order.
//
// EXACT, bit for bit: d2(i, j) is the float32 sum over g = 0 .. D-1, in that order, of (X[i][g] - X[j][g])^2, every subtract,
// multiply and add rounded to float32 — plain operators under `fp contract(off)`, see knn_step: no fused multiply-add, no
// reassociation (tests/knn_ref.py restates it in numpy).  Columns past D are padded with zeros on both sides, which add
// (0 - 0)^2 = +0 and leave the sum as it is.  The K entries of a row are sorted by (d2, row number): a thread keeps them as a
// sorted list in registers, and because candidates arrive in ascending row order a new one goes behind every entry of equal
// distance.  A slot is empty while its row number is negative; segments shorter than K leave (-1, +inf).
//
//   k_knn_rows<KT, DT>       D <= DT <= 128: the query row lives in DT registers.  A candidate tile is CT x DT floats in LDS;
//                            a thread takes 4 candidates at a time (4 independent sums), reading their values as 16-byte LDS
//                            broadcasts — every lane of a wave reads the same address — and spends 3 vector instructions per
//                            value.
//   k_knn_rows_wide<KT>      D <= 4096: columns go through LDS in chunks of 32, for 16 candidates at a time whose 16 sums
//                            stay in registers across the chunks (so each sum still sees g in order); a thread reloads
//                            its query row's chunk from global memory (L2) per chunk.
// KT = list slots (4, 8, 16, 32 >= K).  No atomics; a row's result is written once.
#include "pg_kernels.h"

#pragma clang fp contract(off)

namespace pg {

constexpr uint32_t KNN_WIDE_DC = 32;  // columns per chunk of the wide kernel
constexpr uint32_t KNN_WIDE_CT = 16;  // candidates per tile of the wide kernel

__host__ __device__ constexpr uint32_t knn_ct(uint32_t DT) { return DT <= 8 ? 256 : DT <= 32 ? 128 : 64; }  // candidates per LDS tile
// waves per SIMD asked of the compiler: the query row, the list and about 48 registers of working set — without the bound the
// scheduler hoists a whole candidate group's LDS reads and takes all 256 registers (and scratch) from 64 columns on
__host__ __device__ constexpr uint32_t knn_waves(uint32_t KT, uint32_t DT) {
    const uint32_t regs = (DT + 2 * KT + 48 + 7) & ~7u, w = 512 / regs;
    return w > 8 ? 8 : w < 1 ? 1 : w;
}

// acc + (a - b)^2, three roundings.  Plain operators under this file's `fp contract(off)`: hipcc contracts by default, and
// the __fmul_rn / __fadd_rn of the HIP headers are inline functions compiled under THAT default — their product and sum fuse
// into v_fmac_f32 all the same (seen in the ISA), one rounding short of the contract.
__device__ __forceinline__ float knn_step(float acc, float a, float b) {
    const float d = a - b;
    const float p = d * d;
    return acc + p;
}

// no memory access moves across this point, and the sums named are complete at it (no instruction is emitted): without it
// the compiler hoists every LDS read of an unrolled candidate group to the group's top and sinks the arithmetic to its end,
// takes all 256 registers for the values in between and spills the rest to scratch
__device__ __forceinline__ void knn_fence(float &a, float &b, float &c, float &d) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : : "memory");
}
__device__ __forceinline__ void knn_fence(float &a, float &b) { asm volatile("" : "+v"(a), "+v"(b) : : "memory"); }

template <uint32_t KT>
struct KnnList {
    float d[KT];
    int32_t i[KT];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (uint32_t j = 0; j < KT; ++j) {
            d[j] = __builtin_inff();
            i[j] = -1;
        }
    }
    // does slot j sort behind a new candidate of distance x (whose row number exceeds every held one)?
    __device__ __forceinline__ bool behind(uint32_t j, float x) const { return i[j] < 0 || d[j] > x; }
    __device__ __forceinline__ void push(float x, int32_t row) {
        if (!behind(KT - 1, x)) return;
#pragma unroll
        for (uint32_t j = KT - 1; j > 0; --j) {
            const bool shift = behind(j - 1, x), here = behind(j, x);
            d[j] = shift ? d[j - 1] : here ? x : d[j];
            i[j] = shift ? i[j - 1] : here ? row : i[j];
        }
        if (behind(0, x)) {
            d[0] = x;
            i[0] = row;
        }
    }
    __device__ __forceinline__ void store(uint32_t K, int32_t *__restrict__ io, float *__restrict__ dd) const {
#pragma unroll
        for (uint32_t j = 0; j < KT; ++j)
            if (j < K) {
                io[j] = i[j];
                dd[j] = d[j];
            }
    }
};

// rows [c0, c0 + nr) x columns [g0, g0 + W) of X -> tile[r * W + g], zero outside the matrix's D columns and for the rows
// from nc on (nr = nc rounded up to the candidates a thread takes at a time)
template <uint32_t W>
__device__ __forceinline__ void knn_fill(float *__restrict__ tile, const float *__restrict__ X, uint32_t D, uint32_t c0,
                                         uint32_t nc, uint32_t nr, uint32_t g0) {
    if ((D & 3u) == 0) {  // rows start on 16 bytes
        for (uint32_t e = threadIdx.x; e < nr * (W / 4); e += blockDim.x) {
            const uint32_t r = e / (W / 4), g = g0 + 4 * (e % (W / 4));
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < nc && g < D) v = *reinterpret_cast<const float4 *>(X + (size_t)(c0 + r) * D + g);
            *reinterpret_cast<float4 *>(tile + 4 * e) = v;
        }
    } else {
        for (uint32_t e = threadIdx.x; e < nr * W; e += blockDim.x) {
            const uint32_t r = e / W, g = g0 + e % W;
            tile[e] = r < nc && g < D ? X[(size_t)(c0 + r) * D + g] : 0.f;
        }
    }
}

// a tile of query rows: rows [row0, row0 + nrows) search rows [lo, hi)
struct KnnTile {
    uint32_t row0, nrows, lo, hi;
};

template <uint32_t KT, uint32_t DT>
__global__ __launch_bounds__(256, knn_waves(KT, DT)) void k_knn_rows(const float *__restrict__ X, uint32_t D, uint32_t K,
                                                  const KnnTile *__restrict__ tiles, int32_t *__restrict__ idx_out,
                                                  float *__restrict__ d2_out) {
    constexpr uint32_t CT = knn_ct(DT);
    __shared__ __align__(16) float cand[CT * DT];
    const KnnTile t = tiles[blockIdx.x];
    const bool act = threadIdx.x < t.nrows;
    const uint32_t row = t.row0 + threadIdx.x;
    float q[DT];
#pragma unroll
    for (uint32_t g = 0; g < DT; ++g) q[g] = act && g < D ? X[(size_t)row * D + g] : 0.f;
    KnnList<KT> list;
    list.init();
    for (uint32_t c0 = t.lo; c0 < t.hi; c0 += CT) {
        const uint32_t nc = min(CT, t.hi - c0);
        __syncthreads();  // (every wave has read the tile before)
        knn_fill<DT>(cand, X, D, c0, nc, (nc + 3) & ~3u, 0);
        __syncthreads();
        for (uint32_t c = 0; c < nc; c += 4) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (uint32_t g = 0; g < DT; g += 4) {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const float4 v = *reinterpret_cast<const float4 *>(cand + (c + j) * DT + g);
                    acc[j] = knn_step(acc[j], q[g], v.x);
                    acc[j] = knn_step(acc[j], q[g + 1], v.y);
                    acc[j] = knn_step(acc[j], q[g + 2], v.z);
                    acc[j] = knn_step(acc[j], q[g + 3], v.w);
                }
                if (g % 8 == 4) knn_fence(acc[0], acc[1], acc[2], acc[3]);
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (c + j < nc) list.push(acc[j], (int32_t)(c0 + c + j));
        }
    }
    if (act) list.store(K, idx_out + (size_t)row * K, d2_out + (size_t)row * K);
}

template <uint32_t KT>
__global__ __launch_bounds__(256, knn_waves(KT, KNN_WIDE_DC + KNN_WIDE_CT)) void k_knn_rows_wide(const float *__restrict__ X, uint32_t D, uint32_t K,
                                                       const KnnTile *__restrict__ tiles, int32_t *__restrict__ idx_out,
                                                       float *__restrict__ d2_out) {
    constexpr uint32_t CT = KNN_WIDE_CT, DC = KNN_WIDE_DC;
    __shared__ __align__(16) float cand[CT * DC];
    const KnnTile t = tiles[blockIdx.x];
    const bool act = threadIdx.x < t.nrows;
    const uint32_t row = t.row0 + threadIdx.x;
    KnnList<KT> list;
    list.init();
    for (uint32_t c0 = t.lo; c0 < t.hi; c0 += CT) {
        const uint32_t nc = min(CT, t.hi - c0);
        float acc[CT];
#pragma unroll
        for (uint32_t r = 0; r < CT; ++r) acc[r] = 0.f;
        for (uint32_t g0 = 0; g0 < D; g0 += DC) {
            float q[DC];
#pragma unroll
            for (uint32_t g = 0; g < DC; ++g) q[g] = act && g0 + g < D ? X[(size_t)row * D + g0 + g] : 0.f;
            __syncthreads();
            knn_fill<DC>(cand, X, D, c0, nc, CT, g0);
            __syncthreads();
#pragma unroll
            for (uint32_t r = 0; r < CT; ++r) {
#pragma unroll
                for (uint32_t g = 0; g < DC; g += 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(cand + r * DC + g);
                    acc[r] = knn_step(acc[r], q[g], v.x);
                    acc[r] = knn_step(acc[r], q[g + 1], v.y);
                    acc[r] = knn_step(acc[r], q[g + 2], v.z);
                    acc[r] = knn_step(acc[r], q[g + 3], v.w);
                }
                if (r % 2 == 1) knn_fence(acc[r - 1], acc[r]);
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < CT; ++r)
            if (r < nc) list.push(acc[r], (int32_t)(c0 + r));
    }
    if (act) list.store(K, idx_out + (size_t)row * K, d2_out + (size_t)row * K);
}

template <uint32_t KT>
static void knn_launch_kt(hipStream_t st, const float *X, uint32_t D, uint32_t K, const KnnTile *tiles, uint32_t ntiles,
                          uint32_t threads, int32_t *idx, float *d2) {
    const dim3 grid(ntiles), block(threads);
    if (D <= 8)
        hipLaunchKernelGGL((k_knn_rows<KT, 8>), grid, block, 0, st, X, D, K, tiles, idx, d2);
    else if (D <= 32)
        hipLaunchKernelGGL((k_knn_rows<KT, 32>), grid, block, 0, st, X, D, K, tiles, idx, d2);
    else if (D <= 64)
        hipLaunchKernelGGL((k_knn_rows<KT, 64>), grid, block, 0, st, X, D, K, tiles, idx, d2);
    else if (D <= KNN_REG_COLS)
        hipLaunchKernelGGL((k_knn_rows<KT, KNN_REG_COLS>), grid, block, 0, st, X, D, K, tiles, idx, d2);
    else
        hipLaunchKernelGGL((k_knn_rows_wide<KT>), grid, block, 0, st, X, D, K, tiles, idx, d2);
}

hipError_t launch_knn_rows(hipStream_t st, const float *X, uint32_t D, uint32_t K, const uint32_t *tiles, uint32_t ntiles,
                           uint32_t threads, int32_t *idx, float *d2) {
    static_assert(sizeof(KnnTile) == 16, "a tile is four 32-bit words: row0, nrows, lo, hi");
    if (ntiles == 0) return hipSuccess;
    if (K < 1 || K > KNN_MAX_K || D < 1 || D > KNN_MAX_COLS || (threads != 64 && threads != 256)) return hipErrorInvalidValue;
    const KnnTile *t = reinterpret_cast<const KnnTile *>(tiles);
    if (K <= 4)
        knn_launch_kt<4>(st, X, D, K, t, ntiles, threads, idx, d2);
    else if (K <= 8)
        knn_launch_kt<8>(st, X, D, K, t, ntiles, threads, idx, d2);
    else if (K <= 16)
        knn_launch_kt<16>(st, X, D, K, t, ntiles, threads, idx, d2);
    else
        knn_launch_kt<32>(st, X, D, K, t, ntiles, threads, idx, d2);
    return hipGetLastError();
}

}  // namespace pg
