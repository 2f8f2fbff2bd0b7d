// pg_api_sketch.hip — host side of the C-ABI: distinct-k-mer sketch, MinHash sketches and their distances.
#include "pg_host.h"

#include "pg_keytable_host.h"  // walk_kmers

// ---------------------------------------------------------------------------
// distinct-k-mer sketch (sizes a table before it is built)
// ---------------------------------------------------------------------------
struct pg_sketch {
    pg_ctx *ctx;
    int k;
    uint32_t *d_regs;
};

extern "C" int pg_sketch_create(pg_ctx *ctx, int k, pg_sketch **out) {
    PG_API_BEGIN
    if (!ctx || !out) return fail(PG_E_INVALID, "pg_sketch_create: NULL argument");
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "k=%d unsupported (1..32)", k);
    if (int r = use_device(ctx)) return r;
    uint32_t *regs = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&regs), sizeof(uint32_t) << SKETCH_BITS));
    hipError_t e = hipMemsetAsync(regs, 0, sizeof(uint32_t) << SKETCH_BITS, ctx->stream);
    if (e != hipSuccess) {
        hipFree(regs);
        return fail(PG_E_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    pg_sketch *sk = new pg_sketch{ctx, k, regs};
    ++ctx->refs;
    *out = sk;
    return PG_OK;
    PG_API_END
}

extern "C" int pg_sketch_destroy(pg_sketch *sk) {
    PG_API_BEGIN
    if (!sk) return PG_OK;
    hipSetDevice(sk->ctx->device);
    hipStreamSynchronize(sk->ctx->stream);
    hipFree(sk->d_regs);
    pg_ctx *c = sk->ctx;
    delete sk;
    ctx_release(c);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_sketch_add_seqset(pg_sketch *sk, const pg_seqset *sq) {
    PG_API_BEGIN
    if (!sk || !sq) return fail(PG_E_INVALID, "pg_sketch_add_seqset: NULL argument");
    if (sk->ctx != sq->ctx) return fail(PG_E_INVALID, "sketch and seqset belong to different contexts");
    if (int r = use_device(sk->ctx)) return r;
    // one launch over all contigs (a launch per contig was 76 ms per genome of 20 000 contigs)
    KmerWalk w;
    if (int r = walk_kmers(sq, sk->k, SKETCH_JOB, "pg_sketch_add_seqset", w)) return r;
    const std::vector<uint2> &jobs = w.jobs;
    if (jobs.empty()) return PG_OK;
    hipStream_t st = sk->ctx->stream;
    DevBuf<uint2> d_jobs;
    hipError_t e = d_jobs.alloc(jobs.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(uint2), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_sketch_set(st, sk->k, sq->d_desc, d_jobs.get(), (uint32_t)jobs.size(), sq->d_seqw, sq->d_nmw, sq->d_has_n, sk->d_regs);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the job list goes with the scope)
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_sketch_add_seqset: %s", hipGetErrorString(e));
    return PG_OK;
    PG_API_END
}

extern "C" int pg_sketch_registers(pg_sketch *sk, uint8_t *out) {
    PG_API_BEGIN
    if (!sk || !out) return fail(PG_E_INVALID, "pg_sketch_registers: NULL argument");
    if (int r = use_device(sk->ctx)) return r;
    std::vector<uint32_t> regs((size_t)1 << SKETCH_BITS);
    HIP_TRY(hipMemcpyAsync(regs.data(), sk->d_regs, regs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, sk->ctx->stream));
    HIP_TRY(hipStreamSynchronize(sk->ctx->stream));
    for (size_t i = 0; i < regs.size(); ++i) out[i] = (uint8_t)regs[i];
    return PG_OK;
    PG_API_END
}

// HyperLogLog (Flajolet et al. 2007) with the small-range correction; 64-bit hashes need no
// large-range one.  Standard error 1.04 / sqrt(2^16) = 0.4 %.
extern "C" int pg_sketch_estimate_registers(const uint8_t *regs, uint64_t *distinct) {
    PG_API_BEGIN
    if (!regs || !distinct) return fail(PG_E_INVALID, "pg_sketch_estimate_registers: NULL argument");
    const size_t n = (size_t)1 << SKETCH_BITS;
    const double m = (double)n;
    double sum = 0.0;
    size_t zeros = 0;
    for (size_t i = 0; i < n; ++i) {
        sum += std::ldexp(1.0, -(int)regs[i]);
        zeros += regs[i] == 0;
    }
    double est = (0.7213 / (1.0 + 1.079 / m)) * m * m / sum;
    if (est <= 2.5 * m && zeros) est = m * std::log(m / (double)zeros);
    *distinct = (uint64_t)(est + 0.5);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_sketch_estimate(pg_sketch *sk, uint64_t *distinct) {
    PG_API_BEGIN
    if (!sk || !distinct) return fail(PG_E_INVALID, "pg_sketch_estimate: NULL argument");
    std::vector<uint8_t> regs((size_t)1 << SKETCH_BITS);
    if (int r = pg_sketch_registers(sk, regs.data())) return r;
    return pg_sketch_estimate_registers(regs.data(), distinct);
    PG_API_END
}

extern "C" int pg_sketch_reset(pg_sketch *sk) {
    PG_API_BEGIN
    if (!sk) return fail(PG_E_INVALID, "pg_sketch_reset: NULL argument");
    if (int r = use_device(sk->ctx)) return r;
    HIP_TRY(hipMemsetAsync(sk->d_regs, 0, sizeof(uint32_t) << SKETCH_BITS, sk->ctx->stream));
    return PG_OK;
    PG_API_END
}

// ---------------------------------------------------------------------------
// MinHash sketch (genome_dist.tsv): candidates on the device (pg_minhash.hip), the bottom s on the host
// ---------------------------------------------------------------------------
struct pg_minhash {
    pg_ctx *ctx;
    int k;
    uint32_t s, seed;
    uint64_t tau, capacity;        // overrides (0: automatic)
    std::vector<uint64_t> hashes;  // the sketch so far: ascending, distinct, at most s
    uint64_t bases = 0;
    uint32_t passes = 0;
    uint64_t *d_cand = nullptr;  // candidate buffer, kept for the next sample
    uint64_t cand_cap = 0;
    unsigned long long *d_counts = nullptr;  // [0] candidates, [1] ACGT bases
};

extern "C" int pg_minhash_create(pg_ctx *ctx, int k, uint32_t s, uint32_t seed, uint64_t tau, uint64_t capacity, pg_minhash **out) {
    PG_API_BEGIN
    if (!ctx || !out) return fail(PG_E_INVALID, "pg_minhash_create: NULL argument");
    if (k != MINHASH_K) return fail(PG_E_INVALID, "k=%d unsupported (MinHash sketches: k = %d, mash's default)", k, MINHASH_K);
    if (s == 0) return fail(PG_E_INVALID, "pg_minhash_create: sketch size 0");
    if (int r = use_device(ctx)) return r;
    unsigned long long *counts = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&counts), 2 * sizeof(unsigned long long)));
    pg_minhash *mh = new pg_minhash{ctx, k, s, seed, tau, capacity};
    mh->d_counts = counts;
    ++ctx->refs;
    *out = mh;
    return PG_OK;
    PG_API_END
}

extern "C" int pg_minhash_destroy(pg_minhash *mh) {
    PG_API_BEGIN
    if (!mh) return PG_OK;
    hipSetDevice(mh->ctx->device);
    hipStreamSynchronize(mh->ctx->stream);
    if (mh->d_cand) hipFree(mh->d_cand);
    hipFree(mh->d_counts);
    pg_ctx *c = mh->ctx;
    delete mh;
    ctx_release(c);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_minhash_reset(pg_minhash *mh) {
    PG_API_BEGIN
    if (!mh) return fail(PG_E_INVALID, "pg_minhash_reset: NULL argument");
    mh->hashes.clear();
    mh->bases = 0;
    mh->passes = 0;
    return PG_OK;
    PG_API_END
}

// one pass: candidates h1 <= limit of all jobs -> cand (count may exceed cap: nothing past cap was written)
static int minhash_pass(pg_minhash *mh, const pg_seqset *sq, const uint2 *d_jobs, uint32_t njobs, uint64_t limit,
                        uint64_t cap, unsigned long long counts[2]) {
    hipStream_t st = mh->ctx->stream;
    if (cap > mh->cand_cap) {
        if (mh->d_cand) hipFree(mh->d_cand);
        mh->d_cand = nullptr;
        mh->cand_cap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&mh->d_cand), cap * sizeof(uint64_t)));
        mh->cand_cap = cap;
    }
    HIP_TRY(hipMemsetAsync(mh->d_counts, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(launch_minhash(st, sq->d_desc, d_jobs, njobs, sq->d_seqw, sq->d_nmw, sq->d_has_n, limit, mh->seed, mh->d_cand, cap,
                           mh->d_counts, mh->d_counts + 1));
    HIP_TRY(hipMemcpyAsync(counts, mh->d_counts, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ++mh->passes;
    return PG_OK;
}

extern "C" int pg_minhash_add_seqset(pg_minhash *mh, const pg_seqset *sq, uint64_t expected_distinct) {
    PG_API_BEGIN
    if (!mh || !sq) return fail(PG_E_INVALID, "pg_minhash_add_seqset: NULL argument");
    if (mh->ctx != sq->ctx) return fail(PG_E_INVALID, "MinHash sketch and seqset belong to different contexts");
    if (int r = use_device(mh->ctx)) return r;
    std::vector<uint2> jobs;
    uint64_t positions = 0;
    for (uint32_t c = 0; c < sq->n; ++c) {
        const SeqDesc &sd = sq->desc[c];
        if (sd.len >= (uint64_t)mh->k) positions += sd.len - mh->k + 1;
        for (uint64_t q = 0; q * MINHASH_JOB < sd.len; ++q) jobs.push_back(make_uint2(c, (uint32_t)q));
    }
    if (jobs.empty()) return PG_OK;
    // tau = 2^64 min(1, 4 s / n) as an inclusive limit (tau - 1); UINT64_MAX: every hash
    const uint64_t all = ~0ull;
    uint64_t limit;
    if (mh->tau) {
        limit = mh->tau - 1;
    } else {
        const double n = (double)(expected_distinct ? expected_distinct : std::max<uint64_t>(positions, 1));
        const double t = std::ldexp(4.0 * mh->s / n, 64);
        limit = t >= 18446744073709549568.0 ? all : std::max<uint64_t>((uint64_t)t, 1) - 1;
    }
    // (the candidates: positions x tau / 2^64 on average, repeats included — twice that, never more than the positions)
    uint64_t cap = mh->capacity;
    if (!cap) {
        const double frac = limit == all ? 1.0 : std::ldexp((double)limit + 1.0, -64);
        cap = std::min<uint64_t>(positions, (uint64_t)(2.0 * frac * (double)positions) + 65536);
    }
    cap = std::max<uint64_t>(cap, 1);
    hipStream_t st = mh->ctx->stream;
    DevBuf<uint2> d_jobs;
    std::vector<uint64_t> cand;
    unsigned long long counts[2] = {0, 0};
    hipError_t e = d_jobs.alloc(jobs.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(uint2), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_minhash_add_seqset: %s", hipGetErrorString(e));
    for (;;) {
        if (int rc = minhash_pass(mh, sq, d_jobs.get(), (uint32_t)jobs.size(), limit, cap, counts)) return rc;
        if (counts[0] > cap) {  // the buffer overflowed: the same threshold, a 4x buffer (at most one slot per position)
            cap = std::min<uint64_t>(std::max<uint64_t>(positions, 1), std::max<uint64_t>(cap * 4, counts[0]));
            continue;
        }
        cand.resize(counts[0]);
        if (!cand.empty()) {
            e = hipMemcpy(cand.data(), mh->d_cand, cand.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail(PG_E_HIP, "pg_minhash_add_seqset: %s", hipGetErrorString(e));
        }
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        // s distinct values below tau are the s smallest of the seqset; below 2^64 every hash is a candidate
        if (cand.size() >= mh->s || limit == all) break;
        limit = limit >= (all >> 2) ? all : limit * 4 + 3;  // tau -> 4 tau
    }
    if (cand.size() > mh->s) cand.resize(mh->s);
    std::vector<uint64_t> merged;
    merged.reserve(mh->hashes.size() + cand.size());
    std::set_union(mh->hashes.begin(), mh->hashes.end(), cand.begin(), cand.end(), std::back_inserter(merged));
    if (merged.size() > mh->s) merged.resize(mh->s);
    mh->hashes.swap(merged);
    mh->bases += counts[1];
    return PG_OK;
    PG_API_END
}

extern "C" int pg_minhash_result(pg_minhash *mh, uint64_t *hashes, uint32_t *count, uint64_t *bases, uint32_t *passes) {
    PG_API_BEGIN
    if (!mh || !count) return fail(PG_E_INVALID, "pg_minhash_result: NULL argument");
    if (hashes && !mh->hashes.empty()) std::memcpy(hashes, mh->hashes.data(), mh->hashes.size() * sizeof(uint64_t));
    *count = (uint32_t)mh->hashes.size();
    if (bases) *bases = mh->bases;
    if (passes) *passes = mh->passes;
    return PG_OK;
    PG_API_END
}

// P[Binomial(n, r) >= c] summed in log space from the tail's largest term outwards (lf: log i!, i = 0..n).  The same
// operations in the same order as tests/minhash_ref.py, so that the written file can be predicted byte for byte.
static double minhash_pvalue(uint32_t c, uint32_t n, uint64_t la, uint64_t lb, int k, const std::vector<double> &lf) {
    if (c == 0 || n == 0 || la == 0 || lb == 0) return 1.0;
    const double space = std::ldexp(1.0, 2 * k);
    const double px = 1.0 / (1.0 + space / (double)la);
    const double py = 1.0 / (1.0 + space / (double)lb);
    const double r = px * py / (px + py - px * py);
    if (r >= 1.0) return 1.0;
    const double lr = std::log(r), l1r = std::log1p(-r), step = lr - l1r;
    auto lterm = [&](uint32_t i) { return lf[n] - lf[i] - lf[n - i] + (double)i * lr + (double)(n - i) * l1r; };
    double acc = 1.0, rel = 0.0, p;
    if ((double)c > (double)n * r) {  // the upper tail's terms fall from i = c on
        for (uint32_t i = c; i < n;) {
            rel += std::log((double)(n - i) / ((double)i + 1.0)) + step;
            const double t = std::exp(rel);
            acc += t;
            ++i;
            if (t < 1e-17 * acc) break;
        }
        p = std::exp(lterm(c)) * acc;
    } else {  // 1 - P[X <= c - 1]: those terms fall from i = c - 1 down
        for (uint32_t i = c - 1; i > 0;) {
            rel += std::log((double)i / ((double)(n - i) + 1.0)) - step;
            const double t = std::exp(rel);
            acc += t;
            --i;
            if (t < 1e-17 * acc) break;
        }
        p = 1.0 - std::exp(lterm(c - 1)) * acc;
    }
    return std::min(1.0, std::max(0.0, p));
}

extern "C" int pg_minhash_distances(const uint64_t *hashes, const uint64_t *offsets, uint32_t n, uint32_t s, int k,
                                    const uint64_t *bases, double *dist, double *pvalue, uint32_t *common, uint32_t *denom) {
    PG_API_BEGIN
    if ((!hashes && n && offsets && offsets[n]) || !offsets || !dist || !common || !denom)
        return fail(PG_E_INVALID, "pg_minhash_distances: NULL argument");
    if (s == 0 || k < 1 || k > 32) return fail(PG_E_INVALID, "pg_minhash_distances: s=%u k=%d", s, k);
    for (uint32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(PG_E_INVALID, "pg_minhash_distances: offsets not ascending");
    std::vector<double> lf(s + 1, 0.0);
    for (uint32_t i = 2; i <= s; ++i) lf[i] = lf[i - 1] + std::log((double)i);
    // the pairs (i, j) of row i start at i (2n - i - 1) / 2; rows go to threads round-robin (row i has n - 1 - i pairs)
    const uint32_t nthreads = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({8, std::thread::hardware_concurrency(), n / 16 + 1}));
    auto rows = [&](uint32_t t0) {
        for (uint32_t i = t0; i < n; i += nthreads) {
            uint64_t out = (uint64_t)i * (2ull * n - i - 1) / 2;
            const uint64_t *a = hashes + offsets[i];
            const uint64_t na = offsets[i + 1] - offsets[i];
            for (uint32_t j = i + 1; j < n; ++j, ++out) {
                const uint64_t *b = hashes + offsets[j];
                const uint64_t nb = offsets[j + 1] - offsets[j];
                uint64_t x = 0, y = 0, c = 0, d = 0;
                while (d < s && x < na && y < nb) {
                    if (a[x] < b[y]) {
                        ++x;
                    } else if (a[x] > b[y]) {
                        ++y;
                    } else {
                        ++x, ++y, ++c;
                    }
                    ++d;
                }
                if (d < s) {
                    d = std::min<uint64_t>(s, d + (na - x));
                    d = std::min<uint64_t>(s, d + (nb - y));
                }
                double D;
                if (c == 0) {
                    D = 1.0;
                } else if (c == d) {
                    D = 0.0;
                } else {
                    const double J = (double)c / (double)d;
                    D = std::min(1.0, -std::log(2.0 * J / (1.0 + J)) / k);
                }
                dist[out] = D;
                common[out] = (uint32_t)c;
                denom[out] = (uint32_t)d;
                if (pvalue) pvalue[out] = bases ? minhash_pvalue((uint32_t)c, (uint32_t)d, bases[i], bases[j], k, lf) : 1.0;
            }
        }
    };
    if (nthreads == 1) {
        rows(0);
    } else {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < nthreads; ++t) th.emplace_back(rows, t);
        for (auto &t : th) t.join();
    }
    return PG_OK;
    PG_API_END
}
