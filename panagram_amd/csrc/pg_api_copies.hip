// pg_api_copies.hip — host side of the C-ABI: the count table of target k-mers, a genome counted into one of its planes, and the
// depth histograms of sequences along the planes (pg_copies.hip, pg_copies_host.h); one plane joined with finished bitmap rows
// (pg_place.hip); allele ranges inserted into the table and three planes reduced along them (pg_genotype.hip, pg_genotype_host.h).
#include "pg_host.h"

#include "pg_copies_host.h"
#include "pg_keytable_host.h"

static constexpr uint64_t COPIES_MAX_KEYS = COPIES_MAX_SLOTS / 2;   // (table_slots: the power of two at or above 2 * capacity)
static constexpr uint64_t COPIES_MAX_POSITIONS = 0xFFFFFFFFull;     // of one genome: a counter is 32 bits
static constexpr size_t COPIES_PARTIAL_BYTES = (size_t)256 << 20;   // partials of one profile launch (a longer chunk list goes in pieces)

float *pg::place_ms() {
    static thread_local float ms[2] = {0, 0};
    return ms;
}

struct pg_copytable {
    pg_ctx *ctx;
    int k;
    uint64_t capacity, nslots;
    uint32_t max_probe, nplanes;
    unsigned long long *d_keys = nullptr;
    uint32_t *d_planes = nullptr;  // [nplanes][nslots]
    bool overflowed = false;       // an insert gave up: the table holds a part of the targets and answers nothing any more
};

namespace {

thread_local float g_copies_ms[3] = {0, 0, 0};  // k_copy_insert, k_copy_count, k_copy_profile of this thread's last calls
thread_local float g_genotype_ms[2] = {0, 0};   // k_allele_insert, k_allele_support of this thread's last calls

void copytable_free(pg_copytable *ct) {
    hipSetDevice(ct->ctx->device);
    hipStreamSynchronize(ct->ctx->stream);
    if (ct->d_planes) hipFree(ct->d_planes);
    if (ct->d_keys) hipFree(ct->d_keys);
    pg_ctx *c = ct->ctx;
    delete ct;
    ctx_release(c);
}

int copytable_create(pg_ctx *ctx, int k, uint64_t capacity, uint32_t nplanes, pg_copytable **out) {
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "pg_copytable_create: k=%d unsupported (1..32)", k);
    if (capacity < 1 || capacity > COPIES_MAX_KEYS)
        return fail(PG_E_INVALID, "pg_copytable_create: capacity of %llu keys (1 to 2^30)", (unsigned long long)capacity);
    if (nplanes < 1) return fail(PG_E_INVALID, "pg_copytable_create: at least one plane");
    if (int r = use_device(ctx)) return r;
    std::unique_ptr<pg_copytable> ct(new pg_copytable);
    ct->ctx = ctx;
    ct->k = k;
    ct->capacity = capacity;
    ct->nslots = table_slots(capacity);
    ct->max_probe = table_max_probe(ct->nslots);
    ct->nplanes = nplanes;
    DevBuf<unsigned long long> keys;
    DevBuf<uint32_t> planes;
    hipError_t e = keys.alloc(ct->nslots);
    if (e == hipSuccess) e = planes.alloc((size_t)ct->nslots * nplanes);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PG_E_CAPACITY : PG_E_HIP, "pg_copytable_create: %llu slots, %u planes: %s",
                    (unsigned long long)ct->nslots, nplanes, hipGetErrorString(e));
    e = hipMemsetAsync(keys.get(), 0xFF, ct->nslots * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(planes.get(), 0, (size_t)ct->nslots * nplanes * 4, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_copytable_create: %s", hipGetErrorString(e));
    std::swap(ct->d_keys, keys.p);
    std::swap(ct->d_planes, planes.p);
    ++ctx->refs;
    *out = ct.release();
    return PG_OK;
}

int copytable_insert(pg_copytable *ct, const pg_seqset *sq, uint64_t *distinct) {
    if (ct->ctx != sq->ctx) return fail(PG_E_INVALID, "pg_copytable_insert_seqset: table and seqset belong to different contexts");
    if (ct->overflowed) return fail(PG_E_CAPACITY, "pg_copytable_insert_seqset: the table overflowed before");
    KmerWalk w;
    if (int r = walk_kmers(sq, ct->k, COPIES_JOB, "pg_copytable_insert_seqset", w)) return r;
    if (int r = use_device(ct->ctx)) return r;
    *distinct = 0;
    g_copies_ms[0] = 0;
    if (w.jobs.empty()) return PG_OK;
    hipStream_t st = ct->ctx->stream;
    unsigned long long ctr[2] = {0, 0};
    const hipError_t e = counted_launch(st, w.jobs, ctr, 2, &g_copies_ms[0], [&](const uint2 *jobs, uint32_t njobs, unsigned long long *d_ctr) {
        return launch_copy_insert(st, ct->k, sq->d_desc, jobs, njobs, sq->d_seqw, sq->d_nmw, sq->d_has_n, ct->d_keys, ct->nslots,
                                  ct->max_probe, d_ctr);
    });
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_copytable_insert_seqset: %s", hipGetErrorString(e));
    *distinct = ctr[1];
    if (ctr[0]) {
        ct->overflowed = true;
        return fail(PG_E_CAPACITY, "pg_copytable_insert_seqset: %llu slots (created for %llu keys) do not hold the targets' k-mers",
                    (unsigned long long)ct->nslots, (unsigned long long)ct->capacity);
    }
    return PG_OK;
}

int copytable_count(pg_copytable *ct, uint32_t plane, const pg_seqset *sq, uint64_t *hits) {
    if (plane >= ct->nplanes) return fail(PG_E_INVALID, "pg_copytable_count_seqset: plane %u of %u", plane, ct->nplanes);
    if (ct->ctx != sq->ctx) return fail(PG_E_INVALID, "pg_copytable_count_seqset: table and seqset belong to different contexts");
    if (ct->overflowed) return fail(PG_E_CAPACITY, "pg_copytable_count_seqset: the table overflowed");
    KmerWalk w;
    if (int r = walk_kmers(sq, ct->k, COPIES_JOB, "pg_copytable_count_seqset", w)) return r;
    if (w.nkmers > COPIES_MAX_POSITIONS)
        return fail(PG_E_INVALID, "pg_copytable_count_seqset: %llu k-mer positions in one genome (the counters hold 2^32 - 1)",
                    (unsigned long long)w.nkmers);
    if (int r = use_device(ct->ctx)) return r;
    *hits = 0;
    g_copies_ms[1] = 0;
    if (w.jobs.empty()) return PG_OK;
    hipStream_t st = ct->ctx->stream;
    unsigned long long n = 0;
    const hipError_t e = counted_launch(st, w.jobs, &n, 1, &g_copies_ms[1], [&](const uint2 *jobs, uint32_t njobs, unsigned long long *d_n) {
        return launch_copy_count(st, ct->k, sq->d_desc, jobs, njobs, sq->d_seqw, sq->d_nmw, sq->d_has_n, ct->d_keys, ct->nslots,
                                 ct->max_probe, ct->d_planes + (size_t)plane * ct->nslots, d_n);
    });
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_copytable_count_seqset: %s", hipGetErrorString(e));
    *hits = n;
    return PG_OK;
}

int copytable_profile(pg_copytable *ct, const pg_seqset *sq, uint32_t plane0, uint32_t nplanes, uint64_t *hist_out, uint64_t *valid_out,
                      uint16_t *depth_out) {
    if (nplanes < 1 || plane0 >= ct->nplanes || nplanes > ct->nplanes - plane0)
        return fail(PG_E_INVALID, "pg_copytable_profile: planes [%u, %u + %u) of %u", plane0, plane0, nplanes, ct->nplanes);
    if (ct->ctx != sq->ctx) return fail(PG_E_INVALID, "pg_copytable_profile: table and seqset belong to different contexts");
    if (ct->overflowed) return fail(PG_E_CAPACITY, "pg_copytable_profile: the table overflowed");
    KmerWalk w;
    if (int r = walk_kmers(sq, ct->k, COPIES_CHUNK, "pg_copytable_profile", w)) return r;
    if (int r = use_device(ct->ctx)) return r;
    const size_t row = (size_t)nplanes * COPIES_BINS;
    std::fill(hist_out, hist_out + (size_t)sq->n * row, 0ull);
    std::fill(valid_out, valid_out + sq->n, 0ull);
    g_copies_ms[2] = 0;
    if (w.jobs.empty()) return PG_OK;
    const size_t nchunks = w.jobs.size();
    const size_t per = std::max<size_t>(1, COPIES_PARTIAL_BYTES / (row * 4));  // chunks per launch
    hipStream_t st = ct->ctx->stream;
    DevBuf<uint2> d_chunks;
    DevBuf<uint64_t> d_koff;
    DevBuf<uint32_t> d_part;  // [per][nplanes][64] partials, then [per] valid counts
    DevBuf<uint16_t> d_depth;
    std::vector<uint32_t> partial(nchunks * row), valid_partial(nchunks);
    hipError_t e = d_chunks.upload(w.jobs, st);
    if (e == hipSuccess) e = d_koff.upload(w.koff, st);
    if (e == hipSuccess) e = d_part.alloc(std::min(per, nchunks) * (row + 1));
    if (e == hipSuccess && depth_out) e = d_depth.alloc((size_t)nplanes * w.nkmers);
    if (e == hipErrorOutOfMemory) return fail(PG_E_CAPACITY, "pg_copytable_profile: no memory for %zu chunks of %u planes", nchunks, nplanes);
    float total_ms = 0;
    for (size_t c0 = 0; c0 < nchunks && e == hipSuccess; c0 += per) {
        const size_t n = std::min(per, nchunks - c0);
        float ms = 0;
        LaunchTimer tm(&ms);
        e = tm.start(st);
        if (e == hipSuccess)
            e = launch_copy_profile(st, ct->k, sq->d_desc, d_chunks.get() + c0, (uint32_t)n, d_koff.get(), sq->d_seqw, sq->d_nmw, sq->d_has_n,
                                    ct->d_keys, ct->nslots, ct->max_probe, ct->d_planes + (size_t)plane0 * ct->nslots, nplanes, d_part.get(),
                                    d_part.get() + n * row, d_depth.get(), w.nkmers);
        if (e == hipSuccess) e = tm.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(partial.data() + c0 * row, d_part.get(), n * row * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(valid_partial.data() + c0, d_part.get() + n * row, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) tm.read();
        total_ms += ms;
    }
    if (e == hipSuccess && depth_out) {
        e = hipMemcpyAsync(depth_out, d_depth.get(), (size_t)nplanes * w.nkmers * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_copytable_profile: %s", hipGetErrorString(e));
    g_copies_ms[2] = total_ms;
    copies_stitch(sq->n, w.first.data(), nplanes, COPIES_BINS, partial.data(), valid_partial.data(), hist_out, valid_out);
    return PG_OK;
}

// the sample's column (plane >= min_count) joined with the rows of `r` over windows of its contigs: launches of k_sample_agree over
// the chunks of all windows, the chunks' partials summed per window on the host
int copytable_sample_agree(pg_copytable *ct, uint32_t plane, uint32_t min_count, const pg_seqset *anchor, pg_result *r, uint32_t nwin,
                           const uint32_t *contig, const uint64_t *starts, const uint64_t *ends, uint64_t *valid_out, uint64_t *held_out,
                           uint64_t *col_out, uint64_t *both_out) {
    const char *fn = "pg_copytable_sample_agree";
    if (min_count == 0) return fail(PG_E_INVALID, "%s: min_count must be >= 1", fn);
    if (plane >= ct->nplanes) return fail(PG_E_INVALID, "%s: plane %u of %u", fn, plane, ct->nplanes);
    if (ct->ctx != anchor->ctx || ct->ctx != r->ctx) return fail(PG_E_INVALID, "%s: table, anchor and rows belong to different contexts", fn);
    if (ct->overflowed) return fail(PG_E_CAPACITY, "%s: the table overflowed", fn);
    if (int e = check_window_call(r, 1, 1, nwin, fn, "windows")) return e;
    const uint32_t N = r->N;
    if (N < 1 || N > PROFILE_MAX_GENOMES) return fail(PG_E_INVALID, "%s: %u genomes (1 to %u)", fn, N, PROFILE_MAX_GENOMES);
    if (r->k != ct->k) return fail(PG_E_INVALID, "%s: rows of k = %d, a table of k = %d", fn, r->k, ct->k);
    if (anchor->n != r->ad.size())
        return fail(PG_E_INVALID, "%s: the anchor has %u contigs, the rows %zu", fn, anchor->n, r->ad.size());
    for (uint32_t c = 0; c < anchor->n; ++c) {
        const uint64_t len = anchor->desc[c].len, nk = len >= (uint64_t)ct->k ? len - ct->k + 1 : 0;
        if (r->ad[c].nkmers != nk)
            return fail(PG_E_INVALID, "%s: contig %u has %u rows, its %llu bases hold %llu k-mers", fn, c, r->ad[c].nkmers,
                        (unsigned long long)len, (unsigned long long)nk);
    }
    Windows w;
    if (int e = gather_windows(r, 1, 1, nwin, contig, starts, ends, "window", w)) return e;
    place_ms()[1] = 0;
    if (nwin == 0) return PG_OK;
    std::fill(valid_out, valid_out + nwin, 0ull);
    std::fill(held_out, held_out + nwin, 0ull);
    std::fill(col_out, col_out + (size_t)nwin * N, 0ull);
    std::fill(both_out, both_out + (size_t)nwin * N, 0ull);
    std::vector<uint2> chunks;
    std::vector<uint64_t> first;
    if (int e = cut_chunks(fn, nwin, starts, ends, PLACE_CHUNK, chunks, &first)) return e;
    if (chunks.empty()) return PG_OK;  // (every window empty: zeros)
    const size_t nchunks = chunks.size();
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    const size_t per = std::max<size_t>(1, COPIES_PARTIAL_BYTES / ((size_t)(N + 1) * sizeof(uint2)));  // chunks per launch
    const std::vector<uint32_t> wc(contig, contig + nwin);
    DevBuf<uint2> d_chunks, d_part;  // [n][N] {col, both}, then [n] {valid, held}
    DevBuf<uint32_t> d_wc;
    std::vector<uint2> part(std::min(per, nchunks) * (N + 1));
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_chunks.upload(chunks, st);
    if (e == hipSuccess) e = d_wc.upload(wc, st);
    if (e == hipSuccess) e = d_part.alloc(part.size());
    if (e == hipErrorOutOfMemory) return fail(PG_E_CAPACITY, "%s: no memory for %zu chunks of %u genomes", fn, nchunks, N);
    float total_ms = 0;
    uint32_t win = 0;  // (the chunks are in window order)
    for (size_t c0 = 0; c0 < nchunks && e == hipSuccess; c0 += per) {
        const size_t n = std::min(per, nchunks - c0);
        float ms = 0;
        LaunchTimer tm(&ms);
        e = tm.start(st);
        if (e == hipSuccess)
            e = launch_sample_agree(st, N, ct->k, r->d_out1, w.base(), w.ends(), d_chunks.get() + c0, (uint32_t)n, d_wc.get(), anchor->d_desc,
                                    anchor->d_seqw, anchor->d_nmw, anchor->d_has_n, ct->d_keys, ct->nslots, ct->max_probe,
                                    ct->d_planes + (size_t)plane * ct->nslots, min_count, d_part.get(), d_part.get() + n * N);
        if (e == hipSuccess) e = tm.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(part.data(), d_part.get(), n * (N + 1) * sizeof(uint2), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        tm.read();
        total_ms += ms;
        for (size_t c = 0; c < n; ++c) {
            while (c0 + c >= first[win + 1]) ++win;
            const uint2 *p = part.data() + c * N;
            for (uint32_t g = 0; g < N; ++g) {
                col_out[(size_t)win * N + g] += p[g].x;
                both_out[(size_t)win * N + g] += p[g].y;
            }
            valid_out[win] += part[n * N + c].x;
            held_out[win] += part[n * N + c].y;
        }
    }
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    place_ms()[1] = total_ms;
    return PG_OK;
}

// the ranges of an allele call checked and cut into pieces: range i's pieces are [first[i], first[i + 1])
int allele_pieces(const char *fn, const pg_copytable *ct, const pg_seqset *sq, uint64_t n, const uint32_t *contig, const uint64_t *start,
                  const uint64_t *len, std::vector<AllelePiece> &pieces, std::vector<uint64_t> &first) {
    if (ct->ctx != sq->ctx) return fail(PG_E_INVALID, "%s: table and seqset belong to different contexts", fn);
    first.assign((size_t)n + 1, 0);
    uint64_t npieces = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (contig[i] >= sq->n) return fail(PG_E_INVALID, "%s: range %llu names contig %u of %u", fn, (unsigned long long)i, contig[i], sq->n);
        const uint64_t L = sq->desc[contig[i]].len;
        if (start[i] > L || len[i] > L - start[i])
            return fail(PG_E_INVALID, "%s: range %llu, bases [%llu, %llu + %llu) of a contig of %llu", fn, (unsigned long long)i,
                        (unsigned long long)start[i], (unsigned long long)start[i], (unsigned long long)len[i], (unsigned long long)L);
        uint64_t p0, p1;
        allele_windows(L, (uint32_t)ct->k, start[i], len[i], &p0, &p1);
        first[i] = npieces;
        npieces += allele_piece_count(p1 - p0);
        if (npieces > 0x7FFFFFFFull) return fail(PG_E_INVALID, "%s: more than 2^31 - 1 pieces of %u windows", fn, ALLELE_PIECE);
    }
    first[n] = npieces;
    pieces.clear();
    pieces.reserve(npieces);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t p0, p1;
        allele_windows(sq->desc[contig[i]].len, (uint32_t)ct->k, start[i], len[i], &p0, &p1);
        allele_cut(contig[i], p0, p1, pieces);
    }
    return PG_OK;
}

int copytable_insert_ranges(pg_copytable *ct, const pg_seqset *sq, uint64_t n, const uint32_t *contig, const uint64_t *start,
                            const uint64_t *len, uint64_t *distinct) {
    const char *fn = "pg_copytable_insert_ranges";
    std::vector<AllelePiece> pieces;
    std::vector<uint64_t> first;
    if (int r = allele_pieces(fn, ct, sq, n, contig, start, len, pieces, first)) return r;
    if (ct->overflowed) return fail(PG_E_CAPACITY, "%s: the table overflowed before", fn);
    if (int r = use_device(ct->ctx)) return r;
    *distinct = 0;
    g_genotype_ms[0] = 0;
    if (pieces.empty()) return PG_OK;
    hipStream_t st = ct->ctx->stream;
    DevBuf<AllelePiece> d_pieces;
    DevBuf<unsigned long long> d_ctr;
    unsigned long long ctr[2] = {0, 0};
    LaunchTimer tm(&g_genotype_ms[0]);
    hipError_t e = d_pieces.upload(pieces, st);
    if (e == hipSuccess) e = d_ctr.alloc(2);
    if (e == hipErrorOutOfMemory) return fail(PG_E_CAPACITY, "%s: no memory for %zu pieces", fn, pieces.size());
    if (e == hipSuccess) e = hipMemsetAsync(d_ctr.get(), 0, sizeof ctr, st);
    if (e == hipSuccess) e = tm.start(st);
    if (e == hipSuccess)
        e = launch_allele_insert(st, ct->k, sq->d_desc, d_pieces.get(), (uint32_t)pieces.size(), sq->d_seqw, sq->d_nmw, sq->d_has_n, ct->d_keys,
                                 ct->nslots, ct->max_probe, d_ctr.get());
    if (e == hipSuccess) e = tm.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_ctr.get(), sizeof ctr, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    tm.read();
    *distinct = ctr[1];
    if (ctr[0]) {
        ct->overflowed = true;
        return fail(PG_E_CAPACITY, "%s: %llu slots (created for %llu keys) do not hold the ranges' k-mers", fn,
                    (unsigned long long)ct->nslots, (unsigned long long)ct->capacity);
    }
    return PG_OK;
}

int copytable_allele_support(pg_copytable *ct, const pg_seqset *sq, uint64_t n, const uint32_t *contig, const uint64_t *start,
                             const uint64_t *len, uint32_t own, uint32_t other, uint32_t sample, uint32_t min_count, uint64_t *windows_out,
                             uint64_t *inf_out, uint64_t *seen_out, uint64_t *depth_out) {
    const char *fn = "pg_copytable_allele_support";
    if (own >= ct->nplanes || other >= ct->nplanes || sample >= ct->nplanes)
        return fail(PG_E_INVALID, "%s: planes %u, %u, %u of %u", fn, own, other, sample, ct->nplanes);
    if (own == other) return fail(PG_E_INVALID, "%s: own and other are both plane %u", fn, own);
    if (min_count == 0) return fail(PG_E_INVALID, "%s: min_count must be >= 1", fn);
    std::vector<AllelePiece> pieces;
    std::vector<uint64_t> first;
    if (int r = allele_pieces(fn, ct, sq, n, contig, start, len, pieces, first)) return r;
    if (ct->overflowed) return fail(PG_E_CAPACITY, "%s: the table overflowed", fn);
    if (int r = use_device(ct->ctx)) return r;
    g_genotype_ms[1] = 0;
    if (n == 0) return PG_OK;
    for (uint64_t *out : {windows_out, inf_out, seen_out, depth_out}) std::fill(out, out + n, 0ull);
    if (pieces.empty()) return PG_OK;  // (no range has a window: zeros)
    const size_t npieces = pieces.size();
    const size_t per = std::min(npieces, COPIES_PARTIAL_BYTES / sizeof(AllelePartial));  // pieces per launch
    hipStream_t st = ct->ctx->stream;
    DevBuf<AllelePiece> d_pieces;
    DevBuf<AllelePartial> d_part;
    std::vector<AllelePartial> part(per);
    hipError_t e = d_pieces.upload(pieces, st);
    if (e == hipSuccess) e = d_part.alloc(per);
    if (e == hipErrorOutOfMemory) return fail(PG_E_CAPACITY, "%s: no memory for %zu pieces", fn, npieces);
    float total_ms = 0;
    for (size_t c0 = 0; c0 < npieces && e == hipSuccess; c0 += per) {
        const size_t m = std::min(per, npieces - c0);
        float ms = 0;
        LaunchTimer tm(&ms);
        e = tm.start(st);
        if (e == hipSuccess)
            e = launch_allele_support(st, ct->k, sq->d_desc, d_pieces.get() + c0, (uint32_t)m, sq->d_seqw, sq->d_nmw, sq->d_has_n, ct->d_keys,
                                      ct->nslots, ct->max_probe, ct->d_planes + (size_t)own * ct->nslots,
                                      ct->d_planes + (size_t)other * ct->nslots, ct->d_planes + (size_t)sample * ct->nslots, min_count,
                                      d_part.get());
        if (e == hipSuccess) e = tm.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(part.data(), d_part.get(), m * sizeof(AllelePartial), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        tm.read();
        total_ms += ms;
        allele_stitch(n, first.data(), part.data(), c0, m, windows_out, inf_out, seen_out, depth_out);
    }
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    g_genotype_ms[1] = total_ms;
    return PG_OK;
}

}  // namespace

extern "C" int pg_copytable_create(pg_ctx *ctx, int k, uint64_t capacity_keys, uint32_t nplanes, pg_copytable **out) {
    PG_API_BEGIN
    if (!ctx || !out) return fail(PG_E_INVALID, "pg_copytable_create: NULL argument");
    return copytable_create(ctx, k, capacity_keys, nplanes, out);
    PG_API_END
}

extern "C" int pg_copytable_destroy(pg_copytable *ct) {
    PG_API_BEGIN
    if (ct) copytable_free(ct);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_copytable_insert_seqset(pg_copytable *ct, const pg_seqset *targets, uint64_t *distinct) {
    PG_API_BEGIN
    if (!ct || !targets || !distinct) return fail(PG_E_INVALID, "pg_copytable_insert_seqset: NULL argument");
    return copytable_insert(ct, targets, distinct);
    PG_API_END
}

extern "C" int pg_copytable_count_seqset(pg_copytable *ct, uint32_t plane, const pg_seqset *genome, uint64_t *hits) {
    PG_API_BEGIN
    if (!ct || !genome || !hits) return fail(PG_E_INVALID, "pg_copytable_count_seqset: NULL argument");
    return copytable_count(ct, plane, genome, hits);
    PG_API_END
}

extern "C" int pg_copytable_clear_plane(pg_copytable *ct, uint32_t plane) {
    PG_API_BEGIN
    if (!ct) return fail(PG_E_INVALID, "pg_copytable_clear_plane: NULL argument");
    if (plane >= ct->nplanes) return fail(PG_E_INVALID, "pg_copytable_clear_plane: plane %u of %u", plane, ct->nplanes);
    if (int r = use_device(ct->ctx)) return r;
    HIP_TRY(hipMemsetAsync(ct->d_planes + (size_t)plane * ct->nslots, 0, ct->nslots * 4, ct->ctx->stream));
    HIP_TRY(hipStreamSynchronize(ct->ctx->stream));
    return PG_OK;
    PG_API_END
}

extern "C" int pg_copytable_profile(pg_copytable *ct, const pg_seqset *seqs, uint32_t plane0, uint32_t nplanes, uint64_t *hist_out,
                                    uint64_t *valid_out, uint16_t *depth_out) {
    PG_API_BEGIN
    if (!ct || !seqs || !hist_out || !valid_out) return fail(PG_E_INVALID, "pg_copytable_profile: NULL argument");
    return copytable_profile(ct, seqs, plane0, nplanes, hist_out, valid_out, depth_out);
    PG_API_END
}

extern "C" int pg_copytable_sample_agree(pg_copytable *ct, uint32_t plane, uint32_t min_count, const pg_seqset *anchor, pg_result *rows,
                                         uint32_t nwin, const uint32_t *contig, const uint64_t *starts, const uint64_t *ends,
                                         uint64_t *valid_out, uint64_t *held_out, uint64_t *col_out, uint64_t *both_out) {
    PG_API_BEGIN
    if (!ct || !anchor || !rows || (nwin && (!contig || !starts || !ends || !valid_out || !held_out || !col_out || !both_out)))
        return fail(PG_E_INVALID, "pg_copytable_sample_agree: NULL argument");
    return copytable_sample_agree(ct, plane, min_count, anchor, rows, nwin, contig, starts, ends, valid_out, held_out, col_out, both_out);
    PG_API_END
}

extern "C" int pg_place_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_place_last_timing: NULL argument");
    std::copy(place_ms(), place_ms() + 2, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_copies_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_copies_last_timing: NULL argument");
    std::copy(g_copies_ms, g_copies_ms + 3, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_copytable_insert_ranges(pg_copytable *ct, const pg_seqset *seqs, uint64_t n, const uint32_t *contig, const uint64_t *start,
                                          const uint64_t *len, uint64_t *distinct) {
    PG_API_BEGIN
    if (!ct || !seqs || !distinct || (n && (!contig || !start || !len))) return fail(PG_E_INVALID, "pg_copytable_insert_ranges: NULL argument");
    return copytable_insert_ranges(ct, seqs, n, contig, start, len, distinct);
    PG_API_END
}

extern "C" int pg_copytable_allele_support(pg_copytable *ct, const pg_seqset *seqs, uint64_t n, const uint32_t *contig,
                                           const uint64_t *start, const uint64_t *len, uint32_t own_plane, uint32_t other_plane,
                                           uint32_t sample_plane, uint32_t min_count, uint64_t *windows_out, uint64_t *inf_out,
                                           uint64_t *seen_out, uint64_t *depth_out) {
    PG_API_BEGIN
    if (!ct || !seqs || (n && (!contig || !start || !len || !windows_out || !inf_out || !seen_out || !depth_out)))
        return fail(PG_E_INVALID, "pg_copytable_allele_support: NULL argument");
    return copytable_allele_support(ct, seqs, n, contig, start, len, own_plane, other_plane, sample_plane, min_count, windows_out, inf_out,
                                    seen_out, depth_out);
    PG_API_END
}

extern "C" int pg_genotype_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_genotype_last_timing: NULL argument");
    std::copy(g_genotype_ms, g_genotype_ms + 2, ms_out);
    return PG_OK;
    PG_API_END
}
