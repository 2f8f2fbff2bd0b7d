// pg_api_screen.hip — host side of the C-ABI: a sample screened against the pan table (pg_screen.hip): the counter plane beside
// the table's slots, sequence sets marked into it, and the pass that joins it with the masks.
#include "pg_host.h"

#include "pg_keytable_host.h"

struct pg_screen {
    pg_ctx *ctx;
    pg_table *tbl;
    uint8_t *d_plane = nullptr;  // one byte per slot, rounded up to whole dwords
    uint64_t plane_bytes = 0;
    // the geometry the plane belongs to: a re-hash, an insert of new keys, a clear or a regrow behind the handle changes one of
    // them (an insert that only sets bits of keys already there moves no key: the bytes are still those keys')
    const uint8_t *buckets;
    uint64_t nbuckets, count;
    uint32_t slots, layout;
};

namespace {

thread_local float g_screen_ms[2] = {0, 0};  // k_table_mark, k_table_screen of this thread's last calls

void screen_free(pg_screen *s) {
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    if (s->d_plane) hipFree(s->d_plane);
    pg_table *t = s->tbl;
    delete s;
    table_release(t);
}

// the table as the plane knows it, or an error: a stale plane must not answer
int screen_table(const pg_screen *s, const char *fn, const SubTable **out) {
    const pg_table *t = s->tbl;
    if (t->dead) return fail(PG_E_INVALID, "%s: the table was destroyed", fn);
    if (t->subs.size() != 1) return fail(PG_E_INVALID, "%s: a table of %zu sub-tables", fn, t->subs.size());
    const SubHost &h = t->subs[0];
    if (h.d.buckets != s->buckets || h.d.nbuckets != s->nbuckets || h.d.slots != s->slots || h.d.layout != s->layout || h.count != s->count)
        return fail(PG_E_INVALID,
                    "%s: the table changed behind the screen (%llu lines of %u slots and %llu keys when it was created, %llu of %u and "
                    "%llu now): create a new one",
                    fn, (unsigned long long)s->nbuckets, s->slots, (unsigned long long)s->count, (unsigned long long)h.d.nbuckets, h.d.slots,
                    (unsigned long long)h.count);
    *out = &h.d;
    return PG_OK;
}

int screen_create(pg_table *t, pg_screen **out) {
    if (t->dead) return fail(PG_E_INVALID, "pg_screen_create: the table was destroyed");
    if (t->subs.size() != 1) return fail(PG_E_INVALID, "pg_screen_create: a table of %zu sub-tables", t->subs.size());
    if (int r = use_device(t->ctx)) return r;
    TABLE_WRITER(t);  // (a reader of the geometry: no re-hash swaps the lines meanwhile)
    const SubHost &h = t->subs[0];
    std::unique_ptr<pg_screen> s(new pg_screen);
    s->ctx = t->ctx;
    s->tbl = t;
    s->buckets = h.d.buckets;
    s->nbuckets = h.d.nbuckets;
    s->slots = h.d.slots;
    s->layout = h.d.layout;
    s->count = h.count;
    s->plane_bytes = (h.d.nbuckets * h.d.slots + 3) & ~3ull;
    DevBuf<uint8_t> plane;
    hipError_t e = plane.alloc(std::max<uint64_t>(s->plane_bytes, 4));
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PG_E_CAPACITY : PG_E_HIP, "pg_screen_create: a plane of %llu bytes: %s",
                    (unsigned long long)s->plane_bytes, hipGetErrorString(e));
    e = hipMemsetAsync(plane.get(), 0, std::max<uint64_t>(s->plane_bytes, 4), t->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->ctx->stream);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_screen_create: %s", hipGetErrorString(e));
    std::swap(s->d_plane, plane.p);
    ++t->refs;
    *out = s.release();
    return PG_OK;
}

int screen_add(pg_screen *s, const pg_seqset *sq, uint64_t *windows, uint64_t *hits) {
    const char *fn = "pg_screen_add_seqset";
    if (s->ctx != sq->ctx) return fail(PG_E_INVALID, "%s: screen and seqset belong to different contexts", fn);
    pg_table *t = s->tbl;
    TABLE_WRITER(t);  // (a reader: it keeps a second host thread's re-hash from freeing the lines under the kernel)
    const SubTable *st = nullptr;
    if (int r = screen_table(s, fn, &st)) return r;
    if ((int)st->k != t->k || t->k < 1 || t->k > 32) return fail(PG_E_INVALID, "%s: a table of k = %d whose lines are of k = %u", fn, t->k, st->k);
    KmerWalk w;
    if (int r = walk_kmers(sq, t->k, SCREEN_JOB, fn, w)) return r;
    if (int r = use_device(s->ctx)) return r;
    *windows = *hits = 0;
    g_screen_ms[0] = 0;
    if (w.jobs.empty()) return PG_OK;
    hipStream_t stream = s->ctx->stream;
    unsigned long long ctr[2] = {0, 0};
    const hipError_t e = counted_launch(stream, w.jobs, ctr, 2, &g_screen_ms[0], [&](const uint2 *jobs, uint32_t njobs, unsigned long long *d_ctr) {
        return launch_table_mark(stream, *st, sq->d_desc, jobs, njobs, sq->d_seqw, sq->d_nmw, sq->d_has_n, s->d_plane, d_ctr);
    });
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    *windows = ctr[0];
    *hits = ctr[1];
    return PG_OK;
}

int screen_result(pg_screen *s, uint32_t min_count, uint64_t *distinct, uint64_t *seen, uint64_t *priv, uint64_t *priv_seen, uint64_t *occ,
                  uint64_t *seen_occ, uint64_t *depth_hist, uint64_t *core_depth_hist, uint64_t *nkeys) {
    const char *fn = "pg_screen_result";
    if (min_count < 1 || min_count > SCREEN_DEPTH_MAX) return fail(PG_E_INVALID, "%s: min_count %u (1 to %u)", fn, min_count, SCREEN_DEPTH_MAX);
    pg_table *t = s->tbl;
    if (t->ngenomes < 1 || t->ngenomes > (int)PAIRS_MAX_GENOMES)
        return fail(PG_E_INVALID, "%s: %d genomes (the screen takes 1 to %u)", fn, t->ngenomes, PAIRS_MAX_GENOMES);
    TABLE_WRITER(t);
    const SubTable *st = nullptr;
    if (int r = screen_table(s, fn, &st)) return r;
    if (int r = use_device(s->ctx)) return r;
    const uint32_t N = (uint32_t)t->ngenomes;
    const size_t ntotal = screen_out_words(N);
    hipStream_t stream = s->ctx->stream;
    DevBuf<unsigned long long> d_out;
    std::vector<uint64_t> h(ntotal, 0);
    g_screen_ms[1] = 0;
    LaunchTimer tm(&g_screen_ms[1]);
    hipError_t e = d_out.alloc(ntotal);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, ntotal * 8, stream);
    if (e == hipSuccess) e = tm.start(stream);
    if (e == hipSuccess) e = launch_table_screen(stream, *st, N, s->d_plane, min_count, d_out.get());
    if (e == hipSuccess) e = tm.stop(stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_out.get(), ntotal * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    tm.read();
    // (the order of launch_table_screen's out)
    const uint64_t *p = h.data();
    uint64_t *const dst[8] = {distinct, seen, priv, priv_seen, occ, seen_occ, depth_hist, core_depth_hist};
    const size_t len[8] = {N, N, N, N, (size_t)N + 1, (size_t)N + 1, SCREEN_BINS, SCREEN_BINS};
    for (int i = 0; i < 8; ++i) {
        if (dst[i]) std::copy(p, p + len[i], dst[i]);
        p += len[i];
    }
    if (nkeys) *nkeys = *p;
    return PG_OK;
}

}  // namespace

extern "C" int pg_screen_create(pg_table *tbl, pg_screen **out) {
    PG_API_BEGIN
    if (!tbl || !out) return fail(PG_E_INVALID, "pg_screen_create: NULL argument");
    return screen_create(tbl, out);
    PG_API_END
}

extern "C" int pg_screen_destroy(pg_screen *s) {
    PG_API_BEGIN
    if (s) screen_free(s);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_screen_add_seqset(pg_screen *s, const pg_seqset *seqs, uint64_t *windows, uint64_t *hits) {
    PG_API_BEGIN
    if (!s || !seqs || !windows || !hits) return fail(PG_E_INVALID, "pg_screen_add_seqset: NULL argument");
    return screen_add(s, seqs, windows, hits);
    PG_API_END
}

extern "C" int pg_screen_result(pg_screen *s, uint32_t min_count, uint64_t *distinct, uint64_t *seen, uint64_t *priv, uint64_t *priv_seen,
                                uint64_t *occ, uint64_t *seen_occ, uint64_t *depth_hist, uint64_t *core_depth_hist, uint64_t *nkeys) {
    PG_API_BEGIN
    if (!s) return fail(PG_E_INVALID, "pg_screen_result: NULL argument");
    return screen_result(s, min_count, distinct, seen, priv, priv_seen, occ, seen_occ, depth_hist, core_depth_hist, nkeys);
    PG_API_END
}

extern "C" int pg_screen_clear(pg_screen *s) {
    PG_API_BEGIN
    if (!s) return fail(PG_E_INVALID, "pg_screen_clear: NULL argument");
    if (int r = use_device(s->ctx)) return r;
    HIP_TRY(hipMemsetAsync(s->d_plane, 0, std::max<uint64_t>(s->plane_bytes, 4), s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return PG_OK;
    PG_API_END
}

extern "C" int pg_screen_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_screen_last_timing: NULL argument");
    std::copy(g_screen_ms, g_screen_ms + 2, ms_out);
    return PG_OK;
    PG_API_END
}
