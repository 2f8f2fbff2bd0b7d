// pg_api_novel.hip — host side of the C-ABI: what a sample holds that the pan table does not (pg_novel.hip): the novel key table
// that sequence sets are counted into and that grows in front of them, the pass over its slots, the novel runs of an assembly, and
// the solid keys compacted into unitigs (pg_unitigs.hip).
#include "pg_host.h"

#include "pg_keytable_host.h"
#include "pg_runs_host.h"  // RunsOut, runs_two_pass

static constexpr uint64_t NOVEL_MAX_KEYS = COPIES_MAX_SLOTS / 2;  // (table_slots: the power of two at or above 2 * keys)
static constexpr uint64_t NOVEL_MAX_WINDOWS = 0xFFFFFFFFull;      // of one handle: a depth is 32 bits
static constexpr uint64_t NOVEL_MAX_CONTIG = 0xFFFFFFFFull;       // k-mer positions of one contig of pg_novel_runs: a run's end is a word

struct pg_novel {
    pg_ctx *ctx;
    pg_table *tbl;
    unsigned long long *d_keys = nullptr;
    uint32_t *d_depth = nullptr;
    uint64_t nslots = 0, nkeys = 0, windows = 0;  // windows: the valid windows added since the last clear
    uint32_t max_probe = 0, grown = 0;
    bool overflowed = false;  // a claim gave up (the reservation makes that impossible): the depths are short and answer nothing
    // the geometry of the pan table the keys were filtered by (pg_screen's rule: a re-hash, an insert of new keys, a clear or a
    // regrow behind the handle changes one of them)
    const uint8_t *buckets;
    uint64_t nbuckets, count;
    uint32_t slots, layout;
    // what pg_novel_links and pg_novel_unitigs keep between a counting call and a filling call, for ONE min_count: the two byte
    // planes and the walks' counts.  An add and a clear drop it (unitig_drop): the slots it speaks of are other slots then
    struct Unitigs {
        uint32_t min_count = 0;  // 0: nothing kept
        uint8_t *d_links = nullptr, *d_marks = nullptr;
        // pg_novel_clean ran for this min_count: d_drop is the third plane (a set byte: no node any more), the two planes above are
        // those of the cleaned graph, and its nodes — all and per block of the scan — stand where the scan's solid keys stood
        uint8_t *d_drop = nullptr;
        uint64_t nodes = 0;
        std::vector<uint32_t> block_nodes;
        bool walked = false;                   // the counts below stand and `marks` holds the winners of both rounds
        std::vector<ulonglong2> lin, circ;     // per block of the scan: {winners, their nodes} of the linear / the circular round
        uint64_t nlin = 0, lin_nodes = 0, ncirc = 0, circ_nodes = 0;
        float ms[3] = {0, 0, 0};  // the kernels' times since the planes were built: what pg_novel_unitigs_last_timing reads behind a call on this handle
    } ut;
};

namespace {

thread_local float g_novel_ms[4] = {0, 0, 0, 0};  // k_novel_count, k_novel_grow, k_novel_scan (both passes), k_novel_runs (both passes)

thread_local float g_unitig_ms[3] = {0, 0, 0};  // k_unitig_links, k_unitig_walk of the linear round (all passes), of the circular round
thread_local float g_clean_ms[2] = {0, 0};      // the k_unitig_links passes and the k_unitig_clean passes of the last pg_novel_clean

// (behind a synchronise of the handle's stream: no kernel reads the planes)
void unitig_drop(pg_novel *nv) {
    if (nv->ut.d_links) hipFree(nv->ut.d_links);
    if (nv->ut.d_marks) hipFree(nv->ut.d_marks);
    if (nv->ut.d_drop) hipFree(nv->ut.d_drop);
    nv->ut = pg_novel::Unitigs();
}

void novel_free(pg_novel *nv) {
    hipSetDevice(nv->ctx->device);
    hipStreamSynchronize(nv->ctx->stream);
    unitig_drop(nv);
    if (nv->d_depth) hipFree(nv->d_depth);
    if (nv->d_keys) hipFree(nv->d_keys);
    pg_table *t = nv->tbl;
    delete nv;
    table_release(t);
}

// the pan table as a caller may read it (its writer lock held), or an error
int pan_table(const pg_table *t, const char *fn, const SubTable **out) {
    if (t->dead) return fail(PG_E_INVALID, "%s: the table was destroyed", fn);
    if (t->subs.size() != 1) return fail(PG_E_INVALID, "%s: a table of %zu sub-tables", fn, t->subs.size());
    const SubTable &d = t->subs[0].d;
    if ((int)d.k != t->k || t->k < 1 || t->k > 32) return fail(PG_E_INVALID, "%s: a table of k = %d whose lines are of k = %u", fn, t->k, d.k);
    *out = &d;
    return PG_OK;
}

// ... as the handle knows it: keys filtered by another geometry or key count must not be added to
int novel_table(const pg_novel *nv, const char *fn, const SubTable **out) {
    if (int r = pan_table(nv->tbl, fn, out)) return r;
    const SubHost &h = nv->tbl->subs[0];
    if (h.d.buckets != nv->buckets || h.d.nbuckets != nv->nbuckets || h.d.slots != nv->slots || h.d.layout != nv->layout || h.count != nv->count)
        return fail(PG_E_INVALID,
                    "%s: the table changed behind the novel table (%llu lines of %u slots and %llu keys when it was created, %llu of %u and "
                    "%llu now): create a new one",
                    fn, (unsigned long long)nv->nbuckets, nv->slots, (unsigned long long)nv->count, (unsigned long long)h.d.nbuckets, h.d.slots,
                    (unsigned long long)h.count);
    return PG_OK;
}

// keys and depths of `nslots` free slots
hipError_t novel_alloc(hipStream_t st, uint64_t nslots, DevBuf<unsigned long long> &keys, DevBuf<uint32_t> &depth) {
    hipError_t e = keys.alloc(nslots);
    if (e == hipSuccess) e = depth.alloc(nslots);
    if (e == hipSuccess) e = hipMemsetAsync(keys.get(), 0xFF, nslots * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(depth.get(), 0, nslots * 4, st);
    return e;
}

int novel_create(pg_table *t, uint64_t capacity, pg_novel **out) {
    const char *fn = "pg_novel_create";
    if (capacity < 1 || capacity > NOVEL_MAX_KEYS) return fail(PG_E_INVALID, "%s: capacity of %llu keys (1 to 2^30)", fn, (unsigned long long)capacity);
    if (int r = use_device(t->ctx)) return r;
    TABLE_WRITER(t);  // (a reader of the geometry: no re-hash swaps the lines meanwhile)
    const SubTable *st = nullptr;
    if (int r = pan_table(t, fn, &st)) return r;
    const SubHost &h = t->subs[0];
    std::unique_ptr<pg_novel> nv(new pg_novel);
    nv->ctx = t->ctx;
    nv->tbl = t;
    nv->buckets = h.d.buckets;
    nv->nbuckets = h.d.nbuckets;
    nv->slots = h.d.slots;
    nv->layout = h.d.layout;
    nv->count = h.count;
    nv->nslots = table_slots(capacity);
    nv->max_probe = table_max_probe(nv->nslots);
    DevBuf<unsigned long long> keys;
    DevBuf<uint32_t> depth;
    hipError_t e = novel_alloc(t->ctx->stream, nv->nslots, keys, depth);
    if (e == hipSuccess) e = hipStreamSynchronize(t->ctx->stream);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PG_E_CAPACITY : PG_E_HIP, "%s: %llu slots: %s", fn, (unsigned long long)nv->nslots, hipGetErrorString(e));
    std::swap(nv->d_keys, keys.p);
    std::swap(nv->d_depth, depth.p);
    ++t->refs;
    *out = nv.release();
    return PG_OK;
}

// room for `incoming` more keys at a load of 0.5 at the most: the table re-hashed into one of twice the slots or more (k_novel_grow).
// Nothing of the handle changes when a reservation is refused
int novel_reserve(pg_novel *nv, uint64_t incoming, const char *fn) {
    g_novel_ms[1] = 0;
    const uint64_t need = nv->nkeys + incoming;
    if (2 * need <= nv->nslots) return PG_OK;
    if (need > NOVEL_MAX_KEYS)
        return fail(PG_E_CAPACITY,
                    "%s: %llu novel keys and %llu k-mer positions to add (a novel table holds 2^30 keys with the positions of one sequence set): "
                    "lower --batch-bytes",
                    fn, (unsigned long long)nv->nkeys, (unsigned long long)incoming);
    const uint64_t nslots = table_slots(need);
    const uint32_t max_probe = table_max_probe(nslots);
    hipStream_t st = nv->ctx->stream;
    DevBuf<unsigned long long> keys, d_flag;
    DevBuf<uint32_t> depth;
    unsigned long long flag = 0;
    LaunchTimer tm(&g_novel_ms[1]);
    hipError_t e = novel_alloc(st, nslots, keys, depth);
    if (e == hipErrorOutOfMemory) {
        hipStreamSynchronize(st);
        return fail(PG_E_CAPACITY, "%s: no memory for a novel table of %llu slots: lower --batch-bytes", fn, (unsigned long long)nslots);
    }
    if (e == hipSuccess && nv->nkeys) {
        e = d_flag.alloc(1);
        if (e == hipSuccess) e = hipMemsetAsync(d_flag.get(), 0, 8, st);
        if (e == hipSuccess) e = tm.start(st);
        if (e == hipSuccess) e = launch_novel_grow(st, nv->d_keys, nv->d_depth, nv->nslots, keys.get(), depth.get(), nslots, max_probe, d_flag.get());
        if (e == hipSuccess) e = tm.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag.get(), 8, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);
        return fail(PG_E_HIP, "%s: growing to %llu slots: %s", fn, (unsigned long long)nslots, hipGetErrorString(e));
    }
    if (nv->nkeys) tm.read();
    if (flag) {  // (a load below 0.25: a walk of max_probe slots never fills)
        nv->overflowed = true;
        return fail(PG_E_CAPACITY, "%s: %llu slots did not take the table's %llu keys", fn, (unsigned long long)nslots, (unsigned long long)nv->nkeys);
    }
    std::swap(nv->d_keys, keys.p);  // (the old arrays go with this scope)
    std::swap(nv->d_depth, depth.p);
    nv->nslots = nslots;
    nv->max_probe = max_probe;
    ++nv->grown;
    return PG_OK;
}

int novel_add(pg_novel *nv, const pg_seqset *sq, uint64_t *windows, uint64_t *hits, uint64_t *new_keys) {
    const char *fn = "pg_novel_add_seqset";
    if (nv->ctx != sq->ctx) return fail(PG_E_INVALID, "%s: novel table and seqset belong to different contexts", fn);
    if (nv->overflowed) return fail(PG_E_CAPACITY, "%s: the novel table overflowed before", fn);
    pg_table *t = nv->tbl;
    TABLE_WRITER(t);  // (a reader: it keeps a second host thread's re-hash from freeing the lines under the kernel)
    const SubTable *st = nullptr;
    if (int r = novel_table(nv, fn, &st)) return r;
    KmerWalk w;
    if (int r = walk_kmers(sq, t->k, NOVEL_JOB, fn, w)) return r;
    if (nv->windows + w.nkmers > NOVEL_MAX_WINDOWS)
        return fail(PG_E_INVALID, "%s: %llu windows added and %llu k-mer positions in this set (the depths hold 2^32 - 1 per handle)", fn,
                    (unsigned long long)nv->windows, (unsigned long long)w.nkmers);
    if (int r = use_device(nv->ctx)) return r;
    *windows = *hits = *new_keys = 0;
    g_novel_ms[0] = g_novel_ms[1] = 0;
    if (w.jobs.empty()) return PG_OK;
    unitig_drop(nv);  // (every call of this unit leaves the stream synchronised)
    if (int r = novel_reserve(nv, w.nkmers, fn)) return r;
    hipStream_t stream = nv->ctx->stream;
    unsigned long long ctr[4] = {0, 0, 0, 0};
    const hipError_t e = counted_launch(stream, w.jobs, ctr, 4, &g_novel_ms[0], [&](const uint2 *jobs, uint32_t njobs, unsigned long long *d_ctr) {
        return launch_novel_count(stream, *st, sq->d_desc, jobs, njobs, sq->d_seqw, sq->d_nmw, sq->d_has_n, nv->d_keys, nv->d_depth, nv->nslots,
                                  nv->max_probe, d_ctr);
    });
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    *windows = ctr[0];
    *hits = ctr[1];
    *new_keys = ctr[2];
    nv->windows += ctr[0];
    nv->nkeys += ctr[2];
    if (ctr[3]) {
        nv->overflowed = true;
        return fail(PG_E_CAPACITY, "%s: %llu claims found no slot among %llu", fn, (unsigned long long)ctr[3], (unsigned long long)nv->nslots);
    }
    return PG_OK;
}

// the count pass of k_novel_scan: h = its NOVEL_SCAN_WORDS words, block_solid (when asked for) the solid keys of every block
int novel_scan_count(pg_novel *nv, const char *fn, uint32_t min_count, uint64_t *h, std::vector<uint32_t> *block_solid, float *ms) {
    if (min_count < 1) return fail(PG_E_INVALID, "%s: min_count must be >= 1", fn);
    if (nv->overflowed) return fail(PG_E_CAPACITY, "%s: the novel table overflowed", fn);
    {
        TABLE_WRITER(nv->tbl);  // (a reader of the geometry)
        const SubTable *pan = nullptr;
        if (int r = novel_table(nv, fn, &pan)) return r;  // (keys filtered by a table that is gone answer nothing)
    }
    if (int r = use_device(nv->ctx)) return r;
    hipStream_t st = nv->ctx->stream;
    const uint32_t nblocks = novel_scan_blocks(nv->nslots);
    DevBuf<unsigned long long> d_out;
    DevBuf<uint32_t> d_bs;
    if (block_solid) block_solid->assign(nblocks, 0);
    LaunchTimer tm(ms);
    hipError_t e = d_out.alloc(NOVEL_SCAN_WORDS);
    if (e == hipSuccess) e = d_bs.alloc(nblocks);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, NOVEL_SCAN_WORDS * 8, st);
    if (e == hipSuccess) e = tm.start(st);
    if (e == hipSuccess) e = launch_novel_scan(st, nv->d_keys, nv->d_depth, nv->nslots, min_count, d_out.get(), d_bs.get(), nullptr, 0, nullptr, nullptr);
    if (e == hipSuccess) e = tm.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_out.get(), NOVEL_SCAN_WORDS * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && block_solid) e = hipMemcpyAsync(block_solid->data(), d_bs.get(), (size_t)nblocks * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);  // (the copies' targets are the caller's)
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    tm.read();
    if (h[0] != nv->nkeys)
        return fail(PG_E_HIP, "%s: the pass counted %llu keys, the adds claimed %llu", fn, (unsigned long long)h[0], (unsigned long long)nv->nkeys);
    return PG_OK;
}

int novel_result(pg_novel *nv, uint32_t min_count, uint64_t *nkeys, uint64_t *solid, uint64_t *solid_windows, uint64_t *depth_hist) {
    uint64_t h[NOVEL_SCAN_WORDS];
    g_novel_ms[2] = 0;
    if (int r = novel_scan_count(nv, "pg_novel_result", min_count, h, nullptr, &g_novel_ms[2])) return r;
    if (nkeys) *nkeys = h[0];
    if (solid) *solid = h[1];
    if (solid_windows) *solid_windows = h[2];
    if (depth_hist) std::copy(h + 3, h + 3 + NOVEL_BINS, depth_hist);
    return PG_OK;
}

int novel_keys(pg_novel *nv, uint32_t min_count, uint64_t cap, uint64_t *keys_out, uint32_t *depths_out, uint64_t *n) {
    const char *fn = "pg_novel_keys";
    uint64_t h[NOVEL_SCAN_WORDS];
    std::vector<uint32_t> block_solid;
    float ms_count = 0, ms_emit = 0;
    g_novel_ms[2] = 0;
    if (int r = novel_scan_count(nv, fn, min_count, h, &block_solid, &ms_count)) return r;
    g_novel_ms[2] = ms_count;
    *n = h[1];
    const uint64_t take = std::min<uint64_t>(h[1], cap);
    if (take == 0) return PG_OK;
    std::vector<uint64_t> offs(block_solid.size());
    uint64_t sum = 0;
    for (size_t b = 0; b < block_solid.size(); ++b) {
        offs[b] = sum;
        sum += block_solid[b];
    }
    if (sum != h[1]) return fail(PG_E_HIP, "%s: %llu solid keys by block, %llu in all", fn, (unsigned long long)sum, (unsigned long long)h[1]);
    hipStream_t st = nv->ctx->stream;
    DevBuf<uint64_t> d_offs;
    DevBuf<unsigned long long> d_k;
    DevBuf<uint32_t> d_d;
    LaunchTimer tm(&ms_emit);
    hipError_t e = d_offs.upload(offs, st);
    if (e == hipSuccess) e = d_k.alloc(take);
    if (e == hipSuccess) e = d_d.alloc(take);
    if (e == hipErrorOutOfMemory) {
        hipStreamSynchronize(st);
        return fail(PG_E_CAPACITY, "%s: no memory for %llu keys", fn, (unsigned long long)take);
    }
    if (e == hipSuccess) e = tm.start(st);
    if (e == hipSuccess) e = launch_novel_scan(st, nv->d_keys, nv->d_depth, nv->nslots, min_count, nullptr, nullptr, d_offs.get(), take, d_k.get(), d_d.get());
    if (e == hipSuccess) e = tm.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(keys_out, d_k.get(), take * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(depths_out, d_d.get(), take * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    tm.read();
    g_novel_ms[2] = ms_count + ms_emit;
    return PG_OK;
}

int novel_runs(pg_table *t, const pg_seqset *sq, uint64_t cap, uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint8_t *left_held,
               uint8_t *right_held, uint64_t *nruns, uint64_t *windows, uint64_t *novel_windows) {
    const char *fn = "pg_novel_runs";
    if (t->ctx != sq->ctx) return fail(PG_E_INVALID, "%s: table and seqset belong to different contexts", fn);
    TABLE_WRITER(t);  // (a reader, as pg_novel_add_seqset is)
    const SubTable *pan = nullptr;
    if (int r = pan_table(t, fn, &pan)) return r;
    KmerWalk w;
    w.noun = "chunks";
    if (int r = walk_kmers(sq, t->k, NOVEL_CHUNK, fn, w)) return r;
    for (uint32_t c = 0; c < sq->n; ++c)
        if ((c + 1 < sq->n ? w.koff[c + 1] : w.nkmers) - w.koff[c] > NOVEL_MAX_CONTIG)
            return fail(PG_E_INVALID, "%s: contig %u holds more than 2^32 - 1 k-mer positions", fn, c);
    for (uint2 &ck : w.jobs) ck.y *= NOVEL_CHUNK;  // (k_novel_runs takes a chunk's first position, below 2^32 behind the check above)
    *nruns = *windows = *novel_windows = 0;
    g_novel_ms[3] = 0;
    if (w.jobs.empty()) return PG_OK;
    if (int r = use_device(t->ctx)) return r;
    const uint32_t nchunks = (uint32_t)w.jobs.size();
    hipStream_t st = t->ctx->stream;
    DevBuf<uint2> d_chunks;
    const hipError_t e = d_chunks.upload(w.jobs, st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);  // (the upload's source goes with this scope)
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    const auto launch = [&](uint4 *counts, const ulonglong2 *offs, uint64_t n, uint32_t *words, uint8_t *bytes) {
        return launch_novel_runs(st, *pan, sq->d_desc, d_chunks.get(), nchunks, sq->d_seqw, sq->d_nmw, sq->d_has_n, counts, offs, n, words,
                                 words + n, bytes, bytes + n);
    };
    RunsOut out;  // the first min(runs, cap) runs in (contig, start) order: start, end and the two held flags
    out.nwords = out.nbytes = 2;
    out.cap = cap, out.prefix = true, out.contig = run_contig;
    out.words[0] = run_start, out.words[1] = run_end;
    out.bytes[0] = left_held, out.bytes[1] = right_held;
    std::vector<uint64_t> per(sq->n, 0);
    uint64_t sums[2] = {0, 0};  // the valid windows, the novel ones
    float ms[2] = {0, 0};
    const int r = runs_two_pass(t->ctx, fn, "contig", sq->n, w.first.data(), nchunks, launch, out, per.data(), nullptr, nruns, sums, ms);
    g_novel_ms[3] = ms[0] + ms[1];
    *windows = sums[0];
    *novel_windows = sums[1];
    return r;
}

// the link plane of `min_count` behind a pass of the scan: h = its NOVEL_SCAN_WORDS words (h[1]: the solid keys), block_solid the
// solid keys of every block.  Nothing is launched beyond the scan, and nothing kept, over a table without a solid key
int unitig_planes(pg_novel *nv, const char *fn, uint32_t min_count, uint64_t *h, std::vector<uint32_t> &block_solid) {
    const int k = nv->tbl->k;
    if (k < 2 || k > 32) return fail(PG_E_INVALID, "%s: a table of k = %d (unitigs: 2 to 32)", fn, k);
    float ms_scan = 0;
    if (int r = novel_scan_count(nv, fn, min_count, h, &block_solid, &ms_scan)) return r;
    if (h[1] != 0 && nv->ut.min_count == min_count) {  // (the planes kept: this handle's times go on adding up)
        std::copy(nv->ut.ms, nv->ut.ms + 3, g_unitig_ms);
        if (nv->ut.d_drop) {  // (cleaned: the surviving nodes are the graph)
            h[1] = nv->ut.nodes;
            block_solid = nv->ut.block_nodes;
        }
        return PG_OK;
    }
    g_unitig_ms[0] = g_unitig_ms[1] = g_unitig_ms[2] = 0;
    if (h[1] == 0) return PG_OK;
    unitig_drop(nv);
    hipStream_t st = nv->ctx->stream;
    const size_t bytes = (size_t)std::max<uint64_t>(nv->nslots, 4);  // (the marks are set through 32-bit words)
    DevBuf<uint8_t> links, marks;
    float ms_links = 0;
    LaunchTimer tm(&ms_links);
    hipError_t e = links.alloc(bytes);
    if (e == hipSuccess) e = marks.alloc(bytes);
    if (e == hipErrorOutOfMemory) {
        hipStreamSynchronize(st);
        return fail(PG_E_CAPACITY, "%s: no memory for two byte planes of %llu slots", fn, (unsigned long long)nv->nslots);
    }
    if (e == hipSuccess) e = hipMemsetAsync(marks.get(), 0, bytes, st);
    if (e == hipSuccess) e = tm.start(st);
    if (e == hipSuccess) e = launch_unitig_links(st, nv->d_keys, nv->d_depth, nv->nslots, nv->max_probe, min_count, k, links.get());
    if (e == hipSuccess) e = tm.stop(st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    tm.read();
    std::swap(nv->ut.d_links, links.p);
    std::swap(nv->ut.d_marks, marks.p);
    nv->ut.min_count = min_count;
    nv->ut.ms[0] = g_unitig_ms[0] = ms_links;
    return PG_OK;
}

int novel_links(pg_novel *nv, uint32_t min_count, uint64_t cap, uint64_t *keys_out, uint8_t *links_out, uint64_t *n) {
    const char *fn = "pg_novel_links";
    uint64_t h[NOVEL_SCAN_WORDS];
    std::vector<uint32_t> block_solid;
    if (int r = unitig_planes(nv, fn, min_count, h, block_solid)) return r;
    *n = h[1];
    const uint64_t take = std::min<uint64_t>(h[1], cap);
    if (take == 0) return PG_OK;
    std::vector<uint64_t> offs(block_solid.size());
    uint64_t sum = 0;
    for (size_t b = 0; b < block_solid.size(); ++b) {
        offs[b] = sum;
        sum += block_solid[b];
    }
    if (sum != h[1]) return fail(PG_E_HIP, "%s: %llu solid keys by block, %llu in all", fn, (unsigned long long)sum, (unsigned long long)h[1]);
    hipStream_t st = nv->ctx->stream;
    DevBuf<uint64_t> d_offs;
    DevBuf<unsigned long long> d_k;
    DevBuf<uint8_t> d_l;
    hipError_t e = d_offs.upload(offs, st);
    if (e == hipSuccess) e = d_k.alloc(take);
    if (e == hipSuccess) e = d_l.alloc(take);
    if (e == hipErrorOutOfMemory) {
        hipStreamSynchronize(st);
        return fail(PG_E_CAPACITY, "%s: no memory for %llu keys", fn, (unsigned long long)take);
    }
    if (e == hipSuccess)
        e = launch_unitig_links_emit(st, nv->d_keys, nv->d_depth, nv->ut.d_links, nv->nslots, min_count, d_offs.get(), take, d_k.get(), d_l.get(),
                                     nv->ut.d_drop);
    if (e == hipSuccess) e = hipMemcpyAsync(keys_out, d_k.get(), take * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(links_out, d_l.get(), take, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    return PG_OK;
}

// the rounds of pg_novel_clean: links, clean, a read of the counts; a last links pass behind the last round that dropped something.
// The handle keeps the three planes of the cleaned graph for `min_count`; max_rounds == 0 and a table without a solid key keep nothing
int novel_clean(pg_novel *nv, uint32_t min_count, uint32_t tip_kmers, uint32_t bubble_kmers, uint32_t ratio_milli, uint32_t max_rounds,
                uint64_t *stats) {
    const char *fn = "pg_novel_clean";
    const int k = nv->tbl->k;
    if (k < 2 || k > 32) return fail(PG_E_INVALID, "%s: a table of k = %d (unitigs: 2 to 32)", fn, k);
    if (tip_kmers < 1 || tip_kmers > UNITIG_CLEAN_MAX_KMERS || bubble_kmers < 1 || bubble_kmers > UNITIG_CLEAN_MAX_KMERS)
        return fail(PG_E_INVALID, "%s: tip_kmers = %u, bubble_kmers = %u (1 to %u)", fn, tip_kmers, bubble_kmers, UNITIG_CLEAN_MAX_KMERS);
    if (ratio_milli < 1 || ratio_milli > 999) return fail(PG_E_INVALID, "%s: ratio_milli = %u (1 to 999)", fn, ratio_milli);
    if (max_rounds > UNITIG_CLEAN_MAX_ROUNDS) return fail(PG_E_INVALID, "%s: max_rounds = %u (0 to %u)", fn, max_rounds, UNITIG_CLEAN_MAX_ROUNDS);
    uint64_t h[NOVEL_SCAN_WORDS];
    std::vector<uint32_t> block_solid;
    float ms_scan = 0;
    if (int r = novel_scan_count(nv, fn, min_count, h, &block_solid, &ms_scan)) return r;
    std::fill(stats, stats + 5, 0);
    g_clean_ms[0] = g_clean_ms[1] = 0;
    unitig_drop(nv);  // (the raw graph's planes are built again by whoever asks next)
    if (h[1] == 0 || max_rounds == 0) return PG_OK;
    hipStream_t st = nv->ctx->stream;
    const uint32_t blocks = novel_scan_blocks(nv->nslots);
    const size_t bytes = (size_t)std::max<uint64_t>(nv->nslots, 4);  // (marks and drop bytes are set through 32-bit words)
    DevBuf<uint8_t> links, marks, drop;
    DevBuf<uint32_t> d_nodes, d_flag;
    DevBuf<uint64_t> d_counts;
    hipError_t e = links.alloc(bytes);
    if (e == hipSuccess) e = marks.alloc(bytes);
    if (e == hipSuccess) e = drop.alloc(bytes);
    if (e == hipSuccess) e = d_nodes.alloc(blocks);
    if (e == hipSuccess) e = d_counts.alloc((size_t)blocks * 4);
    if (e == hipSuccess) e = d_flag.alloc(1);
    if (e == hipErrorOutOfMemory) {
        hipStreamSynchronize(st);
        return fail(PG_E_CAPACITY, "%s: no memory for three byte planes of %llu slots", fn, (unsigned long long)nv->nslots);
    }
    if (e == hipSuccess) e = hipMemsetAsync(marks.get(), 0, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(drop.get(), 0, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag.get(), 0, 4, st);
    std::vector<uint32_t> block_nodes(blocks);
    std::vector<uint64_t> counts((size_t)blocks * 4);
    uint32_t flag = 0;
    for (uint32_t round = 0; e == hipSuccess; ++round) {
        float ms_links = 0, ms_clean = 0;
        LaunchTimer tl(&ms_links), tc(&ms_clean);
        const bool last = round == max_rounds;
        e = tl.start(st);
        if (e == hipSuccess)
            e = launch_unitig_links(st, nv->d_keys, nv->d_depth, nv->nslots, nv->max_probe, min_count, k, links.get(), drop.get(), d_nodes.get());
        if (e == hipSuccess) e = tl.stop(st);
        if (e == hipSuccess && !last) {
            e = tc.start(st);
            if (e == hipSuccess)
                e = launch_unitig_clean(st, nv->d_keys, nv->d_depth, nv->nslots, nv->max_probe, min_count, k, links.get(), drop.get(), tip_kmers,
                                        bubble_kmers, ratio_milli, d_counts.get(), d_flag.get());
            if (e == hipSuccess) e = tc.stop(st);
            if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d_counts.get(), counts.size() * 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag.get(), 4, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(block_nodes.data(), d_nodes.get(), (size_t)blocks * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        tl.read();
        g_clean_ms[0] += ms_links;
        if (last) break;
        tc.read();
        g_clean_ms[1] += ms_clean;
        if (flag) return fail(PG_E_INTERNAL, "%s: the link plane contradicts the table in round %u", fn, round + 1);
        uint64_t got[4] = {0, 0, 0, 0};
        for (uint32_t b = 0; b < blocks; ++b)
            for (int i = 0; i < 4; ++i) got[i] += counts[(size_t)b * 4 + i];
        if (got[0] + got[2] == 0) break;  // (nothing dropped: the link plane is the final graph's)
        for (int i = 0; i < 4; ++i) stats[i] += got[i];
        ++stats[4];
    }
    if (e != hipSuccess) {
        hipStreamSynchronize(st);
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    uint64_t nodes = 0;
    for (uint32_t n : block_nodes) nodes += n;
    if (nodes + stats[1] + stats[3] != h[1])
        return fail(PG_E_INTERNAL, "%s: %llu nodes left and %llu dropped of %llu solid keys", fn, (unsigned long long)nodes,
                    (unsigned long long)(stats[1] + stats[3]), (unsigned long long)h[1]);
    std::swap(nv->ut.d_links, links.p);
    std::swap(nv->ut.d_marks, marks.p);
    std::swap(nv->ut.d_drop, drop.p);
    nv->ut.min_count = min_count;
    nv->ut.nodes = nodes;
    nv->ut.block_nodes = block_nodes;
    nv->ut.ms[0] = g_clean_ms[0];
    return PG_OK;
}

// where a round's unitigs go: on the device, cut at the caller's capacities
struct UnitigOut {
    uint64_t cap_u = 0, cap_b = 0;
    DevBuf<uint64_t> offsets, depth_sum;
    DevBuf<uint32_t> kmers;
    DevBuf<uint8_t> circular, bases;
};

// one pass of k_unitig_walk over the table.  Count (offs == NULL): counts = {winners, their nodes} per block.  Emit: offs = {unitigs,
// bases} in front of every block's, out (NULL: the marks only) takes them.  which: the handle's time (1 linear, 2 circular) the pass's is added to
int unitig_pass(pg_novel *nv, const char *fn, bool circular, uint64_t bound, std::vector<ulonglong2> *counts, const std::vector<ulonglong2> *offs,
                UnitigOut *out, int which) {
    hipStream_t st = nv->ctx->stream;
    const uint32_t blocks = novel_scan_blocks(nv->nslots);
    DevBuf<ulonglong2> d_counts, d_offs;
    DevBuf<uint32_t> d_flag;
    uint32_t flag = 0;
    float t = 0;
    LaunchTimer tm(&t);
    hipError_t e = d_flag.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag.get(), 0, 4, st);
    if (e == hipSuccess) e = offs ? d_offs.upload(*offs, st) : d_counts.alloc(blocks);
    if (e == hipSuccess) e = tm.start(st);
    if (e == hipSuccess)
        e = launch_unitig_walk(st, nv->d_keys, nv->d_depth, nv->nslots, nv->max_probe, nv->ut.min_count, nv->tbl->k, nv->ut.d_links, nv->ut.d_marks,
                               circular, bound, d_counts.get(), d_offs.get(), out ? out->cap_u : 0, out ? out->cap_b : 0,
                               out ? out->offsets.get() : nullptr, out ? out->kmers.get() : nullptr, out ? out->depth_sum.get() : nullptr,
                               out ? out->circular.get() : nullptr, out ? out->bases.get() : nullptr, d_flag.get(), nv->ut.d_drop);
    if (e == hipSuccess) e = tm.stop(st);
    if (e == hipSuccess && counts) {
        counts->assign(blocks, make_ulonglong2(0, 0));
        e = hipMemcpyAsync(counts->data(), d_counts.get(), (size_t)blocks * sizeof(ulonglong2), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag.get(), 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);  // (the upload's source and the copies' targets go with this scope)
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    tm.read();
    nv->ut.ms[which] += t;
    g_unitig_ms[which] = nv->ut.ms[which];
    if (flag)
        return fail(PG_E_INTERNAL, "%s: a walk of the %s round did not end within %llu nodes, or the link plane contradicts the table", fn,
                    circular ? "circular" : "linear", (unsigned long long)bound);
    return PG_OK;
}

// {unitigs, bases} in front of every block's, from {u0, b0} on; a unitig of n nodes holds n + k - 1 bases
std::vector<ulonglong2> unitig_offsets(const std::vector<ulonglong2> &counts, int k, uint64_t u0, uint64_t b0) {
    std::vector<ulonglong2> offs(counts.size());
    for (size_t b = 0; b < counts.size(); ++b) {
        offs[b] = make_ulonglong2(u0, b0);
        u0 += counts[b].x;
        b0 += counts[b].y + (uint64_t)(k - 1) * counts[b].x;
    }
    return offs;
}

int novel_unitigs(pg_novel *nv, uint32_t min_count, uint64_t cap_u, uint64_t cap_b, uint64_t *offsets, uint32_t *kmers, uint64_t *depth_sum,
                  uint8_t *circular, uint8_t *bases, uint64_t *nunitigs, uint64_t *nbases, uint64_t *ncircular) {
    const char *fn = "pg_novel_unitigs";
    uint64_t h[NOVEL_SCAN_WORDS];
    std::vector<uint32_t> block_solid;
    if (int r = unitig_planes(nv, fn, min_count, h, block_solid)) return r;
    *nunitigs = *nbases = *ncircular = 0;
    const uint64_t solid = h[1];
    if (solid == 0) return PG_OK;
    pg_novel::Unitigs &u = nv->ut;
    const int k = nv->tbl->k;
    if (!u.walked) {
        // the linear round counted; when its winners' nodes are fewer than the solid keys, its emit pass for the marks alone and the
        // circular round counted over the nodes without one
        if (int r = unitig_pass(nv, fn, false, solid, &u.lin, nullptr, nullptr, 1)) return r;
        u.nlin = u.lin_nodes = u.ncirc = u.circ_nodes = 0;
        for (const ulonglong2 &c : u.lin) {
            u.nlin += c.x;
            u.lin_nodes += c.y;
        }
        if (u.lin_nodes > solid)
            return fail(PG_E_INTERNAL, "%s: the linear unitigs hold %llu nodes of %llu", fn, (unsigned long long)u.lin_nodes, (unsigned long long)solid);
        u.circ.clear();
        if (u.lin_nodes < solid) {
            const std::vector<ulonglong2> offs = unitig_offsets(u.lin, k, 0, 0);
            if (int r = unitig_pass(nv, fn, false, solid, nullptr, &offs, nullptr, 1)) return r;
            if (int r = unitig_pass(nv, fn, true, solid - u.lin_nodes, &u.circ, nullptr, nullptr, 2)) return r;
            for (const ulonglong2 &c : u.circ) {
                u.ncirc += c.x;
                u.circ_nodes += c.y;
            }
            if (u.lin_nodes + u.circ_nodes != solid)
                return fail(PG_E_INTERNAL, "%s: %llu nodes in linear and %llu in circular unitigs, %llu solid keys", fn,
                            (unsigned long long)u.lin_nodes, (unsigned long long)u.circ_nodes, (unsigned long long)solid);
        }
        u.walked = true;
    } else if (u.lin_nodes + u.circ_nodes != solid) {
        return fail(PG_E_INTERNAL, "%s: the counts kept speak of %llu nodes, the table holds %llu solid keys", fn,
                    (unsigned long long)(u.lin_nodes + u.circ_nodes), (unsigned long long)solid);
    }
    const uint64_t lin_bases = u.lin_nodes + (uint64_t)(k - 1) * u.nlin;
    *nunitigs = u.nlin + u.ncirc;
    *nbases = lin_bases + u.circ_nodes + (uint64_t)(k - 1) * u.ncirc;
    *ncircular = u.ncirc;
    UnitigOut out;
    out.cap_u = std::min<uint64_t>(cap_u, *nunitigs);
    out.cap_b = std::min<uint64_t>(cap_b, *nbases);
    if (out.cap_u == 0 && out.cap_b == 0) return PG_OK;
    hipStream_t st = nv->ctx->stream;
    hipError_t e = hipSuccess;
    if (out.cap_u) {
        e = out.offsets.alloc(out.cap_u);
        if (e == hipSuccess) e = out.depth_sum.alloc(out.cap_u);
        if (e == hipSuccess) e = out.kmers.alloc(out.cap_u);
        if (e == hipSuccess) e = out.circular.alloc(out.cap_u);
    }
    if (e == hipSuccess && out.cap_b) e = out.bases.alloc(out.cap_b);
    if (e == hipErrorOutOfMemory)
        return fail(PG_E_CAPACITY, "%s: no memory for %llu unitigs of %llu bases", fn, (unsigned long long)out.cap_u, (unsigned long long)out.cap_b);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    if (u.nlin) {
        const std::vector<ulonglong2> offs = unitig_offsets(u.lin, k, 0, 0);
        if (int r = unitig_pass(nv, fn, false, solid, nullptr, &offs, &out, 1)) return r;
    }
    if (u.ncirc && (out.cap_u > u.nlin || out.cap_b > lin_bases)) {  // (the circular ones stand behind the linear ones)
        const std::vector<ulonglong2> offs = unitig_offsets(u.circ, k, u.nlin, lin_bases);
        if (int r = unitig_pass(nv, fn, true, solid - u.lin_nodes, nullptr, &offs, &out, 2)) return r;
    }
    if (out.cap_u) {
        e = hipMemcpyAsync(offsets, out.offsets.get(), out.cap_u * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(depth_sum, out.depth_sum.get(), out.cap_u * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(kmers, out.kmers.get(), out.cap_u * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(circular, out.circular.get(), out.cap_u, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && out.cap_b) e = hipMemcpyAsync(bases, out.bases.get(), out.cap_b, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    return PG_OK;
}

}  // namespace

extern "C" int pg_novel_create(pg_table *tbl, uint64_t capacity_keys, pg_novel **out) {
    PG_API_BEGIN
    if (!tbl || !out) return fail(PG_E_INVALID, "pg_novel_create: NULL argument");
    return novel_create(tbl, capacity_keys, out);
    PG_API_END
}

extern "C" int pg_novel_destroy(pg_novel *nv) {
    PG_API_BEGIN
    if (nv) novel_free(nv);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_novel_clear(pg_novel *nv) {
    PG_API_BEGIN
    if (!nv) return fail(PG_E_INVALID, "pg_novel_clear: NULL argument");
    if (int r = use_device(nv->ctx)) return r;
    HIP_TRY(hipMemsetAsync(nv->d_keys, 0xFF, nv->nslots * 8, nv->ctx->stream));
    HIP_TRY(hipMemsetAsync(nv->d_depth, 0, nv->nslots * 4, nv->ctx->stream));
    HIP_TRY(hipStreamSynchronize(nv->ctx->stream));
    unitig_drop(nv);
    nv->nkeys = nv->windows = 0;
    nv->overflowed = false;  // (nothing short is left)
    return PG_OK;
    PG_API_END
}

extern "C" int pg_novel_add_seqset(pg_novel *nv, const pg_seqset *seqs, uint64_t *windows, uint64_t *hits, uint64_t *new_keys) {
    PG_API_BEGIN
    if (!nv || !seqs || !windows || !hits || !new_keys) return fail(PG_E_INVALID, "pg_novel_add_seqset: NULL argument");
    return novel_add(nv, seqs, windows, hits, new_keys);
    PG_API_END
}

extern "C" int pg_novel_stats(pg_novel *nv, uint64_t *nkeys, uint64_t *nslots, uint64_t *grown) {
    PG_API_BEGIN
    if (!nv) return fail(PG_E_INVALID, "pg_novel_stats: NULL argument");
    if (nkeys) *nkeys = nv->nkeys;
    if (nslots) *nslots = nv->nslots;
    if (grown) *grown = nv->grown;
    return PG_OK;
    PG_API_END
}

extern "C" int pg_novel_result(pg_novel *nv, uint32_t min_count, uint64_t *nkeys, uint64_t *solid, uint64_t *solid_windows, uint64_t *depth_hist) {
    PG_API_BEGIN
    if (!nv) return fail(PG_E_INVALID, "pg_novel_result: NULL argument");
    return novel_result(nv, min_count, nkeys, solid, solid_windows, depth_hist);
    PG_API_END
}

extern "C" int pg_novel_keys(pg_novel *nv, uint32_t min_count, uint64_t cap, uint64_t *keys, uint32_t *depths, uint64_t *n) {
    PG_API_BEGIN
    if (!nv || !n || (cap && (!keys || !depths))) return fail(PG_E_INVALID, "pg_novel_keys: NULL argument");
    return novel_keys(nv, min_count, cap, keys, depths, n);
    PG_API_END
}

extern "C" int pg_novel_runs(pg_table *tbl, const pg_seqset *seqs, uint64_t cap, uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end,
                             uint8_t *left_held, uint8_t *right_held, uint64_t *nruns, uint64_t *windows, uint64_t *novel_windows) {
    PG_API_BEGIN
    if (!tbl || !seqs || !nruns || !windows || !novel_windows || (cap && (!run_contig || !run_start || !run_end || !left_held || !right_held)))
        return fail(PG_E_INVALID, "pg_novel_runs: NULL argument");
    return novel_runs(tbl, seqs, cap, run_contig, run_start, run_end, left_held, right_held, nruns, windows, novel_windows);
    PG_API_END
}

extern "C" int pg_novel_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_novel_last_timing: NULL argument");
    std::copy(g_novel_ms, g_novel_ms + 4, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_novel_links(pg_novel *nv, uint32_t min_count, uint64_t cap, uint64_t *keys, uint8_t *links, uint64_t *n) {
    PG_API_BEGIN
    if (!nv || !n || (cap && (!keys || !links))) return fail(PG_E_INVALID, "pg_novel_links: NULL argument");
    return novel_links(nv, min_count, cap, keys, links, n);
    PG_API_END
}

extern "C" int pg_novel_unitigs(pg_novel *nv, uint32_t min_count, uint64_t cap_unitigs, uint64_t cap_bases, uint64_t *offsets, uint32_t *kmers,
                                uint64_t *depth_sum, uint8_t *circular, uint8_t *bases, uint64_t *nunitigs, uint64_t *nbases, uint64_t *ncircular) {
    PG_API_BEGIN
    if (!nv || !nunitigs || !nbases || !ncircular || (cap_unitigs && (!offsets || !kmers || !depth_sum || !circular)) || (cap_bases && !bases))
        return fail(PG_E_INVALID, "pg_novel_unitigs: NULL argument");
    return novel_unitigs(nv, min_count, cap_unitigs, cap_bases, offsets, kmers, depth_sum, circular, bases, nunitigs, nbases, ncircular);
    PG_API_END
}

extern "C" int pg_novel_clean(pg_novel *nv, uint32_t min_count, uint32_t tip_kmers, uint32_t bubble_kmers, uint32_t ratio_milli, uint32_t max_rounds,
                              uint64_t *stats) {
    PG_API_BEGIN
    if (!nv || !stats) return fail(PG_E_INVALID, "pg_novel_clean: NULL argument");
    return novel_clean(nv, min_count, tip_kmers, bubble_kmers, ratio_milli, max_rounds, stats);
    PG_API_END
}

extern "C" int pg_novel_clean_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_novel_clean_last_timing: NULL argument");
    std::copy(g_clean_ms, g_clean_ms + 2, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_novel_unitigs_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_novel_unitigs_last_timing: NULL argument");
    std::copy(g_unitig_ms, g_unitig_ms + 3, ms_out);
    return PG_OK;
    PG_API_END
}
