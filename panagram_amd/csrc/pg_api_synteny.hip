// pg_api_synteny.hip — host side of the C-ABI: the position table of two genomes, the mates of A's positions and their collinear
// runs (pg_synteny.hip), the runs chained into blocks (pg_blocks.hip, pg_blocks_host.h), the blocks' links as variants of B
// against A (pg_variants.hip), and the hit runs and loci of queries in a streamed genome (pg_locate.hip).
#include "pg_host.h"

#include "pg_blocks_host.h"
#include "pg_keytable_host.h"
#include "pg_runs_host.h"  // RunsOut, runs_two_pass

static constexpr uint64_t POS_MAX_BASES = 0x7FFFFFFFull;  // a side's bases: the word pos << 1 | rc stays below POS_MULTI
static constexpr uint64_t POS_MAX_KEYS = 1ull << 32;      // two sides of 2^31 k-mers

struct pg_postable {
    pg_ctx *ctx;
    int k;
    uint64_t capacity, nslots;
    uint32_t max_probe;
    void *d_slots = nullptr;
    uint32_t *d_mates = nullptr;  // of the last pg_postable_mates: kept in HBM for the runs
    uint64_t nmates = 0;
    bool inserted[2] = {false, false};
    uint64_t side_bases[2] = {0, 0};  // of the sequence set inserted as each side, and its contigs: pg_postable_locate's seqsQ is
    uint32_t side_contigs[2] = {0, 0};  // held against them
    bool overflowed = false;  // an insert gave up: the table holds a part of a side and answers nothing any more
};

namespace {

thread_local float g_last_ms[5] = {0, 0, 0, 0, 0};  // insert A, insert B, mates, runs (count), runs (emit) of the last pg_synteny_segments
thread_local float g_blocks_ms[7] = {0, 0, 0, 0, 0, 0, 0};  // those five, blocks (count), blocks (emit) of the last pg_synteny_blocks
thread_local float g_locate_ms[4] = {0, 0, 0, 0};  // k_hit_runs (count), (emit), k_run_blocks (count), (emit) of the last hit call
thread_local float g_variants_ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // those seven, variants (count), variants (emit) of the last pg_synteny_variants

// the (contig, chunk) jobs of a side's k-mer positions (walk_kmers), held to the side's limit: behind it the base offsets and
// the k-mer offsets of the contigs fit 32 bits
int walk_side(const pg_seqset *sq, int k, const char *fn, KmerWalk &w) {
    if (int r = walk_kmers(sq, k, SYNTENY_JOB, fn, w)) return r;
    if (w.bases > POS_MAX_BASES)
        return fail(PG_E_INVALID, "%s: more than %llu bases in one side (take fewer chromosomes)", fn, (unsigned long long)POS_MAX_BASES);
    return PG_OK;
}

int postable_create(pg_ctx *ctx, int k, uint64_t capacity, std::unique_ptr<pg_postable> &out) {
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "pg_postable_create: k=%d unsupported (1..32)", k);
    if (capacity < 1 || capacity > POS_MAX_KEYS)
        return fail(PG_E_INVALID, "pg_postable_create: capacity of %llu keys (1 to 2^32)", (unsigned long long)capacity);
    if (int r = use_device(ctx)) return r;
    std::unique_ptr<pg_postable> pt(new pg_postable);
    pt->ctx = ctx;
    pt->k = k;
    pt->capacity = capacity;
    pt->nslots = table_slots(capacity);
    pt->max_probe = table_max_probe(pt->nslots);
    hipError_t e = hipMalloc(&pt->d_slots, pt->nslots * POS_SLOT_BYTES);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PG_E_CAPACITY : PG_E_HIP, "pg_postable_create: %llu slots: %s", (unsigned long long)pt->nslots,
                    hipGetErrorString(e));
    e = hipMemsetAsync(pt->d_slots, 0xFF, pt->nslots * POS_SLOT_BYTES, ctx->stream);
    if (e != hipSuccess) {
        hipFree(pt->d_slots);
        return fail(PG_E_HIP, "pg_postable_create: %s", hipGetErrorString(e));
    }
    ++ctx->refs;
    out = std::move(pt);
    return PG_OK;
}

void postable_free(pg_postable *pt) {
    hipSetDevice(pt->ctx->device);
    hipStreamSynchronize(pt->ctx->stream);
    if (pt->d_mates) hipFree(pt->d_mates);
    hipFree(pt->d_slots);
    pg_ctx *c = pt->ctx;
    delete pt;
    ctx_release(c);
}

int postable_insert(pg_postable *pt, int side, const pg_seqset *sq, float *ms = nullptr) {
    if (side < 0 || side > 1) return fail(PG_E_INVALID, "pg_postable_insert_seqset: side %d (0 or 1)", side);
    if (pt->ctx != sq->ctx) return fail(PG_E_INVALID, "pg_postable_insert_seqset: table and seqset belong to different contexts");
    if (pt->overflowed) return fail(PG_E_CAPACITY, "pg_postable_insert_seqset: the table overflowed before");
    if (pt->inserted[side]) return fail(PG_E_INVALID, "pg_postable_insert_seqset: side %d is inserted already", side);
    KmerWalk w;
    if (int r = walk_side(sq, pt->k, "pg_postable_insert_seqset", w)) return r;
    if (int r = use_device(pt->ctx)) return r;
    pt->inserted[side] = true;
    pt->side_bases[side] = w.bases;
    pt->side_contigs[side] = sq->n;
    if (w.jobs.empty()) return PG_OK;
    hipStream_t st = pt->ctx->stream;
    const std::vector<uint32_t> off(w.off.begin(), w.off.end());
    DevBuf<uint32_t> d_off;
    unsigned long long flags = 0;
    hipError_t e = d_off.upload(off, st);
    if (e == hipSuccess)
        e = counted_launch(st, w.jobs, &flags, 1, ms, [&](const uint2 *jobs, uint32_t njobs, unsigned long long *d_flags) {
            return launch_pos_insert(st, pt->k, (uint32_t)side, sq->d_desc, jobs, njobs, d_off.get(), sq->d_seqw, sq->d_nmw, sq->d_has_n,
                                     pt->d_slots, pt->nslots, pt->max_probe, d_flags);
        });
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_postable_insert_seqset: %s", hipGetErrorString(e));
    if (flags) {
        pt->overflowed = true;
        return fail(PG_E_CAPACITY, "pg_postable_insert_seqset: %llu slots (created for %llu keys) do not hold side %d's k-mers",
                    (unsigned long long)pt->nslots, (unsigned long long)pt->capacity, side);
    }
    return PG_OK;
}

// the mates of seqsA's positions into pt->d_mates; the host copy only when mates_out is given
int postable_mates(pg_postable *pt, const pg_seqset *sq, uint32_t *mates_out, uint64_t *nmated, float *ms = nullptr) {
    if (pt->ctx != sq->ctx) return fail(PG_E_INVALID, "pg_postable_mates: table and seqset belong to different contexts");
    if (pt->overflowed) return fail(PG_E_CAPACITY, "pg_postable_mates: the table overflowed");
    if (!pt->inserted[0]) return fail(PG_E_INVALID, "pg_postable_mates: side 0 has not been inserted");
    KmerWalk w;
    if (int r = walk_side(sq, pt->k, "pg_postable_mates", w)) return r;
    if (int r = use_device(pt->ctx)) return r;
    hipStream_t st = pt->ctx->stream;
    *nmated = 0;
    if (pt->d_mates) {
        HIP_TRY(hipStreamSynchronize(st));
        hipFree(pt->d_mates);
        pt->d_mates = nullptr;
        pt->nmates = 0;
    }
    if (w.jobs.empty()) return PG_OK;
    const std::vector<uint32_t> off(w.off.begin(), w.off.end()), koff(w.koff.begin(), w.koff.end());
    DevBuf<uint32_t> d_off, d_koff, d_m;
    unsigned long long n = 0;
    hipError_t e = d_off.upload(off, st);
    if (e == hipSuccess) e = d_koff.upload(koff, st);
    if (e == hipSuccess) e = d_m.alloc(w.nkmers);
    if (e == hipSuccess)
        e = counted_launch(st, w.jobs, &n, 1, ms, [&](const uint2 *jobs, uint32_t njobs, unsigned long long *d_n) {
            return launch_pos_mates(st, pt->k, sq->d_desc, jobs, njobs, d_off.get(), d_koff.get(), sq->d_seqw, sq->d_nmw, sq->d_has_n,
                                    pt->d_slots, pt->nslots, pt->max_probe, d_m.get(), d_n);
        });
    if (e == hipSuccess && mates_out) {
        e = hipMemcpyAsync(mates_out, d_m.get(), w.nkmers * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_postable_mates: %s", hipGetErrorString(e));
    pt->d_mates = d_m.p;
    d_m.p = nullptr;
    pt->nmates = w.nkmers;
    *nmated = n;
    return PG_OK;
}

// the runs of a mates array in HBM (ncontigs contigs of nkmers[c] entries, back to back); nruns[c] and *total_out always,
// *mated: the mated positions counted
int mate_runs_dev(pg_ctx *ctx, const char *fn, const uint32_t *d_mates, uint32_t ncontigs, const uint64_t *nkmers, const RunsOut &out,
                  uint64_t *nruns, uint64_t *total_out, uint64_t *mated, float *ms = nullptr) {
    std::vector<uint2> contigs(ncontigs), chunks;
    std::vector<uint64_t> first(ncontigs + 1, 0);
    uint64_t tot = 0;
    for (uint32_t c = 0; c < ncontigs; ++c) {
        if (nkmers[c] > POS_MAX_BASES || tot + nkmers[c] > POS_MAX_BASES)
            return fail(PG_E_INVALID, "%s: more than %llu positions", fn, (unsigned long long)POS_MAX_BASES);
        contigs[c] = make_uint2((uint32_t)tot, (uint32_t)nkmers[c]);
        first[c] = chunks.size();
        for (uint64_t p = 0; p < nkmers[c]; p += MATE_CHUNK) chunks.push_back(make_uint2(c, (uint32_t)p));
        tot += nkmers[c];
        nruns[c] = 0;
    }
    first[ncontigs] = chunks.size();
    *total_out = 0;
    if (mated) *mated = 0;
    if (chunks.empty()) return PG_OK;
    const uint32_t nchunks = (uint32_t)chunks.size();
    if (int r = use_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    DevBuf<uint2> d_contigs, d_chunks;
    hipError_t e = d_contigs.upload(contigs, st);
    if (e == hipSuccess) e = d_chunks.upload(chunks, st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);  // (the uploads' sources go with this scope)
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    const auto launch = [&](uint4 *counts, const ulonglong2 *offs, uint64_t n, uint32_t *words, uint8_t *) {
        return launch_mate_runs(st, d_mates, d_contigs.get(), d_chunks.get(), nchunks, counts, offs, n, words, words + n, words + 2 * n);
    };
    uint64_t sums[2] = {0, 0};  // the mated positions, nothing
    const int r = runs_two_pass(ctx, fn, "contig", ncontigs, first.data(), nchunks, launch, out, nruns, nullptr, total_out, sums, ms);
    if (mated) *mated = sums[0];
    return r;
}

// the caller's four host arrays of `cap` entries, under the all-or-nothing capacity protocol
RunsOut host_runs(uint64_t cap, uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint32_t *run_word) {
    RunsOut out;
    out.cap = cap, out.contig = run_contig;
    out.words[0] = run_start, out.words[1] = run_end, out.words[2] = run_word;
    return out;
}

bool runs_args_ok(uint32_t ncontigs, uint64_t cap, const uint32_t *run_contig, const uint32_t *run_start, const uint32_t *run_end,
                  const uint32_t *run_mate, const uint64_t *nruns, const uint64_t *total) {
    return total && (!ncontigs || nruns) && (!cap || (run_contig && run_start && run_end && run_mate));
}

struct BlockParams {
    uint32_t min_run, max_gap, max_shift;
};
struct BlockArrays {  // the caller's eight arrays of `cap` entries
    uint32_t *contig, *start, *end, *mate_first, *mate_last, *kmers, *runs, *shifted;
    bool all() const { return contig && start && end && mate_first && mate_last && kmers && runs && shifted; }
};

int block_params_ok(const char *fn, const BlockParams &p) {
    if (p.min_run < 1) return fail(PG_E_INVALID, "%s: min_run must be at least 1", fn);
    if (p.max_gap < 1 || p.max_gap > BLOCKS_MAX_GAP) return fail(PG_E_INVALID, "%s: max_gap=%u (1 to 2^31 - 1)", fn, p.max_gap);
    if (p.max_shift > BLOCKS_MAX_GAP) return fail(PG_E_INVALID, "%s: max_shift=%u (at most 2^31 - 1)", fn, p.max_shift);
    return PG_OK;
}

// what the blocks' count pass and the stitch leave for the passes behind them: the chunk geometry on both sides of the bus and
// the stitched offsets (the carried predecessor of every chunk among them)
struct BlocksPlan {
    std::vector<uint2> contigs, chunks;
    std::vector<uint64_t> first;
    std::vector<BlockChunkOffs> offs;
    DevBuf<uint2> d_contigs, d_chunks;
    DevBuf<uint64_t> d_boff;
    uint32_t nchunks = 0, nb = 0;
    uint64_t total = 0;
};

// the count half of the blocks of run arrays in HBM (three planes of nruns words: start, end, mate; per_contig[c] runs of contig
// c of A, back to back); boff: the nb + 1 offsets of B's contigs.  nblocks[c], *total_out and the plan; ms: the count launch.
int blocks_count_dev(pg_ctx *ctx, const char *fn, const uint32_t *d_runs, uint64_t nruns, uint32_t ncontigs, const uint64_t *per_contig,
                     const std::vector<uint64_t> &boff, const BlockParams &p, BlocksPlan &plan, uint64_t *nblocks, uint64_t *total_out,
                     float *ms = nullptr) {
    std::vector<uint2> &contigs = plan.contigs, &chunks = plan.chunks;
    std::vector<uint64_t> &first = plan.first;
    contigs.assign(ncontigs, make_uint2(0, 0));
    chunks.clear();
    first.assign(ncontigs + 1, 0);
    uint64_t at = 0;
    for (uint32_t c = 0; c < ncontigs; ++c) {
        contigs[c] = make_uint2((uint32_t)at, (uint32_t)per_contig[c]);
        first[c] = chunks.size();
        for (uint64_t r = 0; r < per_contig[c]; r += RUN_CHUNK) chunks.push_back(make_uint2(c, (uint32_t)r));
        at += per_contig[c];
        nblocks[c] = 0;
    }
    first[ncontigs] = chunks.size();
    *total_out = 0;
    plan.nchunks = 0;
    plan.total = 0;
    if (at != nruns) return fail(PG_E_INVALID, "%s: the contigs hold %llu runs of %llu", fn, (unsigned long long)at, (unsigned long long)nruns);
    if (chunks.empty()) return PG_OK;
    const uint32_t nchunks = (uint32_t)chunks.size(), nb = (uint32_t)boff.size();
    if (int r = use_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    DevBuf<BlockChunkCount> d_counts;
    std::vector<BlockChunkCount> counts(nchunks);
    LaunchTimer tc(ms);
    const uint32_t *rs = d_runs, *re = d_runs + nruns, *rm = d_runs + 2 * nruns;
    hipError_t e = plan.d_contigs.upload(contigs, st);
    if (e == hipSuccess) e = plan.d_chunks.upload(chunks, st);
    if (e == hipSuccess) e = plan.d_boff.upload(boff, st);
    if (e == hipSuccess) e = d_counts.alloc(nchunks);
    if (e == hipSuccess) e = tc.start(st);
    if (e == hipSuccess)
        e = launch_run_blocks(st, rs, re, rm, plan.d_contigs.get(), plan.d_chunks.get(), nchunks, plan.d_boff.get(), nb, p.min_run,
                              p.max_gap, p.max_shift, d_counts.get(), nullptr, 0, nullptr);
    if (e == hipSuccess) e = tc.stop(st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(counts.data(), d_counts.get(), (size_t)nchunks * sizeof(BlockChunkCount), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    tc.read();
    plan.offs.resize(nchunks);
    const uint64_t total = blocks_stitch(ncontigs, first.data(), counts.data(), p.max_gap, p.max_shift, boff.data(), nb, plan.offs.data(), nblocks);
    if (total == ~0ull) return fail(PG_E_HIP, "%s: a contig's block starts and ends differ in number", fn);
    *total_out = total;
    plan.nchunks = nchunks;
    plan.nb = nb;
    plan.total = total;
    return PG_OK;
}

// the emit half: the plan's blocks under the capacity protocol; ms: the emit launch
int blocks_emit_dev(pg_ctx *ctx, const char *fn, const uint32_t *d_runs, uint64_t nruns, uint32_t ncontigs, const BlockParams &p,
                    const BlocksPlan &plan, uint64_t cap, const BlockArrays &out, const uint64_t *nblocks, float *ms = nullptr) {
    const uint64_t total = plan.total;
    if (total == 0 || cap == 0 || total > cap) return PG_OK;  // (nothing to emit / the caller's arrays are too short)
    hipStream_t st = ctx->stream;
    const uint32_t *rs = d_runs, *re = d_runs + nruns, *rm = d_runs + 2 * nruns;
    LaunchTimer te(ms);
    DevBuf<BlockChunkOffs> d_offs;
    DevBuf<uint32_t> d_out;
    std::vector<uint32_t> rec((size_t)10 * total);
    hipError_t e = d_offs.upload(plan.offs, st);
    if (e == hipSuccess) e = d_out.alloc((size_t)10 * total);
    if (e == hipSuccess) e = te.start(st);
    if (e == hipSuccess)
        e = launch_run_blocks(st, rs, re, rm, plan.d_contigs.get(), plan.d_chunks.get(), plan.nchunks, plan.d_boff.get(), plan.nb,
                              p.min_run, p.max_gap, p.max_shift, nullptr, d_offs.get(), total, d_out.get());
    if (e == hipSuccess) e = te.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(rec.data(), d_out.get(), rec.size() * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    te.read();
    // a block's sums: its end record less its start record
    const uint32_t *sr = rec.data(), *er = rec.data() + 5 * total;
    for (uint64_t i = 0; i < total; ++i) {
        out.start[i] = sr[i];
        out.mate_first[i] = sr[total + i];
        out.end[i] = er[i];
        out.mate_last[i] = er[total + i];
        out.kmers[i] = er[2 * total + i] - sr[2 * total + i];
        out.runs[i] = er[3 * total + i] - sr[3 * total + i];
        out.shifted[i] = er[4 * total + i] - sr[4 * total + i];
    }
    uint64_t at = 0;
    for (uint32_t c = 0; c < ncontigs; ++c)
        for (uint64_t i = 0; i < nblocks[c]; ++i) out.contig[at++] = c;
    return PG_OK;
}

// the blocks of run arrays in HBM: counts always, the blocks under the capacity protocol
int run_blocks_dev(pg_ctx *ctx, const char *fn, const uint32_t *d_runs, uint64_t nruns, uint32_t ncontigs, const uint64_t *per_contig,
                   const std::vector<uint64_t> &boff, const BlockParams &p, uint64_t cap, const BlockArrays &out, uint64_t *nblocks,
                   uint64_t *total_out, float *ms = nullptr) {
    BlocksPlan plan;
    if (int r = blocks_count_dev(ctx, fn, d_runs, nruns, ncontigs, per_contig, boff, p, plan, nblocks, total_out, ms)) return r;
    return blocks_emit_dev(ctx, fn, d_runs, nruns, ncontigs, p, plan, cap, out, nblocks, ms ? ms + 1 : nullptr);
}

struct VariantArrays {  // the caller's nine arrays of `cap` entries
    uint32_t *contig, *posA, *lenA, *posB, *lenB, *info, *mismatches;
    uint64_t *alleleA, *alleleB;
    bool all() const { return contig && posA && lenA && posB && lenB && info && mismatches && alleleA && alleleB; }
};

// the links of a plan's blocks as variants (pg_variants.hip): class_counts[6], *links and *total always, the records under the
// capacity protocol; ms[0] the count launch, ms[1] the emit launch
int link_variants_dev(pg_ctx *ctx, const char *fn, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, const uint32_t *d_runs,
                      uint64_t nruns, const BlockParams &p, const BlocksPlan &plan, uint64_t cap, const VariantArrays &out,
                      uint64_t *class_counts, uint64_t *links, uint64_t *total_out, float *ms = nullptr) {
    std::fill(class_counts, class_counts + 6, 0ull);
    *links = *total_out = 0;
    const uint32_t nchunks = plan.nchunks;
    if (nchunks == 0) return PG_OK;
    hipStream_t st = ctx->stream;
    const uint32_t *rs = d_runs, *re = d_runs + nruns, *rm = d_runs + 2 * nruns;
    DevBuf<BlockChunkOffs> d_offs;
    DevBuf<VariantChunkCount> d_counts;
    std::vector<VariantChunkCount> counts(nchunks);
    LaunchTimer tc(ms), te(ms ? ms + 1 : nullptr);
    hipError_t e = d_offs.upload(plan.offs, st);
    if (e == hipSuccess) e = d_counts.alloc(nchunks);
    if (e == hipSuccess) e = tc.start(st);
    if (e == hipSuccess)
        e = launch_link_variants(st, rs, re, rm, plan.d_contigs.get(), plan.d_chunks.get(), nchunks, plan.d_boff.get(), plan.nb,
                                 (uint32_t)k, p.min_run, p.max_gap, p.max_shift, d_offs.get(), seqsA->d_desc, seqsA->d_seqw, seqsA->d_nmw,
                                 seqsB->d_desc, seqsB->n, seqsB->d_seqw, seqsB->d_nmw, d_counts.get(), nullptr, 0, nullptr, nullptr);
    if (e == hipSuccess) e = tc.stop(st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(counts.data(), d_counts.get(), (size_t)nchunks * sizeof(VariantChunkCount), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    tc.read();
    // the exclusive scan of the chunks' records
    std::vector<uint64_t> voffs(nchunks);
    uint64_t total = 0;
    for (uint32_t i = 0; i < nchunks; ++i) {
        voffs[i] = total;
        total += counts[i].records;
        for (int c = 0; c < 6; ++c) class_counts[c] += counts[i].cls[c];
    }
    for (int c = 0; c < 6; ++c) *links += class_counts[c];
    *total_out = total;
    if (total != *links - class_counts[0]) return fail(PG_E_HIP, "%s: %llu records of %llu links that differ", fn, (unsigned long long)total,
                                                        (unsigned long long)(*links - class_counts[0]));
    if (total == 0 || cap == 0 || total > cap) return PG_OK;  // (nothing to emit / the caller's arrays are too short)
    DevBuf<uint64_t> d_voffs, d_out;  // (8 planes: the two of 64-bit words first, then the six of 32-bit words)
    std::vector<uint64_t> rec((size_t)5 * total);
    e = d_voffs.upload(voffs, st);
    if (e == hipSuccess) e = d_out.alloc((size_t)5 * total);
    if (e == hipSuccess) e = te.start(st);
    if (e == hipSuccess)
        e = launch_link_variants(st, rs, re, rm, plan.d_contigs.get(), plan.d_chunks.get(), nchunks, plan.d_boff.get(), plan.nb,
                                 (uint32_t)k, p.min_run, p.max_gap, p.max_shift, d_offs.get(), seqsA->d_desc, seqsA->d_seqw, seqsA->d_nmw,
                                 seqsB->d_desc, seqsB->n, seqsB->d_seqw, seqsB->d_nmw, nullptr, d_voffs.get(), total,
                                 reinterpret_cast<uint32_t *>(d_out.get() + 2 * total), d_out.get());
    if (e == hipSuccess) e = te.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(rec.data(), d_out.get(), rec.size() * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    te.read();
    const uint32_t *w = reinterpret_cast<const uint32_t *>(rec.data() + 2 * total);
    std::copy(rec.data(), rec.data() + total, out.alleleA);
    std::copy(rec.data() + total, rec.data() + 2 * total, out.alleleB);
    std::copy(w, w + total, out.posA);
    std::copy(w + total, w + 2 * total, out.lenA);
    std::copy(w + 2 * total, w + 3 * total, out.posB);
    std::copy(w + 3 * total, w + 4 * total, out.lenB);
    std::copy(w + 4 * total, w + 5 * total, out.info);
    std::copy(w + 5 * total, w + 6 * total, out.mismatches);
    for (uint32_t i = 0; i < nchunks; ++i)  // (a chunk is of one contig of A)
        std::fill(out.contig + voffs[i], out.contig + voffs[i] + counts[i].records, plan.chunks[i].x);
    return PG_OK;
}

int variant_params_ok(const char *fn, const BlockParams &p) {
    if (int r = block_params_ok(fn, p)) return r;
    if (p.max_gap > VARIANTS_MAX_GAP) return fail(PG_E_INVALID, "%s: max_gap=%u (at most %u: a lane compares the gap's bases)", fn, p.max_gap, VARIANTS_MAX_GAP);
    return PG_OK;
}

// the offsets of B's contigs and B's positions; false when they pass 2^32 (no mate word reaches there)
bool contig_offsets(uint32_t n, const uint64_t *lens, std::vector<uint64_t> &boff) {
    boff.assign((size_t)n + 1, 0);
    for (uint32_t c = 0; c < n; ++c) {
        if (lens[c] > (1ull << 32) || boff[c] + lens[c] > (1ull << 32)) return false;
        boff[c + 1] = boff[c] + lens[c];
    }
    return true;
}

// a table of `capacity` keys with both sides inserted and the mates of A in its d_mates; freed with the scope
struct MatedTable {
    pg_postable *p = nullptr;
    ~MatedTable() {
        if (p) postable_free(p);
    }
};
int mated_table(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint64_t capacity, MatedTable &pt, uint64_t *nmated,
                float *ms) {
    std::unique_ptr<pg_postable> made;
    if (int r = postable_create(ctx, k, capacity, made)) return r;
    pt.p = made.release();
    if (int r = postable_insert(pt.p, 0, seqsA, ms)) return r;
    if (int r = postable_insert(pt.p, 1, seqsB, ms + 1)) return r;
    return postable_mates(pt.p, seqsA, nullptr, nmated, ms + 2);
}

// the run list of pg_run_blocks / pg_run_variants checked on the host: sorted, inside B; per[c] = the runs of contig c of A
int runs_ok(const char *fn, const uint32_t *run_contig, const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate,
                   uint64_t nruns, uint32_t ncontigsA, uint64_t sizeB, std::vector<uint64_t> &per) {
    per.assign(ncontigsA, 0);
    for (uint64_t i = 0; i < nruns; ++i) {
        const uint64_t c = run_contig[i], s = run_start[i], e = run_end[i], m = run_mate[i];
        if (c >= ncontigsA) return fail(PG_E_INVALID, "%s: run %llu: contig %llu of %u", fn, (unsigned long long)i, (unsigned long long)c, ncontigsA);
        if (e <= s) return fail(PG_E_INVALID, "%s: run %llu ends at or before its start", fn, (unsigned long long)i);
        if (m == NO_MATE) return fail(PG_E_INVALID, "%s: run %llu has no mate", fn, (unsigned long long)i);
        if (i && (run_contig[i - 1] > c || (run_contig[i - 1] == c && run_end[i - 1] > s)))
            return fail(PG_E_INVALID, "%s: run %llu: the runs are not sorted by (contig, start), or overlap", fn, (unsigned long long)i);
        const uint64_t b = m >> 1, n = e - s;
        if ((m & 1) ? (b < n - 1 || b >= sizeB) : b + (n - 1) >= sizeB)
            return fail(PG_E_INVALID, "%s: run %llu leaves genome B", fn, (unsigned long long)i);
        per[c] += 1;
    }
    return PG_OK;
}

static constexpr uint64_t HIT_MAX_CONTIG = 0xFFFFFFFFull;  // k-mer positions of one streamed contig: a run's exclusive end is a word

// what both hit calls check before anything is launched, and the chunks of the streamed set's k-mer positions: w.jobs[i] =
// {contig, first position}, the chunks of contig c being w.first[c] .. w.first[c + 1]
int hit_walk(const pg_postable *pt, const pg_seqset *sq, const char *fn, KmerWalk &w) {
    if (pt->ctx != sq->ctx) return fail(PG_E_INVALID, "%s: table and seqset belong to different contexts", fn);
    if (pt->overflowed) return fail(PG_E_CAPACITY, "%s: the table overflowed", fn);
    if (!pt->inserted[1]) return fail(PG_E_INVALID, "%s: side 1 (the queries) has not been inserted", fn);
    w.noun = "chunks";
    if (int r = walk_kmers(sq, pt->k, LOCATE_CHUNK, fn, w)) return r;
    for (uint32_t c = 0; c < sq->n; ++c)
        if ((c + 1 < sq->n ? w.koff[c + 1] : w.nkmers) - w.koff[c] > HIT_MAX_CONTIG)
            return fail(PG_E_INVALID, "%s: contig %u holds more than 2^32 - 1 k-mer positions", fn, c);
    for (uint2 &ck : w.jobs) ck.y *= LOCATE_CHUNK;  // (k_hit_runs takes a chunk's first position, below 2^32 behind the check above)
    return PG_OK;
}

// the hit runs of sq streamed through pt (k_hit_runs): nruns[c], hits[c] (when given), *total_out and *nhits always, the runs as
// mate_runs_dev leaves them; ms[0] the count launch, ms[1] the emit launch
int hit_runs_dev(pg_postable *pt, const char *fn, const pg_seqset *sq, const KmerWalk &w, const RunsOut &out, uint64_t *nruns,
                 uint64_t *hits, uint64_t *total_out, uint64_t *nhits, float *ms = nullptr) {
    for (uint32_t c = 0; c < sq->n; ++c) {
        nruns[c] = 0;
        if (hits) hits[c] = 0;
    }
    *total_out = *nhits = 0;
    if (w.jobs.empty()) return PG_OK;
    const uint32_t nchunks = (uint32_t)w.jobs.size();
    if (int r = use_device(pt->ctx)) return r;
    hipStream_t st = pt->ctx->stream;
    DevBuf<uint2> d_chunks;
    const hipError_t e = d_chunks.upload(w.jobs, st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);  // (the upload's source is the caller's)
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    const auto launch = [&](uint4 *counts, const ulonglong2 *offs, uint64_t n, uint32_t *words, uint8_t *) {
        return launch_hit_runs(st, pt->k, sq->d_desc, d_chunks.get(), nchunks, sq->d_seqw, sq->d_nmw, sq->d_has_n, pt->d_slots, pt->nslots,
                               pt->max_probe, counts, offs, n, words, words + n, words + 2 * n);
    };
    uint64_t sums[2] = {0, 0};  // the hits, nothing
    const int r = runs_two_pass(pt->ctx, fn, "contig", sq->n, w.first.data(), nchunks, launch, out, nruns, hits, total_out, sums, ms);
    *nhits = sums[0];
    return r;
}

}  // namespace

extern "C" int pg_postable_create(pg_ctx *ctx, int k, uint64_t capacity_keys, pg_postable **out) {
    PG_API_BEGIN
    if (!ctx || !out) return fail(PG_E_INVALID, "pg_postable_create: NULL argument");
    std::unique_ptr<pg_postable> pt;
    if (int r = postable_create(ctx, k, capacity_keys, pt)) return r;
    *out = pt.release();
    return PG_OK;
    PG_API_END
}

extern "C" int pg_postable_destroy(pg_postable *pt) {
    PG_API_BEGIN
    if (pt) postable_free(pt);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_postable_insert_seqset(pg_postable *pt, int side, const pg_seqset *seqs) {
    PG_API_BEGIN
    if (!pt || !seqs) return fail(PG_E_INVALID, "pg_postable_insert_seqset: NULL argument");
    return postable_insert(pt, side, seqs);
    PG_API_END
}

extern "C" int pg_postable_mates(pg_postable *pt, const pg_seqset *seqsA, uint32_t *mates_out, uint64_t *nmated) {
    PG_API_BEGIN
    if (!pt || !seqsA || !nmated) return fail(PG_E_INVALID, "pg_postable_mates: NULL argument");
    return postable_mates(pt, seqsA, mates_out, nmated);
    PG_API_END
}

extern "C" int pg_mate_runs(pg_ctx *ctx, const uint32_t *mates, uint32_t ncontigs, const uint64_t *nkmers, uint64_t cap,
                            uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint32_t *run_mate,
                            uint64_t *nruns_per_contig, uint64_t *total) {
    PG_API_BEGIN
    if (!ctx || (ncontigs && !nkmers) || !runs_args_ok(ncontigs, cap, run_contig, run_start, run_end, run_mate, nruns_per_contig, total))
        return fail(PG_E_INVALID, "pg_mate_runs: NULL argument");
    uint64_t n = 0;
    for (uint32_t c = 0; c < ncontigs; ++c) {
        if (nkmers[c] > POS_MAX_BASES || n + nkmers[c] > POS_MAX_BASES)
            return fail(PG_E_INVALID, "pg_mate_runs: more than %llu positions", (unsigned long long)POS_MAX_BASES);
        n += nkmers[c];
    }
    if (n && !mates) return fail(PG_E_INVALID, "pg_mate_runs: NULL argument");
    if (int r = use_device(ctx)) return r;
    DevBuf<uint32_t> d_mates;
    if (n) {
        hipError_t e = d_mates.alloc(n);
        if (e == hipSuccess) e = hipMemcpyAsync(d_mates.get(), mates, n * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(PG_E_HIP, "pg_mate_runs: %s", hipGetErrorString(e));
    }
    const RunsOut out = host_runs(cap, run_contig, run_start, run_end, run_mate);
    const int r = mate_runs_dev(ctx, "pg_mate_runs", d_mates.get(), ncontigs, nkmers, out, nruns_per_contig, total, nullptr);
    if (n) hipStreamSynchronize(ctx->stream);  // (the upload's source is the caller's; the buffer goes with the scope)
    return r;
    PG_API_END
}

extern "C" int pg_synteny_segments(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint64_t cap,
                                   uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint32_t *run_mate,
                                   uint64_t *nruns_per_contig, uint64_t *total, uint64_t *nmated) {
    PG_API_BEGIN
    if (!ctx || !seqsA || !seqsB || !nmated ||
        !runs_args_ok(seqsA->n, cap, run_contig, run_start, run_end, run_mate, nruns_per_contig, total))
        return fail(PG_E_INVALID, "pg_synteny_segments: NULL argument");
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "pg_synteny_segments: k=%d unsupported (1..32)", k);
    if (seqsA->ctx != ctx || seqsB->ctx != ctx) return fail(PG_E_INVALID, "pg_synteny_segments: a seqset of another context");
    // both sides' limits before anything is launched
    std::vector<uint64_t> nk(seqsA->n);
    KmerWalk a, b;
    if (int r = walk_side(seqsA, k, "pg_synteny_segments", a)) return r;
    if (int r = walk_side(seqsB, k, "pg_synteny_segments", b)) return r;
    for (uint32_t c = 0; c < seqsA->n; ++c) nk[c] = seqsA->desc[c].len >= (uint64_t)k ? seqsA->desc[c].len - k + 1 : 0;
    *total = *nmated = 0;
    for (uint32_t c = 0; c < seqsA->n; ++c) nruns_per_contig[c] = 0;
    std::fill(g_last_ms, g_last_ms + 5, 0.0f);
    if (a.nkmers == 0 || b.nkmers == 0) return PG_OK;  // (no k-mer on one side: no mate)
    MatedTable pt;
    float *ms = g_last_ms;
    if (int r = mated_table(ctx, k, seqsA, seqsB, a.nkmers + b.nkmers, pt, nmated, ms)) return r;
    uint64_t mated = 0;
    const RunsOut out = host_runs(cap, run_contig, run_start, run_end, run_mate);
    if (int r = mate_runs_dev(ctx, "pg_synteny_segments", pt.p->d_mates, seqsA->n, nk.data(), out, nruns_per_contig, total, &mated, ms + 3))
        return r;
    if (mated != *nmated)  // (two kernels counted the same array)
        return fail(PG_E_HIP, "pg_synteny_segments: %llu mates written, %llu read", (unsigned long long)*nmated, (unsigned long long)mated);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_synteny_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_synteny_last_timing: NULL argument");
    std::copy(g_last_ms, g_last_ms + 5, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_run_blocks(pg_ctx *ctx, const uint32_t *run_contig, const uint32_t *run_start, const uint32_t *run_end,
                             const uint32_t *run_mate, uint64_t nruns, uint32_t ncontigsA, uint32_t ncontigsB, const uint64_t *lensB,
                             uint32_t min_run, uint32_t max_gap, uint32_t max_shift, uint64_t cap, uint32_t *blk_contig,
                             uint32_t *blk_start, uint32_t *blk_end, uint32_t *blk_mate_first, uint32_t *blk_mate_last,
                             uint32_t *blk_kmers, uint32_t *blk_runs, uint32_t *blk_shifted, uint64_t *nblocks_per_contig,
                             uint64_t *total) {
    PG_API_BEGIN
    const BlockArrays out{blk_contig, blk_start, blk_end, blk_mate_first, blk_mate_last, blk_kmers, blk_runs, blk_shifted};
    if (!ctx || !total || (ncontigsA && !nblocks_per_contig) || (ncontigsB && !lensB) || (cap && !out.all()) ||
        (nruns && !(run_contig && run_start && run_end && run_mate)))
        return fail(PG_E_INVALID, "pg_run_blocks: NULL argument");
    const BlockParams p{min_run, max_gap, max_shift};
    if (int r = block_params_ok("pg_run_blocks", p)) return r;
    if (nruns > POS_MAX_BASES) return fail(PG_E_INVALID, "pg_run_blocks: more than %llu runs", (unsigned long long)POS_MAX_BASES);
    std::vector<uint64_t> boff;
    if (!contig_offsets(ncontigsB, lensB, boff)) return fail(PG_E_INVALID, "pg_run_blocks: genome B of more than 2^32 positions");
    std::vector<uint64_t> per;
    if (int r = runs_ok("pg_run_blocks", run_contig, run_start, run_end, run_mate, nruns, ncontigsA, boff.back(), per)) return r;
    *total = 0;
    for (uint32_t c = 0; c < ncontigsA; ++c) nblocks_per_contig[c] = 0;
    if (nruns == 0) return PG_OK;
    if (int r = use_device(ctx)) return r;
    DevBuf<uint32_t> d_runs;
    hipError_t e = d_runs.alloc((size_t)3 * nruns);
    if (e == hipSuccess) e = hipMemcpyAsync(d_runs.get(), run_start, nruns * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_runs.get() + nruns, run_end, nruns * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_runs.get() + 2 * nruns, run_mate, nruns * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        hipStreamSynchronize(ctx->stream);
        return fail(PG_E_HIP, "pg_run_blocks: %s", hipGetErrorString(e));
    }
    const int r = run_blocks_dev(ctx, "pg_run_blocks", d_runs.get(), nruns, ncontigsA, per.data(), boff, p, cap, out, nblocks_per_contig, total);
    hipStreamSynchronize(ctx->stream);  // (the uploads' sources are the caller's; the buffer goes with the scope)
    return r;
    PG_API_END
}

extern "C" int pg_synteny_blocks(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint32_t min_run, uint32_t max_gap,
                                 uint32_t max_shift, uint64_t cap, uint32_t *blk_contig, uint32_t *blk_start, uint32_t *blk_end,
                                 uint32_t *blk_mate_first, uint32_t *blk_mate_last, uint32_t *blk_kmers, uint32_t *blk_runs,
                                 uint32_t *blk_shifted, uint64_t *nblocks_per_contig, uint64_t *total, uint64_t *nmated, uint64_t *nruns) {
    PG_API_BEGIN
    const BlockArrays out{blk_contig, blk_start, blk_end, blk_mate_first, blk_mate_last, blk_kmers, blk_runs, blk_shifted};
    if (!ctx || !seqsA || !seqsB || !total || !nmated || !nruns || (seqsA->n && !nblocks_per_contig) || (cap && !out.all()))
        return fail(PG_E_INVALID, "pg_synteny_blocks: NULL argument");
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "pg_synteny_blocks: k=%d unsupported (1..32)", k);
    if (seqsA->ctx != ctx || seqsB->ctx != ctx) return fail(PG_E_INVALID, "pg_synteny_blocks: a seqset of another context");
    const BlockParams p{min_run, max_gap, max_shift};
    if (int r = block_params_ok("pg_synteny_blocks", p)) return r;
    // both sides' limits before anything is launched
    std::vector<uint64_t> nk(seqsA->n), per(seqsA->n, 0), lensB(seqsB->n), boff;
    KmerWalk a, b;
    if (int r = walk_side(seqsA, k, "pg_synteny_blocks", a)) return r;
    if (int r = walk_side(seqsB, k, "pg_synteny_blocks", b)) return r;
    for (uint32_t c = 0; c < seqsA->n; ++c) nk[c] = seqsA->desc[c].len >= (uint64_t)k ? seqsA->desc[c].len - k + 1 : 0;
    for (uint32_t c = 0; c < seqsB->n; ++c) lensB[c] = seqsB->desc[c].len;
    contig_offsets(seqsB->n, lensB.data(), boff);  // (a side of at most 2^31 - 1 bases: checked by walk_side)
    *total = *nmated = *nruns = 0;
    for (uint32_t c = 0; c < seqsA->n; ++c) nblocks_per_contig[c] = 0;
    std::fill(g_blocks_ms, g_blocks_ms + 7, 0.0f);
    if (a.nkmers == 0 || b.nkmers == 0) return PG_OK;  // (no k-mer on one side: no mate)
    MatedTable pt;
    float *ms = g_blocks_ms;
    if (int r = mated_table(ctx, k, seqsA, seqsB, a.nkmers + b.nkmers, pt, nmated, ms)) return r;
    uint64_t mated = 0;
    DevBuf<uint32_t> d_runs;  // the runs: emitted into HBM and read there
    RunsOut runs_out;
    runs_out.keep = &d_runs;
    if (int r = mate_runs_dev(ctx, "pg_synteny_blocks", pt.p->d_mates, seqsA->n, nk.data(), runs_out, per.data(), nruns, &mated, ms + 3))
        return r;
    if (mated != *nmated)  // (two kernels counted the same array)
        return fail(PG_E_HIP, "pg_synteny_blocks: %llu mates written, %llu read", (unsigned long long)*nmated, (unsigned long long)mated);
    if (*nruns == 0) return PG_OK;
    return run_blocks_dev(ctx, "pg_synteny_blocks", d_runs.get(), *nruns, seqsA->n, per.data(), boff, p, cap, out, nblocks_per_contig,
                          total, ms + 5);
    PG_API_END
}

extern "C" int pg_synteny_blocks_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_synteny_blocks_last_timing: NULL argument");
    std::copy(g_blocks_ms, g_blocks_ms + 7, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_run_variants(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, const uint32_t *run_contig,
                               const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate, uint64_t nruns,
                               uint32_t min_run, uint32_t max_gap, uint32_t max_shift, uint64_t cap, uint32_t *var_contig,
                               uint32_t *var_posA, uint32_t *var_lenA, uint32_t *var_posB, uint32_t *var_lenB, uint32_t *var_info,
                               uint32_t *var_mismatches, uint64_t *var_alleleA, uint64_t *var_alleleB, uint64_t *class_counts,
                               uint64_t *links, uint64_t *total) {
    PG_API_BEGIN
    const VariantArrays out{var_contig, var_posA, var_lenA, var_posB, var_lenB, var_info, var_mismatches, var_alleleA, var_alleleB};
    if (!ctx || !seqsA || !seqsB || !class_counts || !links || !total || (cap && !out.all()) ||
        (nruns && !(run_contig && run_start && run_end && run_mate)))
        return fail(PG_E_INVALID, "pg_run_variants: NULL argument");
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "pg_run_variants: k=%d unsupported (1..32)", k);
    if (seqsA->ctx != ctx || seqsB->ctx != ctx) return fail(PG_E_INVALID, "pg_run_variants: a seqset of another context");
    const BlockParams p{min_run, max_gap, max_shift};
    if (int r = variant_params_ok("pg_run_variants", p)) return r;
    if (nruns > POS_MAX_BASES) return fail(PG_E_INVALID, "pg_run_variants: more than %llu runs", (unsigned long long)POS_MAX_BASES);
    KmerWalk wa, wb;  // (a side of at most 2^31 - 1 bases)
    if (int r = walk_side(seqsA, k, "pg_run_variants", wa)) return r;
    if (int r = walk_side(seqsB, k, "pg_run_variants", wb)) return r;
    std::vector<uint64_t> lensB(seqsB->n), boff, per, nblocks(seqsA->n, 0);
    for (uint32_t c = 0; c < seqsB->n; ++c) lensB[c] = seqsB->desc[c].len;
    contig_offsets(seqsB->n, lensB.data(), boff);
    if (int r = runs_ok("pg_run_variants", run_contig, run_start, run_end, run_mate, nruns, seqsA->n, boff.back(), per)) return r;
    for (uint64_t i = 0; i < nruns; ++i) {
        // the bases of the run's k-mers: inside its contig of A, and inside ONE contig of B
        const uint64_t n = run_end[i] - run_start[i], b = run_mate[i] >> 1, lo = (run_mate[i] & 1) ? b - (n - 1) : b;
        if ((uint64_t)run_end[i] + (uint64_t)k - 1 > seqsA->desc[run_contig[i]].len)
            return fail(PG_E_INVALID, "pg_run_variants: run %llu leaves its contig of A", (unsigned long long)i);
        const size_t cb = (size_t)(std::upper_bound(boff.begin(), boff.end(), lo) - boff.begin()) - 1;
        if (lo + n + (uint64_t)k - 1 > boff[cb + 1])
            return fail(PG_E_INVALID, "pg_run_variants: run %llu leaves its contig of B", (unsigned long long)i);
    }
    std::fill(class_counts, class_counts + 6, 0ull);
    *links = *total = 0;
    if (nruns == 0) return PG_OK;
    if (int r = use_device(ctx)) return r;
    DevBuf<uint32_t> d_runs;
    hipError_t e = d_runs.alloc((size_t)3 * nruns);
    if (e == hipSuccess) e = hipMemcpyAsync(d_runs.get(), run_start, nruns * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_runs.get() + nruns, run_end, nruns * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_runs.get() + 2 * nruns, run_mate, nruns * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        hipStreamSynchronize(ctx->stream);
        return fail(PG_E_HIP, "pg_run_variants: %s", hipGetErrorString(e));
    }
    BlocksPlan plan;
    uint64_t nblk = 0;
    int r = blocks_count_dev(ctx, "pg_run_variants", d_runs.get(), nruns, seqsA->n, per.data(), boff, p, plan, nblocks.data(), &nblk);
    if (r == PG_OK)
        r = link_variants_dev(ctx, "pg_run_variants", k, seqsA, seqsB, d_runs.get(), nruns, p, plan, cap, out, class_counts, links, total);
    hipStreamSynchronize(ctx->stream);  // (the uploads' sources are the caller's; the buffer goes with the scope)
    return r;
    PG_API_END
}

extern "C" int pg_synteny_variants(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint32_t min_run, uint32_t max_gap,
                                   uint32_t max_shift, uint64_t cap, uint32_t *var_contig, uint32_t *var_posA, uint32_t *var_lenA,
                                   uint32_t *var_posB, uint32_t *var_lenB, uint32_t *var_info, uint32_t *var_mismatches,
                                   uint64_t *var_alleleA, uint64_t *var_alleleB, uint64_t *class_counts, uint64_t *links, uint64_t *total,
                                   uint64_t *nmated, uint64_t *nruns, uint64_t *nblocks) {
    PG_API_BEGIN
    const VariantArrays out{var_contig, var_posA, var_lenA, var_posB, var_lenB, var_info, var_mismatches, var_alleleA, var_alleleB};
    if (!ctx || !seqsA || !seqsB || !class_counts || !links || !total || !nmated || !nruns || !nblocks || (cap && !out.all()))
        return fail(PG_E_INVALID, "pg_synteny_variants: NULL argument");
    if (k < 1 || k > 32) return fail(PG_E_INVALID, "pg_synteny_variants: k=%d unsupported (1..32)", k);
    if (seqsA->ctx != ctx || seqsB->ctx != ctx) return fail(PG_E_INVALID, "pg_synteny_variants: a seqset of another context");
    const BlockParams p{min_run, max_gap, max_shift};
    if (int r = variant_params_ok("pg_synteny_variants", p)) return r;
    // both sides' limits before anything is launched
    std::vector<uint64_t> nk(seqsA->n), per(seqsA->n, 0), perblk(seqsA->n, 0), lensB(seqsB->n), boff;
    KmerWalk a, b;
    if (int r = walk_side(seqsA, k, "pg_synteny_variants", a)) return r;
    if (int r = walk_side(seqsB, k, "pg_synteny_variants", b)) return r;
    for (uint32_t c = 0; c < seqsA->n; ++c) nk[c] = seqsA->desc[c].len >= (uint64_t)k ? seqsA->desc[c].len - k + 1 : 0;
    for (uint32_t c = 0; c < seqsB->n; ++c) lensB[c] = seqsB->desc[c].len;
    contig_offsets(seqsB->n, lensB.data(), boff);  // (a side of at most 2^31 - 1 bases: checked by walk_side)
    std::fill(class_counts, class_counts + 6, 0ull);
    *links = *total = *nmated = *nruns = *nblocks = 0;
    std::fill(g_variants_ms, g_variants_ms + 9, 0.0f);
    if (a.nkmers == 0 || b.nkmers == 0) return PG_OK;  // (no k-mer on one side: no mate)
    MatedTable pt;
    float *ms = g_variants_ms;
    if (int r = mated_table(ctx, k, seqsA, seqsB, a.nkmers + b.nkmers, pt, nmated, ms)) return r;
    uint64_t mated = 0;
    DevBuf<uint32_t> d_runs;  // the runs: emitted into HBM and read there
    RunsOut runs_out;
    runs_out.keep = &d_runs;
    if (int r = mate_runs_dev(ctx, "pg_synteny_variants", pt.p->d_mates, seqsA->n, nk.data(), runs_out, per.data(), nruns, &mated, ms + 3))
        return r;
    if (mated != *nmated)  // (two kernels counted the same array)
        return fail(PG_E_HIP, "pg_synteny_variants: %llu mates written, %llu read", (unsigned long long)*nmated, (unsigned long long)mated);
    if (*nruns == 0) return PG_OK;
    BlocksPlan plan;
    if (int r = blocks_count_dev(ctx, "pg_synteny_variants", d_runs.get(), *nruns, seqsA->n, per.data(), boff, p, plan, perblk.data(), nblocks,
                                 ms + 5))
        return r;
    return link_variants_dev(ctx, "pg_synteny_variants", k, seqsA, seqsB, d_runs.get(), *nruns, p, plan, cap, out, class_counts, links,
                             total, ms + 7);
    PG_API_END
}

extern "C" int pg_synteny_variants_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_synteny_variants_last_timing: NULL argument");
    std::copy(g_variants_ms, g_variants_ms + 9, ms_out);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_postable_hit_runs(pg_postable *pt, const pg_seqset *seqsG, uint64_t cap, uint32_t *run_contig, uint32_t *run_start,
                                    uint32_t *run_end, uint32_t *run_hit, uint64_t *nruns_per_contig, uint64_t *hits_per_contig,
                                    uint64_t *total, uint64_t *nhits) {
    PG_API_BEGIN
    if (!pt || !seqsG || !nhits || !runs_args_ok(seqsG->n, cap, run_contig, run_start, run_end, run_hit, nruns_per_contig, total))
        return fail(PG_E_INVALID, "pg_postable_hit_runs: NULL argument");
    KmerWalk w;
    if (int r = hit_walk(pt, seqsG, "pg_postable_hit_runs", w)) return r;
    std::fill(g_locate_ms, g_locate_ms + 4, 0.0f);
    const RunsOut out = host_runs(cap, run_contig, run_start, run_end, run_hit);
    return hit_runs_dev(pt, "pg_postable_hit_runs", seqsG, w, out, nruns_per_contig, hits_per_contig, total, nhits, g_locate_ms);
    PG_API_END
}

extern "C" int pg_postable_locate(pg_postable *pt, const pg_seqset *seqsG, const pg_seqset *seqsQ, uint32_t min_run, uint32_t max_gap,
                                  uint32_t max_shift, uint64_t cap, uint32_t *blk_contig, uint32_t *blk_start, uint32_t *blk_end,
                                  uint32_t *blk_hit_first, uint32_t *blk_hit_last, uint32_t *blk_kmers, uint32_t *blk_runs,
                                  uint32_t *blk_shifted, uint64_t *nblocks_per_contig, uint64_t *total, uint64_t *nhits, uint64_t *nruns) {
    PG_API_BEGIN
    const BlockArrays out{blk_contig, blk_start, blk_end, blk_hit_first, blk_hit_last, blk_kmers, blk_runs, blk_shifted};
    if (!pt || !seqsG || !seqsQ || !total || !nhits || !nruns || (seqsG->n && !nblocks_per_contig) || (cap && !out.all()))
        return fail(PG_E_INVALID, "pg_postable_locate: NULL argument");
    const BlockParams p{min_run, max_gap, max_shift};
    if (int r = block_params_ok("pg_postable_locate", p)) return r;
    if (seqsQ->ctx != pt->ctx) return fail(PG_E_INVALID, "pg_postable_locate: table and queries belong to different contexts");
    KmerWalk w;
    if (int r = hit_walk(pt, seqsG, "pg_postable_locate", w)) return r;
    // the queries: the set inserted as side 1, whose contigs' offsets the same-contig condition needs
    std::vector<uint64_t> lensQ(seqsQ->n), boff, per(seqsG->n, 0);
    uint64_t basesQ = 0;
    for (uint32_t c = 0; c < seqsQ->n; ++c) basesQ += (lensQ[c] = seqsQ->desc[c].len);
    if (seqsQ->n != pt->side_contigs[1] || basesQ != pt->side_bases[1])
        return fail(PG_E_INVALID, "pg_postable_locate: seqsQ (%u contigs, %llu bases) is not the set inserted as side 1 (%u, %llu)", seqsQ->n,
                    (unsigned long long)basesQ, pt->side_contigs[1], (unsigned long long)pt->side_bases[1]);
    contig_offsets(seqsQ->n, lensQ.data(), boff);  // (a side of at most 2^31 - 1 bases: checked when it was inserted)
    *total = *nhits = *nruns = 0;
    for (uint32_t c = 0; c < seqsG->n; ++c) nblocks_per_contig[c] = 0;
    std::fill(g_locate_ms, g_locate_ms + 4, 0.0f);
    DevBuf<uint32_t> d_runs;  // the runs: emitted into HBM and read there
    RunsOut runs_out;
    runs_out.keep = &d_runs;
    if (int r = hit_runs_dev(pt, "pg_postable_locate", seqsG, w, runs_out, per.data(), nullptr, nruns, nhits, g_locate_ms)) return r;
    if (*nruns == 0) return PG_OK;
    if (*nruns > POS_MAX_BASES)  // (the run kernels number a contig's runs in 32 bits; known only once they are counted)
        return fail(PG_E_CAPACITY, "pg_postable_locate: more than %llu runs (stream fewer contigs at a time)", (unsigned long long)POS_MAX_BASES);
    return run_blocks_dev(pt->ctx, "pg_postable_locate", d_runs.get(), *nruns, seqsG->n, per.data(), boff, p, cap, out, nblocks_per_contig,
                          total, g_locate_ms + 2);
    PG_API_END
}

extern "C" int pg_locate_last_timing(float *ms_out) {
    PG_API_BEGIN
    if (!ms_out) return fail(PG_E_INVALID, "pg_locate_last_timing: NULL argument");
    std::copy(g_locate_ms, g_locate_ms + 4, ms_out);
    return PG_OK;
    PG_API_END
}
