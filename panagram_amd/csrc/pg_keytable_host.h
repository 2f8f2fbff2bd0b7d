// pg_keytable_host.h — the host's half of the key tables (pg_keytable_dev.h has the policy and the device's half): how many slots
// a table of a given capacity gets and how far a lane walks, the (contig, piece) jobs that the kernels over a seqset's k-mer
// positions take, and the launch of a kernel that counts into a few 64-bit counters.  For the position table
// (pg_api_synteny.hip), the count table (pg_api_copies.hip) and the distinct-k-mer sketch (pg_api_sketch.hip).
#pragma once
#include "pg_host.h"

static constexpr uint32_t KEYTABLE_MAX_PROBE = 4096;  // slots a lane walks before it gives up (load <= 0.5: tens at the most)

// slots = the power of two at or above 2 * capacity, two at the least
inline uint64_t table_slots(uint64_t capacity) {
    uint64_t n = 2;
    while (n < 2 * capacity) n <<= 1;
    return n;
}
inline uint32_t table_max_probe(uint64_t nslots) { return (uint32_t)std::min<uint64_t>(nslots, KEYTABLE_MAX_PROBE); }

// The k-mer positions of a seqset's contigs in pieces of `piece`: jobs[j] = (contig, piece number), the jobs of contig c being
// first[c] .. first[c + 1]; off[c] = the bases and koff[c] = the k-mer positions of the contigs before c.  All in 64 bits: a
// caller holds them against its own limit before it narrows them.
struct KmerWalk {
    std::vector<uint2> jobs;
    std::vector<uint64_t> first, off, koff;  // [n + 1], [n], [n]
    uint64_t bases = 0, nkmers = 0;
    const char *noun = "pieces";  // what the caller's documents call its pieces, for the one message here
};

// the one limit every such launch has: a block per piece, 2^31 - 1 blocks
inline int walk_kmers(const pg_seqset *sq, int k, uint32_t piece, const char *fn, KmerWalk &w) {
    const uint32_t n = sq->n;
    w.first.assign((size_t)n + 1, 0);
    w.off.resize(n);
    w.koff.resize(n);
    uint64_t njobs = 0;
    for (uint32_t c = 0; c < n; ++c) {
        const uint64_t len = sq->desc[c].len, nk = len >= (uint64_t)k ? len - k + 1 : 0;
        w.first[c] = njobs;
        w.off[c] = w.bases;
        w.koff[c] = w.nkmers;
        njobs += (nk + piece - 1) / piece;
        if (njobs > 0x7FFFFFFFull) return fail(PG_E_INVALID, "%s: more than 2^31 - 1 %s of %u positions", fn, w.noun, piece);
        w.bases += len;
        w.nkmers += nk;
    }
    w.first[n] = njobs;
    w.jobs.resize(njobs);
    for (uint32_t c = 0; c < n; ++c)
        for (uint64_t j = w.first[c]; j < w.first[c + 1]; ++j) w.jobs[j] = make_uint2(c, (uint32_t)(j - w.first[c]));
    return PG_OK;
}

// One launch that counts: the jobs uploaded, ctr[0 .. n) zeroed in HBM, launch(jobs, njobs, counters) enqueued between the two
// events of `ms` (NULL: not timed), the counters read back into ctr and the stream synchronised.  What the launch reads beside the
// jobs is the caller's, enqueued before; what it leaves beside the counters is complete when this returns.
template <class Launch>
hipError_t counted_launch(hipStream_t st, const std::vector<uint2> &jobs, unsigned long long *ctr, size_t n, float *ms, Launch launch) {
    DevBuf<uint2> d_jobs;
    DevBuf<unsigned long long> d_ctr;
    LaunchTimer tm(ms);
    hipError_t e = d_jobs.upload(jobs, st);
    if (e == hipSuccess) e = d_ctr.alloc(n);
    if (e == hipSuccess) e = hipMemsetAsync(d_ctr.get(), 0, n * 8, st);
    if (e == hipSuccess) e = tm.start(st);
    if (e == hipSuccess) e = launch(d_jobs.get(), (uint32_t)jobs.size(), d_ctr.get());
    if (e == hipSuccess) e = tm.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_ctr.get(), n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) tm.read();
    return e;
}
