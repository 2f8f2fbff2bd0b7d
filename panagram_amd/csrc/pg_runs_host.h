// pg_runs_host.h — the host half of every run kernel that works in two passes over chunks (k_mate_runs, k_hit_runs, k_novel_runs:
// pg_runscan.h; k_find_runs: pg_find.hip): the scans between the count pass and the emit pass, and the walk through both.
//
// runs_stitch is plain C++ without a GPU call, so that a stand-alone program can hold it to a loop over the chunks under the host
// sanitizers (tools/runs_stitch_check.cpp); runs_two_pass, behind it, is compiled by hipcc only.
#pragma once
#include <cstdint>

namespace pg {

// Group g's chunks (a contig's, a window's) are [first[g], first[g + 1]), in order — a group may have none.  counts[chunk] is what
// the count pass left, in the one field order of all run kernels: {x: tally a, y: run starts, z: run ends, w: tally b} (a uint4, or
// a struct with these members).  Starts and ends are scanned separately, over all groups: offs[chunk] = {x: the starts, y: the ends
// of all chunks before it} — the i-th start and the i-th end of a group are one run, which may begin in one chunk and end in a
// later one.  nruns[g] = the runs of group g; tally_a[g] (when given) = the group's sum of tally a; sums = the two tallies overall.
// Returns the runs of all groups, or ~0 when a group's starts and ends differ (every run of a group starts and ends inside it:
// never, by construction) — bad = {the group, the starts up to and with it, the ends}.
template <class Count4, class Offs2>
inline uint64_t runs_stitch(uint32_t ngroups, const uint64_t *first, const Count4 *counts, Offs2 *offs, uint64_t *nruns, uint64_t *tally_a,
                            uint64_t sums[2], uint64_t bad[3]) {
    uint64_t nstarts = 0, nends = 0, na = 0, nb = 0;
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint64_t s0 = nstarts, a0 = na;
        for (uint64_t i = first[g]; i < first[g + 1]; ++i) {
            offs[i].x = nstarts, offs[i].y = nends;
            na += counts[i].x;
            nstarts += counts[i].y;
            nends += counts[i].z;
            nb += counts[i].w;
        }
        nruns[g] = nstarts - s0;
        if (tally_a) tally_a[g] = na - a0;
        if (nstarts != nends) {
            bad[0] = g, bad[1] = nstarts, bad[2] = nends;
            return ~0ull;
        }
    }
    sums[0] = na, sums[1] = nb;
    return nstarts;
}

}  // namespace pg

#ifdef __HIPCC__
#include "pg_host.h"

namespace pg {

// Where the runs of runs_two_pass go, and in what shape.  The emit pass writes `nwords` planes of 32-bit words — the run's start,
// its end, then what the kernel stores beside a start — and `nbytes` planes of bytes, each of as many entries as runs are emitted.
//   the caller's host arrays   words[i] / bytes[i], `cap` entries each, and `contig` (when given) for the group number of every run.
//       More runs than cap: prefix false — none is emitted, the caller sees the total and asks again; prefix true — the first cap
//       runs in (group, start) order are.  (The caller chose that number: should the device have no memory for it, that is a
//       PG_E_CAPACITY, to be answered with a smaller one.)
//   keep   all runs, whatever their number, stay in HBM as the word planes back to back in *keep; nothing is downloaded.
struct RunsOut {
    uint32_t nwords = 3, nbytes = 0;
    uint64_t cap = 0;
    bool prefix = false;
    uint32_t *contig = nullptr;
    uint32_t *words[3] = {nullptr, nullptr, nullptr};
    uint8_t *bytes[2] = {nullptr, nullptr};
    DevBuf<uint32_t> *keep = nullptr;
};

// The two passes of a run kernel over its chunks: count, runs_stitch, emit.  launch(counts, offs, n, words, bytes) enqueues one pass
// over nchunks chunks — offs NULL: the count pass; otherwise the emit pass of the first n runs, plane i at words + i * n and at
// bytes + i * n.  The chunks of group g are first[g] .. first[g + 1]; `group` names one in a message ("contig", "window").
// nruns[g], tally_a[g] (when given), *total_out and sums[2] always; the runs under `out`; ms (when given): ms[0] the count launch,
// ms[1] the emit launch.  The caller zeroes its outputs and uploads its chunks; an error's message begins with fn.
template <class Launch>
PG_INTERNAL int runs_two_pass(pg_ctx *ctx, const char *fn, const char *group, uint32_t ngroups, const uint64_t *first, uint32_t nchunks,
                              Launch launch, const RunsOut &out, uint64_t *nruns, uint64_t *tally_a, uint64_t *total_out, uint64_t sums[2],
                              float *ms) {
    hipStream_t st = ctx->stream;
    const auto hip_fail = [&](hipError_t e) {
        hipStreamSynchronize(st);  // (the sources of the uploads and the targets of the copies go with the callers' scopes)
        return fail(PG_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    };
    DevBuf<uint4> d_counts;
    std::vector<uint4> counts(nchunks);
    LaunchTimer tc(ms), te(ms ? ms + 1 : nullptr);
    hipError_t e = d_counts.alloc(nchunks);
    if (e == hipSuccess) e = tc.start(st);
    if (e == hipSuccess) e = launch(d_counts.get(), nullptr, 0, nullptr, nullptr);
    if (e == hipSuccess) e = tc.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d_counts.get(), (size_t)nchunks * sizeof(uint4), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e);
    tc.read();
    std::vector<ulonglong2> offs(nchunks);
    uint64_t bad[3];
    const uint64_t total = runs_stitch(ngroups, first, counts.data(), offs.data(), nruns, tally_a, sums, bad);
    if (total == ~0ull)
        return fail(PG_E_HIP, "%s: %s %u: %llu run starts, %llu run ends", fn, group, (uint32_t)bad[0], (unsigned long long)bad[1],
                    (unsigned long long)bad[2]);
    *total_out = total;
    // the runs to emit: all of them, or none / the first cap when the caller's arrays are too short
    const uint64_t n = out.keep || total <= out.cap ? total : out.prefix ? out.cap : 0;
    if (n == 0) return PG_OK;
    DevBuf<ulonglong2> d_offs;
    DevBuf<uint32_t> d_words;
    DevBuf<uint8_t> d_bytes;
    e = d_offs.upload(offs, st);
    if (e == hipSuccess) e = d_words.alloc((size_t)out.nwords * n);
    if (e == hipSuccess && out.nbytes) e = d_bytes.alloc((size_t)out.nbytes * n);
    if (e == hipErrorOutOfMemory && out.prefix) {
        hipStreamSynchronize(st);
        return fail(PG_E_CAPACITY, "%s: no memory for %llu runs", fn, (unsigned long long)n);
    }
    if (e == hipSuccess) e = te.start(st);
    if (e == hipSuccess) e = launch(nullptr, d_offs.get(), n, d_words.get(), d_bytes.get());
    if (e == hipSuccess) e = te.stop(st);
    for (uint32_t i = 0; i < out.nwords && !out.keep && e == hipSuccess; ++i)
        e = hipMemcpyAsync(out.words[i], d_words.get() + i * n, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    for (uint32_t i = 0; i < out.nbytes && !out.keep && e == hipSuccess; ++i)
        e = hipMemcpyAsync(out.bytes[i], d_bytes.get() + i * n, (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e);
    te.read();
    if (out.keep) {
        std::swap(out.keep->p, d_words.p);
        return PG_OK;
    }
    if (out.contig) {
        uint64_t at = 0;
        for (uint32_t g = 0; g < ngroups && at < n; ++g)
            for (uint64_t i = 0; i < nruns[g] && at < n; ++i) out.contig[at++] = g;
    }
    return PG_OK;
}

}  // namespace pg
#endif
