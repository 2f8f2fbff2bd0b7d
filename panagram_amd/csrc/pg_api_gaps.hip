// pg_api_gaps.hip — host side of the C-ABI: the absence runs of a result's finished rows (a window query: it opens with
// pg_api_query.hip's shared prologue, as pg_api_patterns.hip does).
#include "pg_host.h"
#include "pg_gaps_host.h"

static_assert(sizeof(GapEdge) == sizeof(uint2) && sizeof(GapRun) == sizeof(uint4), "the kernel's records, field by field");

// absence runs over sampled rows (query_bitmap with a per-column np.diff of the absence vector): one launch over the chunks
// of all windows, the stitch of the chunks' edges on the host, and — when the selected runs fit the caller's arrays — their
// records sorted
extern "C" int pg_result_absence_runs(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                                      const uint64_t *starts, const uint64_t *ends, const uint32_t *select_words, uint32_t maxlen,
                                      uint32_t min_len, uint32_t max_len, uint64_t cap, uint32_t *run_genome, uint32_t *run_start,
                                      uint32_t *run_rows, uint64_t *hist_out, uint64_t *absent_out, uint64_t *edge_out,
                                      uint64_t *nruns_out, uint64_t *total_out) {
    PG_API_BEGIN
    if (!r || !total_out || (nwin && (!contig || !starts || !ends || !hist_out || !absent_out || !edge_out || !nruns_out)) ||
        (cap && (!run_genome || !run_start || !run_rows)))
        return fail(PG_E_INVALID, "pg_result_absence_runs: NULL argument");
    if (int e = check_window_call(r, step, stride, nwin, "pg_result_absence_runs", "windows")) return e;
    const uint32_t N = r->N;
    if (N < 1 || N > GAPS_MAX_GENOMES) return fail(PG_E_INVALID, "pg_result_absence_runs: %u genomes (1 to %u)", N, GAPS_MAX_GENOMES);
    if (maxlen < 1 || maxlen > GAPS_MAX_MAXLEN)
        return fail(PG_E_INVALID, "pg_result_absence_runs: maxlen = %u (the spectrum takes 1 to %u)", maxlen, GAPS_MAX_MAXLEN);
    if (min_len < 1) return fail(PG_E_INVALID, "pg_result_absence_runs: min_len must be >= 1");
    Windows w;
    if (int e = gather_windows(r, step, stride, nwin, contig, starts, ends, "window", w)) return e;
    *total_out = 0;
    if (nwin == 0) return PG_OK;
    const std::vector<uint32_t> sw = mask_words(N, select_words, 0xFFFFFFFFu);  // (NULL: every genome)
    const size_t nb = (size_t)maxlen + 1, ncol = (size_t)nwin * N, nh = ncol * nb;
    std::fill(hist_out, hist_out + nh, 0);
    std::fill(absent_out, absent_out + ncol, 0);
    std::fill(edge_out, edge_out + 2 * ncol, 0);
    std::fill(nruns_out, nruns_out + nwin, 0);
    std::vector<uint2> chunks;
    std::vector<uint64_t> first;
    if (int e = cut_chunks("pg_result_absence_runs", nwin, starts, ends, GAPS_CHUNK, chunks, &first)) return e;
    bool any = false;
    for (uint32_t d : sw) any = any || d;
    if (chunks.empty() || !any) return PG_OK;  // (every window empty / no column selected: zeros)
    const uint32_t nchunks = (uint32_t)chunks.size();
    // room for the kernel's records: never more than the closed runs there can be (every other row of a column)
    uint64_t most = 0;
    for (uint32_t i = 0; i < nwin; ++i) most += (ends[i] - starts[i]) / 2 * N;
    const uint64_t dcap = std::min<uint64_t>(cap, most);
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    DevBuf<uint32_t> d_sw, d_hist;
    DevBuf<uint2> d_chunks, d_edges;
    DevBuf<unsigned long long> d_cnt;  // [nwin N] absent rows, [nwin] selected runs, the cursor
    DevBuf<uint4> d_recs;
    const size_t ncnt = ncol + nwin + 1;
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_sw.upload(sw, st);
    if (e == hipSuccess) e = d_chunks.upload(chunks, st);
    if (e == hipSuccess) e = d_hist.alloc(nh);
    if (e == hipSuccess) e = d_edges.alloc((size_t)nchunks * N);
    if (e == hipSuccess) e = d_cnt.alloc(ncnt);
    if (e == hipSuccess && dcap) e = d_recs.alloc(dcap);
    if (e == hipSuccess) e = hipMemsetAsync(d_hist.get(), 0, nh * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_edges.get(), 0, (size_t)nchunks * N * sizeof(uint2), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt.get(), 0, ncnt * 8, st);
    if (e == hipSuccess)
        e = launch_absence_runs(st, N, step == 1 ? r->d_out1 : r->d_out100, stride, w.base(), w.ends(), d_chunks.get(), nchunks,
                                d_sw.get(), maxlen, min_len, max_len, d_hist.get(), d_cnt.get(), d_edges.get(), d_cnt.get() + ncol,
                                d_cnt.get() + ncol + nwin, dcap, d_recs.get());
    std::vector<uint32_t> h_hist(nh);
    std::vector<GapEdge> h_edges((size_t)nchunks * N);
    std::vector<unsigned long long> h_cnt(ncnt);
    if (e == hipSuccess) e = hipMemcpyAsync(h_hist.data(), d_hist.get(), nh * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_edges.data(), d_edges.get(), h_edges.size() * sizeof(GapEdge), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt.data(), d_cnt.get(), ncnt * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_absence_runs: %s", hipGetErrorString(e));
    for (size_t i = 0; i < nh; ++i) hist_out[i] = h_hist[i];
    for (size_t i = 0; i < ncol; ++i) absent_out[i] = h_cnt[i];
    uint64_t in_chunks = 0;  // the selected runs the kernel closed
    for (uint32_t i = 0; i < nwin; ++i) in_chunks += (nruns_out[i] = h_cnt[ncol + i]);
    if (dcap && in_chunks != h_cnt[ncol + nwin])  // (with room to write to, the cursor has counted every selected run)
        return fail(PG_E_HIP, "pg_result_absence_runs: %llu selected runs counted, the cursor at %llu", (unsigned long long)in_chunks,
                    h_cnt[ncol + nwin]);
    std::vector<GapRun> runs;
    gaps_stitch(N, nwin, starts, ends, first.data(), GAPS_CHUNK, h_edges.data(), sw.data(), maxlen, min_len, max_len, hist_out,
                edge_out, nruns_out, runs);
    const uint64_t total = in_chunks + runs.size();
    *total_out = total;
    if (total == 0 || cap == 0 || total > cap) return PG_OK;  // (nothing to emit / the caller's arrays are too short)
    if (in_chunks > dcap)
        return fail(PG_E_HIP, "pg_result_absence_runs: %llu runs closed inside chunks, room for %llu", (unsigned long long)in_chunks,
                    (unsigned long long)dcap);
    const size_t stitched = runs.size();
    runs.resize(total);
    if (in_chunks) {
        e = hipMemcpyAsync(runs.data() + stitched, d_recs.get(), (size_t)in_chunks * sizeof(GapRun), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_absence_runs: %s", hipGetErrorString(e));
    }
    gaps_sort(runs);
    for (size_t i = 0; i < runs.size(); ++i) {
        run_genome[i] = runs[i].genome;
        run_start[i] = runs[i].start;
        run_rows[i] = runs[i].rows;
    }
    return PG_OK;
    PG_API_END
}
