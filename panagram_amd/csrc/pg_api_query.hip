// pg_api_query.hip — host side of the C-ABI: window queries over a result's finished rows, k-NN of rows.
#include "pg_host.h"

#include "pg_runs_host.h"  // RunsOut, runs_two_pass

// What the window queries (here and in pg_api_patterns.hip) share, beside check_step (pg_api.hip): one wording of every refusal,
// whoever asks.  A call opens with check_window_call, makes its own checks, and goes on with gather_windows.
// the step, the stride and the number n of windows ("bins", "windows") of entry point fn
int pg::check_window_call(const pg_result *r, int step, uint32_t stride, uint32_t n, const char *fn, const char *nouns) {
    if (int e = check_step(r, step)) return e;
    if (stride < 1) return fail(PG_E_INVALID, "%s: stride must be >= 1", fn);
    if (n > 0x7FFFFFFFu) return fail(PG_E_INVALID, "%s: %u %s (at most 2^31 - 1 per call)", fn, n, nouns);
    return PG_OK;
}
static int check_rows_readable(const pg_result *r, int step) {
    if (r->flags & PG_ANCHOR_COLUMNS_ONLY) return fail(PG_E_INVALID, "the result has no row buffer");
    if (!r->ev_ok) return fail(PG_E_INVALID, "pg_anchor_run has not been called on this result");
    if (step != 1 && (r->flags & PG_ANCHOR_ROWS_ONLY) && !r->ev_epi && !r->rows_valid)
        return fail(PG_E_INVALID, "rows-only result: the low-resolution rows need pg_rows_epilogue first");
    return PG_OK;
}
// the rows must be readable; then n windows ("bin", "window": the noun of the messages) of sampled rows, refused unless each
// lies within its contig -> w
int pg::gather_windows(const pg_result *r, int step, uint32_t stride, uint32_t n, const uint32_t *contig, const uint64_t *starts,
                       const uint64_t *ends, const char *noun, Windows &w) {
    if (int e = check_rows_readable(r, step)) return e;
    std::vector<uint64_t> &se = w.se;
    se.assign((size_t)n * 3, 0);
    w.n = n;
    w.longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (contig[i] >= r->ad.size()) return fail(PG_E_INVALID, "%s %u: contig %u out of range", noun, i, contig[i]);
        const AnchorDesc &a = r->ad[contig[i]];
        const uint64_t nrows = step == 1 ? (uint64_t)a.nkmers : r->nrows100[contig[i]];
        if (starts[i] > ends[i]) return fail(PG_E_INVALID, "%s %u: start %llu past end %llu", noun, i, (unsigned long long)starts[i],
                                             (unsigned long long)ends[i]);
        if (ends[i] > starts[i] && (nrows == 0 || ends[i] - 1 > (nrows - 1) / stride))
            return fail(PG_E_INVALID, "%s %u: sampled row %llu (x %u) past the %llu rows of contig %u", noun, i,
                        (unsigned long long)(ends[i] - 1), stride, (unsigned long long)nrows, contig[i]);
        se[i] = step == 1 ? a.out_off : a.out100_off;
        se[n + i] = starts[i];
        se[2 * (size_t)n + i] = ends[i];
        w.longest = std::max(w.longest, ends[i] - starts[i]);
    }
    return PG_OK;
}
// the bits of word d of a genome mask that are genomes: the bits at and past N never count
uint32_t pg::valid_word(uint32_t N, uint32_t d) { return N - 32 * d >= 32 ? 0xFFFFFFFFu : (1u << (N - 32 * d)) - 1u; }
// a caller's genome mask as ceil(N / 32) clamped words; a NULL pointer stands for if_null in every word
std::vector<uint32_t> pg::mask_words(uint32_t N, const uint32_t *words, uint32_t if_null) {
    std::vector<uint32_t> out((N + 31) / 32);
    for (uint32_t d = 0; d < out.size(); ++d) out[d] = (words ? words[d] : if_null) & valid_word(N, d);
    return out;
}
// pieces of a window for a (windows, pieces) grid: about 32 K sampled rows each for the longest window, then doubled (up to
// cap) while the grid has fewer than 4096 blocks and a piece keeps more than 4096 rows
uint32_t pg::pieces_for(uint64_t longest, uint32_t nwin, uint32_t cap) {
    uint32_t pieces = (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, longest / 32768));
    while (pieces < cap && (uint64_t)nwin * pieces < 4096 && (uint64_t)pieces * 4096 < longest) pieces *= 2;
    return pieces;
}
// the windows cut into chunks {window, first sampled row} of chunk_rows sampled rows each, a window's in order (an empty window
// has none); window i's chunks are [first[i], first[i + 1])
int pg::cut_chunks(const char *fn, uint32_t nwin, const uint64_t *starts, const uint64_t *ends, uint32_t chunk_rows,
                   std::vector<uint2> &chunks, std::vector<uint64_t> *first) {
    if (first) first->assign((size_t)nwin + 1, 0);
    for (uint32_t i = 0; i < nwin; ++i) {
        for (uint64_t c0 = starts[i]; c0 < ends[i]; c0 += chunk_rows) chunks.push_back(make_uint2(i, (uint32_t)c0));
        if (first) (*first)[i + 1] = chunks.size();
    }
    if (chunks.size() > 0x7FFFFFFFu)
        return fail(PG_E_INVALID, "%s: %zu chunks of %u sampled rows (at most 2^31 - 1 per call)", fn, chunks.size(), chunk_rows);
    return PG_OK;
}

// ---------------------------------------------------------------------------
// window statistics over finished rows resident in HBM
// ---------------------------------------------------------------------------
extern "C" int pg_result_window_stats(pg_result *r, uint32_t idx, int step, uint32_t nwin, const uint64_t *starts,
                                      const uint64_t *ends, uint64_t *hist, uint64_t *colsums) {
    PG_API_BEGIN
    if (!r || (nwin && (!starts || !ends || !hist))) return fail(PG_E_INVALID, "pg_result_window_stats: NULL argument");
    if (idx >= r->ad.size()) return fail(PG_E_INVALID, "contig %u out of range", idx);
    if (int e = check_step(r, step)) return e;
    if (!r->ev_ok) return fail(PG_E_INVALID, "pg_anchor_run has not been called on this result");
    if (nwin == 0) return PG_OK;
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    const uint32_t N = r->N;
    const AnchorDesc &a = r->ad[idx];
    const uint8_t *rows = step == 1 ? r->d_out1 + a.out_off : r->d_out100 + a.out100_off;
    const uint64_t nrows = step == 1 ? (uint64_t)a.nkmers : r->nrows100[idx];
    uint64_t longest = 0;
    for (uint32_t i = 0; i < nwin; ++i)
        if (ends[i] > starts[i]) longest = std::max(longest, std::min(ends[i], nrows) - std::min(starts[i], nrows));
    const uint32_t pieces = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, longest / 32768));
    DevBuf<uint64_t> d_se;
    DevBuf<unsigned long long> d_out;
    const size_t nh = (size_t)nwin * (N + 1), nc = colsums ? (size_t)nwin * N : 0;
    hipError_t e = d_se.alloc((size_t)nwin * 2);
    if (e == hipSuccess) e = d_out.alloc(nh + nc);
    if (e == hipSuccess) e = hipMemcpyAsync(d_se.get(), starts, (size_t)nwin * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_se.get() + nwin, ends, (size_t)nwin * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, (nh + nc) * 8, st);
    if (e == hipSuccess)
        e = launch_window_stats(st, N, rows, nrows, nwin, pieces, d_se.get(), d_se.get() + nwin, d_out.get(),
                                colsums ? d_out.get() + nh : nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(hist, d_out.get(), nh * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && colsums) e = hipMemcpyAsync(colsums, d_out.get() + nh, nc * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_window_stats: %s", hipGetErrorString(e));
    return PG_OK;
    PG_API_END
}

// masked per-bin column sums over sampled rows (call_introgressions.py: bitmap_to_bins): one launch for bins of any of
// the result's contigs
extern "C" int pg_result_bin_colsums(pg_result *r, int step, uint32_t stride, uint32_t nbins, const uint32_t *contig,
                                     const uint64_t *starts, const uint64_t *ends, const uint32_t *keep_words, int omit_fixed,
                                     uint64_t *cs_out, uint64_t *kept_out) {
    PG_API_BEGIN
    if (!r || (nbins && (!contig || !starts || !ends || !cs_out || !kept_out)))
        return fail(PG_E_INVALID, "pg_result_bin_colsums: NULL argument");
    if (int e = check_window_call(r, step, stride, nbins, "pg_result_bin_colsums", "bins")) return e;
    const uint32_t N = r->N;
    if (N < 1 || N > 4096) return fail(PG_E_INVALID, "pg_result_bin_colsums: %u genomes (1 to 4096)", N);
    Windows w;
    if (int e = gather_windows(r, step, stride, nbins, contig, starts, ends, "bin", w)) return e;
    const std::vector<uint32_t> kw = mask_words(N, keep_words, 0u);  // (NULL: no keep mask)
    if (nbins == 0) return PG_OK;
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    const uint32_t pieces = pieces_for(w.longest, nbins, 256);
    DevBuf<uint32_t> d_kw;
    DevBuf<unsigned long long> d_out;
    const size_t nc = (size_t)nbins * N;
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_kw.upload(kw, st);
    if (e == hipSuccess) e = d_out.alloc(nc + nbins);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, (nc + nbins) * 8, st);
    if (e == hipSuccess)
        e = launch_bin_colsums(st, N, step == 1 ? r->d_out1 : r->d_out100, stride, nbins, pieces, w.base(), w.starts(), w.ends(),
                               d_kw.get(), omit_fixed ? 1u : 0u, d_out.get(), d_out.get() + nc);
    if (e == hipSuccess) e = hipMemcpyAsync(cs_out, d_out.get(), nc * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(kept_out, d_out.get() + nc, (size_t)nbins * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_bin_colsums: %s", hipGetErrorString(e));
    return PG_OK;
    PG_API_END
}

// pair counts over sampled rows (the matrix behind view.py:751-764's tree of the genomes over a region): one launch for
// windows of any of the result's contigs
extern "C" int pg_result_pair_counts(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                                     const uint64_t *starts, const uint64_t *ends, uint64_t *pairs_out) {
    PG_API_BEGIN
    if (!r || (nwin && (!contig || !starts || !ends || !pairs_out)))
        return fail(PG_E_INVALID, "pg_result_pair_counts: NULL argument");
    if (int e = check_window_call(r, step, stride, nwin, "pg_result_pair_counts", "windows")) return e;
    const uint32_t N = r->N;
    if (N < 1 || N > PAIRS_MAX_GENOMES)
        return fail(PG_E_INVALID, "pg_result_pair_counts: %u genomes (the pair counts take 1 to %u)", N, PAIRS_MAX_GENOMES);
    Windows w;
    if (int e = gather_windows(r, step, stride, nwin, contig, starts, ends, "window", w)) return e;
    if (nwin == 0) return PG_OK;
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    // up to 2048 pieces, not bin_colsums' 256: a lone window of 32 M rows in 256 pieces leaves three quarters of the SIMDs' wave
    // slots empty (3.3 ms, in 2048 pieces as here); a piece keeps more than 4096 rows as it ends with up to N^2 / 2 atomics
    const uint32_t pieces = pieces_for(w.longest, nwin, 2048);
    DevBuf<unsigned long long> d_out;
    const size_t nc = (size_t)nwin * N * N;
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_out.alloc(nc);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, nc * 8, st);
    if (e == hipSuccess)
        e = launch_pair_counts(st, N, step == 1 ? r->d_out1 : r->d_out100, stride, nwin, pieces, w.base(), w.starts(), w.ends(),
                               d_out.get());
    if (e == hipSuccess) e = hipMemcpyAsync(pairs_out, d_out.get(), nc * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_pair_counts: %s", hipGetErrorString(e));
    // the kernel counts the pairs on and above the diagonal: the matrix is symmetric
    for (size_t i = 0; i < nwin; ++i) {
        uint64_t *m = pairs_out + i * N * N;
        for (uint32_t a = 0; a < N; ++a)
            for (uint32_t b = a + 1; b < N; ++b) m[(size_t)b * N + a] = m[(size_t)a * N + b];
    }
    return PG_OK;
    PG_API_END
}

// pattern runs over sampled rows (scripts/query_index.py's "custom" branch: the rows where these genomes' bits are set and
// those genomes' are not): a count launch over the chunks of all windows, the scans of their counts on the host, and — when
// the runs fit the caller's arrays — an emit launch
extern "C" int pg_result_find_runs(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                                   const uint64_t *starts, const uint64_t *ends, const uint32_t *have_words,
                                   const uint32_t *lack_words, uint32_t min_have, uint32_t max_lack, uint64_t cap,
                                   uint32_t *run_start, uint32_t *run_end, uint64_t *nruns_out, uint64_t *matched_out,
                                   uint64_t *total_out) {
    PG_API_BEGIN
    if (!r || !total_out || (nwin && (!contig || !starts || !ends || !nruns_out || !matched_out)) || (cap && (!run_start || !run_end)))
        return fail(PG_E_INVALID, "pg_result_find_runs: NULL argument");
    if (int e = check_window_call(r, step, stride, nwin, "pg_result_find_runs", "windows")) return e;
    const uint32_t N = r->N;
    if (N < 1 || N > FIND_MAX_GENOMES) return fail(PG_E_INVALID, "pg_result_find_runs: %u genomes (1 to %u)", N, FIND_MAX_GENOMES);
    Windows w;
    if (int e = gather_windows(r, step, stride, nwin, contig, starts, ends, "window", w)) return e;
    *total_out = 0;
    if (nwin == 0) return PG_OK;
    // the masks, have then lack: a NULL pointer is the empty set
    const uint32_t ndw = (N + 31) / 32;
    std::vector<uint32_t> mw = mask_words(N, have_words, 0u);
    const std::vector<uint32_t> lw = mask_words(N, lack_words, 0u);
    mw.insert(mw.end(), lw.begin(), lw.end());
    for (uint32_t i = 0; i < nwin; ++i) nruns_out[i] = matched_out[i] = 0;
    std::vector<uint2> chunks;
    std::vector<uint64_t> first;
    if (int e = cut_chunks("pg_result_find_runs", nwin, starts, ends, FIND_CHUNK, chunks, &first)) return e;
    if (chunks.empty()) return PG_OK;
    const uint32_t nchunks = (uint32_t)chunks.size();
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    const uint8_t *rows = step == 1 ? r->d_out1 : r->d_out100;
    DevBuf<uint32_t> d_mw;
    DevBuf<uint2> d_chunks;
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_mw.upload(mw, st);
    if (e == hipSuccess) e = d_chunks.upload(chunks, st);
    if (e != hipSuccess) {
        hipStreamSynchronize(st);  // (the uploads' sources go with this scope)
        return fail(PG_E_HIP, "pg_result_find_runs: %s", hipGetErrorString(e));
    }
    const auto launch = [&](uint4 *counts, const ulonglong2 *offs, uint64_t n, uint32_t *words, uint8_t *) {
        return launch_find_runs(st, N, rows, stride, w.base(), w.starts(), w.ends(), d_chunks.get(), nchunks, d_mw.get(), d_mw.get() + ndw,
                                min_have, max_lack, counts, offs, n, words, words + n);
    };
    RunsOut out;  // all runs or none: start and end (a run's window is told by nruns_out)
    out.nwords = 2, out.cap = cap;
    out.words[0] = run_start, out.words[1] = run_end;
    uint64_t sums[2];
    return runs_two_pass(r->ctx, "pg_result_find_runs", "window", nwin, first.data(), nchunks, launch, out, nruns_out, matched_out, total_out,
                         sums, nullptr);
    PG_API_END
}

// exact k nearest neighbours among the rows of a host matrix (the neighbour graph of index.py:1131-1137's umap.UMAP): the
// rows of every segment are cut into tiles of query rows, one block each, and all segments share one launch
extern "C" int pg_knn_rows(pg_ctx *ctx, const float *X, uint64_t n, uint32_t ncols, uint32_t k, const uint64_t *seg,
                           uint32_t nseg, int32_t *idx_out, float *d2_out) {
    PG_API_BEGIN
    if (k < 1 || k > KNN_MAX_K) return fail(PG_E_INVALID, "pg_knn_rows: k = %u (1 to %u neighbours)", k, KNN_MAX_K);
    if (ncols < 1 || ncols > KNN_MAX_COLS) return fail(PG_E_INVALID, "pg_knn_rows: %u columns (1 to %u)", ncols, KNN_MAX_COLS);
    if (!ctx || (n && (!X || !idx_out || !d2_out))) return fail(PG_E_INVALID, "pg_knn_rows: NULL argument");
    if (n > 0x7FFFFFFFull) return fail(PG_E_INVALID, "pg_knn_rows: %llu rows (row numbers are 31 bits)", (unsigned long long)n);
    const uint64_t whole[2] = {0, n};
    if (!seg) {
        seg = whole;
        nseg = 1;
    }
    if (nseg > 0x7FFFFFFFu) return fail(PG_E_INVALID, "pg_knn_rows: %u segments", nseg);
    if (seg[0] != 0 || seg[nseg] != n)
        return fail(PG_E_INVALID, "pg_knn_rows: the segments must run from row 0 to row %llu, not %llu to %llu",
                    (unsigned long long)n, (unsigned long long)seg[0], (unsigned long long)seg[nseg]);
    for (uint32_t s = 0; s < nseg; ++s)
        if (seg[s] > seg[s + 1])
            return fail(PG_E_INVALID, "pg_knn_rows: segment offsets not ascending (%llu before %llu at segment %u)",
                        (unsigned long long)seg[s], (unsigned long long)seg[s + 1], s);
    if (n == 0) return PG_OK;
    // tiles of 256 query rows; of 64 — one wave per block — while 256 would leave the grid short of two blocks per CU
    uint64_t t256 = 0;
    for (uint32_t s = 0; s < nseg; ++s) t256 += (seg[s + 1] - seg[s] + 255) / 256;
    const uint32_t threads = t256 < 512 ? 64 : 256;
    std::vector<uint32_t> tiles;
    for (uint32_t s = 0; s < nseg; ++s)
        for (uint64_t r = seg[s]; r < seg[s + 1]; r += threads) {
            const uint32_t t[4] = {(uint32_t)r, (uint32_t)std::min<uint64_t>(threads, seg[s + 1] - r), (uint32_t)seg[s],
                                   (uint32_t)seg[s + 1]};
            tiles.insert(tiles.end(), t, t + 4);
        }
    const uint32_t ntiles = (uint32_t)(tiles.size() / 4);
    if (int e = use_device(ctx)) return e;
    hipStream_t st = ctx->stream;
    DevBuf<float> d_x, d_d2;
    DevBuf<int32_t> d_idx;
    DevBuf<uint32_t> d_tiles;
    const size_t xb = (size_t)n * ncols * 4, ob = (size_t)n * k * 4;
    hipError_t e = d_x.alloc((size_t)n * ncols);
    if (e == hipSuccess) e = d_idx.alloc((size_t)n * k);
    if (e == hipSuccess) e = d_d2.alloc((size_t)n * k);
    if (e == hipSuccess) e = d_tiles.alloc(tiles.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_x.get(), X, xb, hipMemcpyDefault, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tiles.get(), tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_knn_rows(st, d_x.get(), ncols, k, d_tiles.get(), ntiles, threads, d_idx.get(), d_d2.get());
    if (e == hipSuccess) e = hipMemcpyAsync(idx_out, d_idx.get(), ob, hipMemcpyDefault, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d2_out, d_d2.get(), ob, hipMemcpyDefault, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_knn_rows: %s", hipGetErrorString(e));
    return PG_OK;
    PG_API_END
}
