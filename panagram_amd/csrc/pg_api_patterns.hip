// pg_api_patterns.hip — host side of the C-ABI: the presence/absence pattern spectrum of a result's finished rows.
#include "pg_host.h"

static constexpr uint64_t PATTERN_CAP_LIMIT = 1ull << 30;  // (a table of 2^31 slots: 32 GiB)

// pattern spectrum over sampled rows (query_bitmap + DataFrame.value_counts() without the frame): one launch over the chunks of
// all windows into a hash table of at least 2 * cap slots, then — when no more than cap distinct patterns showed — the table's
// download and its sort by key on the host
extern "C" int pg_result_pattern_counts(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                                        const uint64_t *starts, const uint64_t *ends, const uint32_t *select_words, uint64_t cap,
                                        uint64_t *keys_out, uint64_t *counts_out, uint64_t *ndistinct_out, uint64_t *rows_out,
                                        int *exceeded_out) {
    PG_API_BEGIN
    if (!r || !ndistinct_out || !rows_out || !exceeded_out || (nwin && (!contig || !starts || !ends)) || (cap && (!keys_out || !counts_out)))
        return fail(PG_E_INVALID, "pg_result_pattern_counts: NULL argument");
    if (int e = check_window_call(r, step, stride, nwin, "pg_result_pattern_counts", "windows")) return e;
    if (cap > PATTERN_CAP_LIMIT)
        return fail(PG_E_INVALID, "pg_result_pattern_counts: room for %llu patterns asked (at most 2^30 per call)", (unsigned long long)cap);
    const uint32_t N = r->N;
    if (N < 1 || N > PATTERN_MAX_GENOMES)
        return fail(PG_E_INVALID, "pg_result_pattern_counts: %u genomes (1 to %u)", N, PATTERN_MAX_GENOMES);
    const uint32_t ndw = (N + 31) / 32;
    const std::vector<uint32_t> sw = mask_words(N, select_words, 0xFFFFFFFFu);  // (NULL: every genome)
    uint32_t m = 0;
    for (uint32_t d = 0; d < ndw; ++d) m += (uint32_t)__builtin_popcount(sw[d]);
    if (m == 0) return fail(PG_E_INVALID, "pg_result_pattern_counts: no genome selected");
    if (m > 64)
        return fail(PG_E_INVALID, "pg_result_pattern_counts: %u genomes selected (a pattern takes 1 to 64: select fewer)", m);
    bool low_columns = true;  // the selection is columns 0..m-1: a key is the row's first bytes
    for (uint32_t d = 0; d < ndw; ++d) low_columns = low_columns && sw[d] == (m <= 32 * d ? 0u : valid_word(m, d));
    Windows w;
    if (int e = gather_windows(r, step, stride, nwin, contig, starts, ends, "window", w)) return e;
    uint64_t total = 0;
    for (uint32_t i = 0; i < nwin; ++i) total += ends[i] - starts[i];
    *rows_out = total;
    *ndistinct_out = 0;
    *exceeded_out = 0;
    if (total == 0) return PG_OK;
    std::vector<uint2> chunks;
    if (int e = cut_chunks("pg_result_pattern_counts", nwin, starts, ends, PATTERN_CHUNK, chunks)) return e;
    const uint32_t nchunks = (uint32_t)chunks.size();
    uint64_t slots = 1024;
    while (slots < 2 * cap) slots *= 2;
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    DevBuf<uint32_t> d_sw;
    DevBuf<uint2> d_chunks;
    DevBuf<unsigned long long> d_keys, d_cnt;  // d_cnt: the counts, then the four counters
    unsigned long long ctr[4] = {0, 0, 0, 0};
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_sw.upload(sw, st);
    if (e == hipSuccess) e = d_chunks.upload(chunks, st);
    if (e == hipSuccess) e = d_keys.alloc(slots);
    if (e == hipSuccess) e = d_cnt.alloc(slots + 4);
    if (e == hipSuccess) e = hipMemsetAsync(d_keys.get(), 0xFF, slots * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt.get(), 0, (slots + 4) * 8, st);
    if (e == hipSuccess)
        e = launch_pattern_counts(st, N, step == 1 ? r->d_out1 : r->d_out100, stride, w.base(), w.ends(), d_chunks.get(), nchunks,
                                  d_sw.get(), m, low_columns, cap, d_keys.get(), d_cnt.get(), slots, d_cnt.get() + slots);
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_cnt.get() + slots, sizeof ctr, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_pattern_counts: %s", hipGetErrorString(e));
    // ctr: {slots claimed, rows dropped at a full table, rows of the all-ones key (64 genomes selected: kept out of the table)}
    const uint64_t ndistinct = ctr[0] + (ctr[2] ? 1 : 0);
    if (ndistinct > cap || ctr[1]) {
        *exceeded_out = 1;
        return PG_OK;
    }
    std::vector<uint64_t> hk(slots), hc(slots);
    e = hipMemcpyAsync(hk.data(), d_keys.get(), slots * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), d_cnt.get(), slots * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_pattern_counts: %s", hipGetErrorString(e));
    std::vector<std::pair<uint64_t, uint64_t>> found;
    found.reserve(ndistinct);
    uint64_t seen = ctr[2];
    for (uint64_t s = 0; s < slots; ++s)
        if (hk[s] != ~0ull) {
            found.emplace_back(hk[s], hc[s]);
            seen += hc[s];
        }
    if (found.size() != ctr[0] || seen != total)  // (every sampled row is in exactly one pattern)
        return fail(PG_E_HIP, "pg_result_pattern_counts: %zu patterns of %llu rows in the table, %llu claimed and %llu rows read",
                    found.size(), (unsigned long long)seen, ctr[0], (unsigned long long)total);
    std::sort(found.begin(), found.end());
    if (ctr[2]) found.emplace_back(~0ull, ctr[2]);  // (the largest key there is)
    for (size_t i = 0; i < found.size(); ++i) {
        keys_out[i] = found[i].first;
        counts_out[i] = found[i].second;
    }
    *ndistinct_out = found.size();
    return PG_OK;
    PG_API_END
}
