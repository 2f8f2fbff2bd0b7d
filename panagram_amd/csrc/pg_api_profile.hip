// pg_api_profile.hip — host side of the C-ABI: the presence profile of windows of a result's finished rows (a window query: it
// opens with pg_api_query.hip's shared prologue, as pg_api_gaps.hip does).
#include "pg_host.h"
#include "pg_profile_host.h"

static_assert(sizeof(ProfilePartial) == 2 * sizeof(uint4) && sizeof(ProfileRows) == sizeof(uint2), "the kernel's partials, field by field");

// per window and genome: hits, runs, longest, first, end, covered of the genome's column over the window's rows; per window the
// rows with every selected genome's bit and with none.  One launch over the chunks of all windows, one download of the chunks'
// partials, their stitch on the host.
extern "C" int pg_result_presence_profile(pg_result *r, uint32_t nwin, const uint32_t *contig, const uint64_t *starts,
                                          const uint64_t *ends, const uint32_t *select_words, uint32_t *profile_out,
                                          uint32_t *rows_out) {
    PG_API_BEGIN
    if (!r || (nwin && (!contig || !starts || !ends || !profile_out || !rows_out)))
        return fail(PG_E_INVALID, "pg_result_presence_profile: NULL argument");
    if (int e = check_window_call(r, 1, 1, nwin, "pg_result_presence_profile", "windows")) return e;
    const uint32_t N = r->N;
    if (N < 1 || N > PROFILE_MAX_GENOMES)
        return fail(PG_E_INVALID, "pg_result_presence_profile: %u genomes (1 to %u)", N, PROFILE_MAX_GENOMES);
    if (r->k < 1) return fail(PG_E_INVALID, "pg_result_presence_profile: k = %d", r->k);
    const uint32_t k = (uint32_t)r->k;
    for (uint32_t i = 0; i < nwin; ++i)
        if (ends[i] > starts[i] && ends[i] - starts[i] + (k - 1) >= (1ull << 32))
            return fail(PG_E_INVALID, "window %u: %llu rows of k = %u are %llu bases (below 2^32 per window)", i,
                        (unsigned long long)(ends[i] - starts[i]), k, (unsigned long long)(ends[i] - starts[i] + (k - 1)));
    Windows w;
    if (int e = gather_windows(r, 1, 1, nwin, contig, starts, ends, "window", w)) return e;
    if (nwin == 0) return PG_OK;
    const std::vector<uint32_t> sw = mask_words(N, select_words, 0xFFFFFFFFu);  // (NULL: every genome)
    std::fill(profile_out, profile_out + (size_t)nwin * N * PROFILE_FIELDS, 0u);
    std::fill(rows_out, rows_out + (size_t)nwin * 2, 0u);
    std::vector<uint2> chunks;
    std::vector<uint64_t> first;
    if (int e = cut_chunks("pg_result_presence_profile", nwin, starts, ends, PROFILE_CHUNK, chunks, &first)) return e;
    bool any = false;
    for (uint32_t d : sw) any = any || d;
    if (chunks.empty() || !any) return PG_OK;  // (every window empty / no column selected: zeros)
    const uint32_t nchunks = (uint32_t)chunks.size();
    if (int e = use_device(r->ctx)) return e;
    if (int e = join_result(r)) return e;
    hipStream_t st = r->ctx->stream;
    // one buffer, one download: [nchunks][N] partials of two uint4 each, then [nchunks] {all, none} (8 bytes: half a uint4)
    const size_t npart = (size_t)nchunks * N * 2, nq = npart + ((size_t)nchunks + 1) / 2;
    DevBuf<uint32_t> d_sw;
    DevBuf<uint2> d_chunks;
    DevBuf<uint4> d_out;
    hipError_t e = w.upload(st);
    if (e == hipSuccess) e = d_sw.upload(sw, st);
    if (e == hipSuccess) e = d_chunks.upload(chunks, st);
    if (e == hipSuccess) e = d_out.alloc(nq);
    if (e == hipSuccess)
        e = launch_presence_profile(st, N, r->d_out1, w.base(), w.ends(), d_chunks.get(), nchunks, d_sw.get(), k, d_out.get(),
                                    reinterpret_cast<uint2 *>(d_out.get() + npart));
    std::vector<uint4> h_out(nq);
    if (e == hipSuccess) e = hipMemcpyAsync(h_out.data(), d_out.get(), nq * sizeof(uint4), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_result_presence_profile: %s", hipGetErrorString(e));
    profile_stitch(N, nwin, starts, ends, first.data(), PROFILE_CHUNK, reinterpret_cast<const ProfilePartial *>(h_out.data()),
                   reinterpret_cast<const ProfileRows *>(h_out.data() + npart), sw.data(), k, profile_out, rows_out);
    return PG_OK;
    PG_API_END
}
