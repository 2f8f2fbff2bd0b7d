// pg_api_tablestats.hip — host side of the C-ABI: shared distinct k-mer counts of a pan table (k_table_pair_counts).
#include "pg_host.h"

// one pass over the table's slots on the context's stream, behind whatever launch last wrote the table; the four outputs are
// accumulated in one zeroed device buffer: pairs [N * N], occ [N + 1], priv [N], nkeys [1]
extern "C" int pg_table_pair_counts(pg_table *t, uint64_t *pairs, uint64_t *occ, uint64_t *priv, uint64_t *nkeys) {
    PG_API_BEGIN
    if (!t || !pairs) return fail(PG_E_INVALID, "pg_table_pair_counts: NULL argument");
    if (t->ngenomes < 1 || t->ngenomes > (int)PAIRS_MAX_GENOMES)
        return fail(PG_E_INVALID, "pg_table_pair_counts: %d genomes (the pair counts take 1 to %u)", t->ngenomes, PAIRS_MAX_GENOMES);
    const uint32_t N = (uint32_t)t->ngenomes;
    const size_t npairs = (size_t)N * N, ntotal = npairs + (N + 1) + N + 1;
    if (int e = use_device(t->ctx)) return e;
    TABLE_WRITER(t);  // (a reader: it only keeps a second host thread's re-hash from freeing the lines under the kernel)
    hipStream_t st = t->ctx->stream;
    DevBuf<unsigned long long> d_out;
    std::vector<uint64_t> h(ntotal, 0);
    hipError_t e = d_out.alloc(ntotal);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, ntotal * 8, st);
    for (auto &s : t->subs)
        if (e == hipSuccess)
            e = launch_table_pair_counts(st, s.d, N, d_out.get(), d_out.get() + npairs, d_out.get() + npairs + N + 1,
                                         d_out.get() + npairs + 2 * (size_t)N + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_out.get(), ntotal * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(PG_E_HIP, "pg_table_pair_counts: %s", hipGetErrorString(e));
    // the kernel counts the pairs on and above the diagonal: the matrix is symmetric
    for (uint32_t a = 0; a < N; ++a)
        for (uint32_t b = a; b < N; ++b) pairs[(size_t)a * N + b] = pairs[(size_t)b * N + a] = h[(size_t)a * N + b];
    if (occ) std::copy(h.begin() + npairs, h.begin() + npairs + N + 1, occ);
    if (priv) std::copy(h.begin() + npairs + N + 1, h.begin() + npairs + 2 * (size_t)N + 1, priv);
    if (nkeys) *nkeys = h[ntotal - 1];
    return PG_OK;
    PG_API_END
}
