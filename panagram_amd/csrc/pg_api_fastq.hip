// pg_api_fastq.hip — host side of the C-ABI: FASTQ text to a sequence set of one contig (pg_fastq.hip).  A unit of its own beside
// pg_api_seqset.hip, whose handle it fills.
#include "pg_host.h"

extern "C" int pg_seqset_from_fastq(pg_ctx *ctx, const void *text, uint64_t nbytes, pg_seqset **out, uint64_t *nreads, uint64_t *consumed) {
    PG_API_BEGIN
    if (!ctx || !out || !nreads || !consumed || (nbytes && !text)) return fail(PG_E_INVALID, "pg_seqset_from_fastq: NULL argument");
    const uint64_t ntiles64 = (nbytes + FASTQ_TILE - 1) / FASTQ_TILE;
    if (ntiles64 > 0x7FFFFFFFull) return fail(PG_E_INVALID, "pg_seqset_from_fastq: %llu bytes of text (below 2^43 per call)", (unsigned long long)nbytes);
    const uint32_t ntiles = (uint32_t)ntiles64;
    if (int r = use_device(ctx)) return r;
    *out = nullptr;
    *nreads = *consumed = 0;
    place_ms()[0] = 0;
    hipStream_t st = ctx->stream;
    uint64_t summary[3] = {0, ~0ull, 0}, fin[2] = {0, 0};
    DevBuf<uint8_t> d_text, d_ascii;
    DevBuf<FastqTileSum> d_sums;
    DevBuf<ulonglong2> d_bases;
    DevBuf<uint64_t> d_small;  // summary[3], fin[2]
    float ms_scan = 0, ms_join = 0, ms_pack = 0;
    if (ntiles) {
        // (the text is readable, and zero, up to the tiles' end and 16 bytes beyond)
        const uint64_t tcap = ntiles64 * FASTQ_TILE + 16;
        LaunchTimer tm(&ms_scan);
        hipError_t e = d_text.alloc(tcap);
        if (e == hipSuccess) e = d_ascii.alloc(nbytes + 16);  // (every output byte is one of the text's)
        if (e == hipSuccess) e = d_sums.alloc(ntiles);
        if (e == hipSuccess) e = d_bases.alloc(ntiles);
        if (e == hipSuccess) e = d_small.alloc(5);
        if (e == hipErrorOutOfMemory) return fail(PG_E_CAPACITY, "pg_seqset_from_fastq: no memory for %llu bytes of text", (unsigned long long)nbytes);
        if (e == hipSuccess) e = hipMemsetAsync(d_text.get() + nbytes, 0, tcap - nbytes, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_text.get(), text, nbytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_small.get(), 0, 5 * 8, st);
        if (e == hipSuccess) e = tm.start(st);
        if (e == hipSuccess) e = launch_fastq_scan(st, d_text.get(), nbytes, ntiles, d_sums.get(), d_bases.get(), d_small.get());
        if (e == hipSuccess) e = tm.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(summary, d_small.get(), 3 * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(PG_E_HIP, "pg_seqset_from_fastq: %s", hipGetErrorString(e));
        tm.read();
    }
    const uint64_t nrec = summary[0] / 4;
    if (summary[1] != ~0ull)
        return fail(PG_E_INVALID, "pg_seqset_from_fastq: record %llu: its %s", (unsigned long long)(summary[1] / 4),
                    (summary[1] & 3) == 0 ? "header line does not begin with '@'" : "separator line does not begin with '+'");
    if (nrec) {
        LaunchTimer tm(&ms_join);
        hipError_t e = tm.start(st);
        if (e == hipSuccess)
            e = launch_fastq_join(st, d_text.get(), nbytes, ntiles, d_bases.get(), 4 * nrec, d_ascii.get(), nbytes, d_small.get() + 3);
        if (e == hipSuccess) e = tm.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(fin, d_small.get() + 3, 2 * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(PG_E_HIP, "pg_seqset_from_fastq: %s", hipGetErrorString(e));
        tm.read();
        if (fin[0] > nbytes || fin[1] > nbytes || fin[1] == 0)
            return fail(PG_E_HIP, "pg_seqset_from_fastq: %llu bases, %llu bytes consumed of %llu", (unsigned long long)fin[0],
                        (unsigned long long)fin[1], (unsigned long long)nbytes);
    }
    // one contig: of length 0 when the text holds no complete record
    const uint64_t len = fin[0];
    pg_seqset *s = nullptr;
    if (int r = pg_seqset_create(ctx, 1, &len, &s)) return r;
    s->names.push_back(std::string());
    if (len) {
        LaunchTimer tm(&ms_pack);
        hipError_t e = tm.start(st);
        int r = e == hipSuccess ? pg_seqset_load_dev(s, 0, d_ascii.get(), len) : PG_OK;
        if (e == hipSuccess && r == PG_OK) e = tm.stop(st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the ASCII goes with this call)
        if (e != hipSuccess || r != PG_OK) {
            (void)hipStreamSynchronize(st);
            pg_seqset_destroy(s);
            return r != PG_OK ? r : fail(PG_E_HIP, "pg_seqset_from_fastq: %s", hipGetErrorString(e));
        }
        tm.read();
    }
    place_ms()[0] = ms_scan + ms_join + ms_pack;
    *out = s;
    *nreads = nrec;
    *consumed = fin[1];
    return PG_OK;
    PG_API_END
}
