// pg_api_seqset.hip — host side of the C-ABI: sequence sets, the FASTA parser included.
#include "pg_host.h"

// ---------------------------------------------------------------------------
// seqset
// ---------------------------------------------------------------------------
extern "C" int pg_seqset_create(pg_ctx *ctx, uint32_t ncontigs, const uint64_t *lens, pg_seqset **out) {
    PG_API_BEGIN
    if (!ctx || !out || (ncontigs && !lens)) return fail(PG_E_INVALID, "pg_seqset_create: NULL argument");
    if (int r = use_device(ctx)) return r;
    pg_seqset *s = new pg_seqset();
    s->ctx = ctx;
    ++ctx->refs;
    s->n = ncontigs;
    s->d_seqw = nullptr;
    s->d_nmw = nullptr;
    s->d_has_n = nullptr;
    s->d_desc = nullptr;
    s->d_stage = nullptr;
    s->stage_cap = 0;
    uint64_t off = 0;
    for (uint32_t i = 0; i < ncontigs; ++i) {
        SeqDesc d;
        d.len = lens[i];
        d.nwords = (lens[i] + 31) / 32 + 2;  // +2 zero words: the kernels read one word past a window
        d.seq_off = off;
        off += d.nwords;
        s->desc.push_back(d);
    }
    s->total_words = off;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    size_t nw = std::max<uint64_t>(off, 1), nc = std::max<uint32_t>(ncontigs, 1);
    if ((e = hipMalloc(reinterpret_cast<void **>(&s->d_seqw), nw * 8)) == hipSuccess &&
        (e = hipMalloc(reinterpret_cast<void **>(&s->d_nmw), nw * 4)) == hipSuccess &&
        (e = hipMalloc(reinterpret_cast<void **>(&s->d_has_n), nc * 4)) == hipSuccess &&
        (e = hipMalloc(reinterpret_cast<void **>(&s->d_desc), nc * sizeof(SeqDesc))) == hipSuccess &&
        (e = hipMemsetAsync(s->d_seqw, 0, nw * 8, st)) == hipSuccess &&
        (e = hipMemsetAsync(s->d_nmw, 0, nw * 4, st)) == hipSuccess &&
        (e = hipMemsetAsync(s->d_has_n, 0, nc * 4, st)) == hipSuccess) {
        if (ncontigs)
            e = hipMemcpyAsync(s->d_desc, s->desc.data(), ncontigs * sizeof(SeqDesc), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        pg_seqset_destroy(s);
        return fail(PG_E_HIP, "seqset allocation failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return PG_OK;
    PG_API_END
}

static void seqset_free(pg_seqset *s) {
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    hipFree(s->d_seqw);
    hipFree(s->d_nmw);
    hipFree(s->d_has_n);
    hipFree(s->d_desc);
    if (s->d_stage) hipFree(s->d_stage);
    pg_ctx *c = s->ctx;
    delete s;
    ctx_release(c);
}
void pg::seqset_release(pg_seqset *s) {
    if (--s->refs == 0 && s->dead) seqset_free(s);
}

extern "C" int pg_seqset_destroy(pg_seqset *s) {
    PG_API_BEGIN
    if (!s || s->dead) return PG_OK;
    s->dead = true;
    if (s->refs == 0) seqset_free(s);
    return PG_OK;
    PG_API_END
}

extern "C" int pg_seqset_load_dev(pg_seqset *s, uint32_t idx, const void *d_ascii, uint64_t len) {
    PG_API_BEGIN
    if (!s || (len && !d_ascii)) return fail(PG_E_INVALID, "pg_seqset_load_dev: NULL argument");
    if (idx >= s->n) return fail(PG_E_INVALID, "contig %u out of range (0..%u)", idx, s->n ? s->n - 1 : 0);
    const SeqDesc &d = s->desc[idx];
    if (len != d.len) return fail(PG_E_INVALID, "contig %u: length %llu != declared %llu", idx, (unsigned long long)len, (unsigned long long)d.len);
    if (int r = use_device(s->ctx)) return r;
    HIP_TRY(hipMemsetAsync(s->d_has_n + idx, 0, 4, s->ctx->stream));
    HIP_TRY(launch_pack(s->ctx->stream, d_ascii, len, s->d_seqw + d.seq_off, s->d_nmw + d.seq_off,
                        (len + 31) / 32, s->d_has_n + idx));
    return PG_OK;
    PG_API_END
}

extern "C" int pg_seqset_load_host(pg_seqset *s, uint32_t idx, const char *ascii, uint64_t len) {
    PG_API_BEGIN
    if (!s || (len && !ascii)) return fail(PG_E_INVALID, "pg_seqset_load_host: NULL argument");
    if (idx >= s->n) return fail(PG_E_INVALID, "contig %u out of range", idx);
    if (int r = use_device(s->ctx)) return r;
    if (len > s->stage_cap) {
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        if (s->d_stage) hipFree(s->d_stage);
        s->d_stage = nullptr;
        s->stage_cap = 0;
        size_t cap = (len + 4095) & ~(size_t)4095;
        HIP_TRY(hipMalloc(&s->d_stage, cap));
        s->stage_cap = cap;
    }
    if (len) HIP_TRY(hipMemcpyAsync(s->d_stage, ascii, len, hipMemcpyHostToDevice, s->ctx->stream));
    if (int r = pg_seqset_load_dev(s, idx, s->d_stage, len)) return r;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));  // staging buffer is reused by the next call
    return PG_OK;
    PG_API_END
}

// ---------------------------------------------------------------------------
// FASTA text -> seqset.  Host: locate the header lines (memchr over the text, '>' is rare).
// GPU: drop the white space of the sequence lines and pack (k_text_count/scan/pack).
// ---------------------------------------------------------------------------
static inline bool host_is_ws(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

extern "C" int pg_seqset_from_fasta(pg_ctx *ctx, const void *text_, uint64_t nbytes, pg_seqset **out) {
    PG_API_BEGIN
    if (!ctx || !out || (nbytes && !text_)) return fail(PG_E_INVALID, "pg_seqset_from_fasta: NULL argument");
    if (int r = use_device(ctx)) return r;
    const unsigned char *text = static_cast<const unsigned char *>(text_);
    // The text goes up while the host looks for the header lines: the copy out of pageable memory (the runtime stages it,
    // ~10 GB/s) and the memchr pass over the same bytes each take 6-10 ms per 100 MB, one after the other they were most
    // of what a genome's load costs.  The upload runs on a helper thread and a stream of its own; the text buffer comes out of the context's buffer cache (one per genome of a pangenome, all about the
    // same size: freeing GBs is paid by the next big allocation).
    const uint64_t tcap = (nbytes + 4095) / 4096 * 4096 + 4096;
    uint8_t *d_text = nullptr;
    uint64_t text_cap = 0;
    hipError_t e_up = row_alloc(ctx, tcap, &d_text, &text_cap);
    if (e_up != hipSuccess) return fail(PG_E_HIP, "FASTA packing failed: %s", hipGetErrorString(e_up));
    struct Upload {  // (joined on every way out, also an exception's)
        std::thread th;
        ~Upload() {
            if (th.joinable()) th.join();
        }
    } up;
    struct TextGuard {  // (given back after the upload has been joined: declared after it would free it first)
        pg_ctx *c;
        uint8_t *p;
        uint64_t cap;
        Upload *u;
        ~TextGuard() {
            if (u->th.joinable()) u->th.join();
            row_free(c, p, cap);
        }
    } text_guard{ctx, d_text, text_cap, &up};
    auto upload = [&]() noexcept {
        if (hipSetDevice(ctx->device) != hipSuccess) {
            e_up = hipErrorInvalidDevice;
            return;
        }
        // (a stream of its own: several genomes may be loading at once — Index.load_inputs parses in its reader threads —
        // and the staging of a pageable copy is host work that runs in the calling thread)
        Stream us;
        e_up = us.create();
        if (e_up == hipSuccess) e_up = hipMemsetAsync(d_text + nbytes, 0, tcap - nbytes, us.get());
        if (e_up == hipSuccess && nbytes) e_up = hipMemcpyAsync(d_text, text, nbytes, hipMemcpyHostToDevice, us.get());
        if (e_up == hipSuccess) e_up = hipStreamSynchronize(us.get());
    };
    if (nbytes < (1u << 20)) {
        upload();  // (a small text: a thread and a stream per call cost more than the overlap brings)
    } else {
        try {
            up.th = std::thread(upload);
        } catch (const std::system_error &) {  // no thread to be had: the copy runs here, before the scan
            upload();
        }
    }
    struct Rec {
        std::string name;
        uint64_t s, e;
    };
    std::vector<Rec> recs;
    // A large text's header lines are looked for ON THE DEVICE once the text is there (k_text_headers): the host's memchr pass
    // over the same bytes runs at 20 GB/s — 10 ms per 200 MB, more than the DMA of a page-locked text takes (4 ms), and beside
    // the staging copy of a pageable one it competes for the same memory.  The few positions come back sorted; more than
    // HDR_CAP of them (a read set passed off as FASTA), or any error: the host looks for itself, as for small texts.
    constexpr uint32_t HDR_CAP = 1u << 16;
    std::vector<uint64_t> hdrs;
    bool have_hdrs = false;
    if (nbytes >= (4u << 20) && !getenv("PG_FASTA_HOST_SCAN")) {
        if (up.th.joinable()) up.th.join();
        DevBuf<uint64_t> d_hdr;
        DevBuf<uint32_t> d_nhdr;
        uint32_t nh = 0;
        if (e_up == hipSuccess && d_hdr.alloc(HDR_CAP) == hipSuccess && d_nhdr.alloc(1) == hipSuccess) {
            hipStream_t st = ctx->stream;
            if (launch_text_headers(st, d_text, nbytes, d_hdr.get(), HDR_CAP, d_nhdr.get()) == hipSuccess &&
                hipMemcpyAsync(&nh, d_nhdr.get(), 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && nh <= HDR_CAP) {
                hdrs.resize(nh);
                if (nh == 0 || hipMemcpy(hdrs.data(), d_hdr.get(), (size_t)nh * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                    std::sort(hdrs.begin(), hdrs.end());
                    have_hdrs = true;
                }
            }
        }
        (void)hipGetLastError();
    }
    size_t hdr_at = 0;
    // first header: at offset 0 or right after a newline; anything before it is ignored
    auto next_header = [&](uint64_t from) -> uint64_t {
        if (have_hdrs) {  // (asked for in ascending order)
            while (hdr_at < hdrs.size() && hdrs[hdr_at] < from) ++hdr_at;
            return hdr_at < hdrs.size() ? hdrs[hdr_at] : nbytes;
        }
        uint64_t p = from;
        while (p < nbytes) {
            const void *q = memchr(text + p, '>', nbytes - p);
            if (!q) return nbytes;
            p = (uint64_t)(static_cast<const unsigned char *>(q) - text);
            if (p == 0 || text[p - 1] == '\n') return p;
            ++p;
        }
        return nbytes;
    };
    uint64_t h = next_header(0);
    while (h < nbytes) {
        const void *q = memchr(text + h, '\n', nbytes - h);
        const uint64_t eol = q ? (uint64_t)(static_cast<const unsigned char *>(q) - text) : nbytes;
        uint64_t a = h + 1;
        while (a < eol && host_is_ws(text[a])) ++a;
        uint64_t b = a;
        while (b < eol && !host_is_ws(text[b])) ++b;
        Rec r;
        r.name.assign(reinterpret_cast<const char *>(text + a), b - a);
        r.s = std::min<uint64_t>(eol + 1, nbytes);
        const uint64_t hn = next_header(r.s);
        r.e = hn;
        recs.push_back(r);
        h = hn;
    }
    const uint32_t nrec = (uint32_t)recs.size();
    // upper-bound layout (text bytes >= bases): the packed planes can be laid out before counting
    std::vector<uint64_t> ub(nrec);
    std::vector<TextChunk> chunks;
    std::vector<uint64_t> chunk0(nrec + 1, 0);
    for (uint32_t i = 0; i < nrec; ++i) {
        ub[i] = recs[i].e - recs[i].s;
        chunk0[i] = chunks.size();
        for (uint64_t p = recs[i].s; p < recs[i].e;) {
            const uint64_t lim = std::min<uint64_t>(recs[i].e, (p / 4096 + 1) * 4096);
            TextChunk c;
            c.off = p;
            c.len = (uint32_t)(lim - p);
            c.rec = i;
            chunks.push_back(c);
            p = lim;
        }
    }
    chunk0[nrec] = chunks.size();
    pg_seqset *s = nullptr;
    if (int r = pg_seqset_create(ctx, nrec, ub.data(), &s)) return r;
    for (auto &r : recs) s->names.push_back(r.name);
    if (nrec == 0) {
        *out = s;
        return PG_OK;
    }
    hipStream_t st = ctx->stream;
    const uint64_t nch = chunks.size();
    DevBuf<TextChunk> d_chunks;
    DevBuf<uint64_t> d_chunk0, d_base, d_len;
    DevBuf<uint32_t> d_counts;
    std::vector<uint64_t> lens(nrec, 0);
    hipError_t e = d_chunks.alloc(std::max<uint64_t>(nch, 1));
    if (e == hipSuccess) e = d_chunk0.alloc(nrec + 1);
    if (e == hipSuccess) e = d_base.alloc(std::max<uint64_t>(nch, 1));
    if (e == hipSuccess) e = d_len.alloc(nrec);
    if (e == hipSuccess) e = d_counts.alloc(std::max<uint64_t>(nch, 1));
    if (e == hipSuccess) {
        if (up.th.joinable()) up.th.join();  // (the text is up — the helper waited for its stream)
        e = e_up;
    }
    if (e == hipSuccess && nch) e = hipMemcpyAsync(d_chunks.get(), chunks.data(), nch * sizeof(TextChunk), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_chunk0.get(), chunk0.data(), (nrec + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = launch_text_pack(st, d_text, d_chunks.get(), nch, d_chunk0.get(), nrec, d_counts.get(), d_base.get(), d_len.get(),
                             s->d_desc, s->d_seqw, s->d_nmw, s->d_has_n);
    if (e == hipSuccess) e = hipMemcpyAsync(lens.data(), d_len.get(), nrec * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        for (uint32_t i = 0; i < nrec; ++i) s->desc[i].len = lens[i];
        e = hipMemcpyAsync(s->d_desc, s->desc.data(), nrec * sizeof(SeqDesc), hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // (an error may have come back with kernels still queued on st that read the text buffer — the upload ran on a stream of
    // its own, nothing else orders them against the buffer's next user once it is back in the context's cache)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        pg_seqset_destroy(s);
        return fail(PG_E_HIP, "FASTA packing failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return PG_OK;
    PG_API_END
}

// one seqset holding contigs [first[i], first[i] + count[i]) of sets[i], in order (device-to-device copy of the packed
// planes); first == NULL: every contig of every set
static int seqset_concat(pg_ctx *ctx, const pg_seqset *const *sets, const uint32_t *first, const uint32_t *count,
                         uint32_t nsets, pg_seqset **out) {
    if (!ctx || !out || (nsets && !sets)) return fail(PG_E_INVALID, "pg_seqset_concat: NULL argument");
    std::vector<uint64_t> lens;
    for (uint32_t i = 0; i < nsets; ++i) {
        if (!sets[i] || sets[i]->ctx != ctx) return fail(PG_E_INVALID, "pg_seqset_concat: seqset %u is NULL or of another context", i);
        const uint32_t f = first ? first[i] : 0, n = first ? count[i] : sets[i]->n;
        if ((uint64_t)f + n > sets[i]->n) return fail(PG_E_INVALID, "pg_seqset_concat_ranges: contigs %u..%u of seqset %u out of range", f, f + n, i);
        for (uint32_t j = f; j < f + n; ++j) lens.push_back(sets[i]->desc[j].len);
    }
    pg_seqset *s = nullptr;
    if (int r = pg_seqset_create(ctx, (uint32_t)lens.size(), lens.data(), &s)) return r;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    // one gather launch for all contigs (a copy per plane and contig was 9 us each: 1.3 s for the 160 000 contigs of
    // eight fragmented assemblies); the job list goes up in one piece
    std::vector<SeqCopy> jobs;
    jobs.reserve(lens.size());
    uint64_t max_words = 0;
    uint32_t c = 0;
    for (uint32_t i = 0; i < nsets; ++i) {
        const pg_seqset *src = sets[i];
        const uint32_t f = first ? first[i] : 0, n = first ? count[i] : src->n;
        for (uint32_t j = f; j < f + n; ++j, ++c) {
            SeqCopy q;
            q.src_seqw = src->d_seqw;
            q.src_nmw = src->d_nmw;
            q.src_has_n = src->d_has_n + j;
            q.src_off = src->desc[j].seq_off;
            q.dst_off = s->desc[c].seq_off;
            q.nwords = std::min(src->desc[j].nwords, s->desc[c].nwords);
            max_words = std::max(max_words, q.nwords);
            jobs.push_back(q);
            s->names.push_back(j < src->names.size() ? src->names[j] : std::string());
        }
    }
    DevBuf<SeqCopy> d_jobs;
    if (!jobs.empty()) {
        e = d_jobs.alloc(jobs.size());
        if (e == hipSuccess) e = hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(SeqCopy), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launch_seq_gather(st, d_jobs.get(), (uint32_t)jobs.size(), max_words, s->d_seqw, s->d_nmw, s->d_has_n);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        pg_seqset_destroy(s);
        return fail(PG_E_HIP, "pg_seqset_concat: %s", hipGetErrorString(e));
    }
    *out = s;
    return PG_OK;
}

extern "C" int pg_seqset_concat(pg_ctx *ctx, const pg_seqset *const *sets, uint32_t nsets, pg_seqset **out) {
    PG_API_BEGIN
    return seqset_concat(ctx, sets, nullptr, nullptr, nsets, out);
    PG_API_END
}

extern "C" int pg_seqset_concat_ranges(pg_ctx *ctx, const pg_seqset *const *sets, const uint32_t *first_contig,
                                       const uint32_t *ncontigs, uint32_t nsets, pg_seqset **out) {
    PG_API_BEGIN
    if (nsets && (!first_contig || !ncontigs)) return fail(PG_E_INVALID, "pg_seqset_concat_ranges: NULL argument");
    return seqset_concat(ctx, sets, first_contig, ncontigs, nsets, out);
    PG_API_END
}

extern "C" int pg_seqset_slice(pg_ctx *ctx, const pg_seqset *src, uint32_t n, const uint32_t *contig, const uint64_t *start,
                               const uint64_t *len, pg_seqset **out) {
    PG_API_BEGIN
    if (!ctx || !src || !out || (n && (!contig || !start || !len))) return fail(PG_E_INVALID, "pg_seqset_slice: NULL argument");
    if (src->ctx != ctx) return fail(PG_E_INVALID, "pg_seqset_slice: the seqset belongs to another context");
    for (uint32_t i = 0; i < n; ++i) {
        if (contig[i] >= src->n) return fail(PG_E_INVALID, "pg_seqset_slice: contig %u out of range (0..%u)", contig[i], src->n ? src->n - 1 : 0);
        if (start[i] & 31u) return fail(PG_E_INVALID, "pg_seqset_slice: piece %u starts at base %llu — starts must be multiples of 32", i, (unsigned long long)start[i]);
        if (start[i] > src->desc[contig[i]].len || len[i] > src->desc[contig[i]].len - start[i])
            return fail(PG_E_INVALID, "pg_seqset_slice: piece %u (%llu + %llu) exceeds contig %u of %llu bases", i, (unsigned long long)start[i],
                        (unsigned long long)len[i], contig[i], (unsigned long long)src->desc[contig[i]].len);
    }
    pg_seqset *s = nullptr;
    if (int r = pg_seqset_create(ctx, n, len, &s)) return r;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    for (uint32_t i = 0; i < n && e == hipSuccess; ++i) {
        const SeqDesc &from = src->desc[contig[i]];
        const uint64_t w0 = start[i] >> 5, nw = (len[i] + 31) >> 5;  // (whole words: the piece starts on a word boundary)
        if (nw) {
            e = hipMemcpyAsync(s->d_seqw + s->desc[i].seq_off, src->d_seqw + from.seq_off + w0, nw * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(s->d_nmw + s->desc[i].seq_off, src->d_nmw + from.seq_off + w0, nw * 4, hipMemcpyDeviceToDevice, st);
        }
        // (the contig's "holds a byte outside ACGT" flag is inherited: a piece without one only reads a zero plane)
        if (e == hipSuccess) e = hipMemcpyAsync(s->d_has_n + i, src->d_has_n + contig[i], 4, hipMemcpyDeviceToDevice, st);
        std::string nm = contig[i] < src->names.size() ? src->names[contig[i]] : std::string();
        s->names.push_back(nm + ":" + std::to_string((unsigned long long)start[i]));
    }
    if (e == hipSuccess) e = launch_seq_tailmask(st, s->d_desc, n, s->d_seqw, s->d_nmw);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        pg_seqset_destroy(s);
        return fail(PG_E_HIP, "pg_seqset_slice: %s", hipGetErrorString(e));
    }
    *out = s;
    return PG_OK;
    PG_API_END
}

extern "C" uint32_t pg_seqset_ncontigs(const pg_seqset *s) { return s ? s->n : 0; }

extern "C" int pg_seqset_contig(const pg_seqset *s, uint32_t idx, const char **name, uint64_t *len) {
    PG_API_BEGIN
    if (!s) return fail(PG_E_INVALID, "seqset is NULL");
    if (idx >= s->n) return fail(PG_E_INVALID, "contig %u out of range", idx);
    if (name) *name = idx < s->names.size() ? s->names[idx].c_str() : "";
    if (len) *len = s->desc[idx].len;
    return PG_OK;
    PG_API_END
}

extern "C" int pg_seqset_describe(const pg_seqset *s, uint64_t *lens, char *names, uint64_t names_cap, uint64_t *names_bytes) {
    PG_API_BEGIN
    if (!s) return fail(PG_E_INVALID, "seqset is NULL");
    uint64_t need = 0;
    for (uint32_t i = 0; i < s->n; ++i) {
        if (lens) lens[i] = s->desc[i].len;
        need += (i < s->names.size() ? s->names[i].size() : 0) + 1;
    }
    if (names_bytes) *names_bytes = need;
    if (names) {
        if (names_cap < need) return fail(PG_E_INVALID, "pg_seqset_describe: %llu bytes of names, room for %llu", (unsigned long long)need, (unsigned long long)names_cap);
        char *p = names;
        for (uint32_t i = 0; i < s->n; ++i) {
            if (i < s->names.size()) {
                memcpy(p, s->names[i].data(), s->names[i].size());
                p += s->names[i].size();
            }
            *p++ = 0;
        }
    }
    return PG_OK;
    PG_API_END
}

extern "C" int pg_seqset_unpack(const pg_seqset *s, uint32_t idx, char *out) {
    PG_API_BEGIN
    if (!s || !out) return fail(PG_E_INVALID, "pg_seqset_unpack: NULL argument");
    if (idx >= s->n) return fail(PG_E_INVALID, "contig %u out of range", idx);
    if (int r = use_device(s->ctx)) return r;
    const SeqDesc &d = s->desc[idx];
    const uint64_t nw = (d.len + 31) / 32;
    std::vector<uint64_t> w(nw);
    std::vector<uint32_t> nm(nw);
    if (nw) {
        HIP_TRY(hipMemcpyAsync(w.data(), s->d_seqw + d.seq_off, nw * 8, hipMemcpyDeviceToHost, s->ctx->stream));
        HIP_TRY(hipMemcpyAsync(nm.data(), s->d_nmw + d.seq_off, nw * 4, hipMemcpyDeviceToHost, s->ctx->stream));
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    }
    for (uint64_t i = 0; i < d.len; ++i)
        out[i] = ((nm[i >> 5] >> (i & 31)) & 1u) ? 'N' : "ACGT"[(w[i >> 5] >> (2 * (i & 31))) & 3u];
    return PG_OK;
    PG_API_END
}

extern "C" uint64_t pg_seqset_total_kmers(const pg_seqset *s, int k) {
    uint64_t t = 0;
    if (s)
        for (auto &d : s->desc)
            if (d.len >= (uint64_t)k) t += d.len - k + 1;
    return t;
}
