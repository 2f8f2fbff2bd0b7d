// pg_api_bgzf.hip — host side of the C-ABI: a result's rows to and from BGZF files, deflated / inflated on the GPU.
#include "pg_host.h"

// ---------------------------------------------------------------------------
// GPU-compressed BGZF: k_row_deflate turns every 65280 payload bytes into a finished BGZF block in
// a 64 KiB slot; the host copies the slots back in batches and appends the blocks to the file.
// ---------------------------------------------------------------------------
static constexpr uint32_t CRC_TAB_WORDS = DF_CRC_TAB_WORDS;
// [0..1024): CRC-32 slicing-by-four tables T0..T3 (T0 = the byte table); then DF_CRC_LEVELS sets of 4 x 256: set j = the
// register after DF_CHUNK_BYTES * 2^j more (zero) bytes, as a function of each of its four bytes
static const uint32_t *crc_tables_host() {
    static uint32_t tab[CRC_TAB_WORDS];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
        for (uint32_t k = 1; k < 4; ++k)
            for (uint32_t b = 0; b < 256; ++b) tab[256 * k + b] = (tab[256 * (k - 1) + b] >> 8) ^ tab[tab[256 * (k - 1) + b] & 255u];
        uint32_t *T0 = tab + 1024;
        for (uint32_t k = 0; k < 4; ++k)
            for (uint32_t b = 0; b < 256; ++b) {
                uint32_t s = b << (8 * k);
                for (uint32_t z = 0; z < DF_CHUNK_BYTES; ++z) s = tab[s & 255u] ^ (s >> 8);
                T0[256 * k + b] = s;
            }
        for (uint32_t j = 1; j < DF_CRC_LEVELS; ++j) {  // set j = set j-1 applied twice
            const uint32_t *P = tab + 1024 + 1024 * (j - 1);
            uint32_t *T = tab + 1024 + 1024 * j;
            auto apply = [&](uint32_t x) { return P[x & 255u] ^ P[256 + ((x >> 8) & 255u)] ^ P[512 + ((x >> 16) & 255u)] ^ P[768 + (x >> 24)]; };
            for (uint32_t k = 0; k < 4; ++k)
                for (uint32_t b = 0; b < 256; ++b) T[256 * k + b] = apply(apply(b << (8 * k)));
        }
    });
    return tab;
}

#ifndef PG_DF_BATCH
#define PG_DF_BATCH 1024
#endif
static constexpr uint32_t DF_BATCH = PG_DF_BATCH;  // BGZF blocks per k_row_deflate launch (64 KiB slot each)

static pg_ctx::DfSet *df_acquire(pg_ctx *ctx) {
    std::unique_lock<std::mutex> lk(ctx->df_mu);
    for (;;) {
        for (auto &d : ctx->df)
            if (!d.busy) {
                d.busy = true;
                return &d;
            }
        ctx->df_cv.wait(lk);  // more writer threads than staging sets: wait for one to be released
    }
}
static void df_release(pg_ctx *ctx, pg_ctx::DfSet *D) {
    {
        std::lock_guard<std::mutex> lk(ctx->df_mu);
        D->busy = false;
    }
    ctx->df_cv.notify_one();
}
// device + pinned buffers of a staging set (all or nothing: a partial set is given back at once)
void pg::df_free_buffers(pg_ctx::DfSet &d) {
    for (int i = 0; i < 2; ++i) {
        if (d.d_slots[i]) hipFree(d.d_slots[i]);
        if (d.d_packed[i]) hipFree(d.d_packed[i]);
        if (d.d_sizes[i]) hipFree(d.d_sizes[i]);
        if (d.d_offs[i]) hipFree(d.d_offs[i]);
        if (d.h_slots[i]) hipHostFree(d.h_slots[i]);
        if (d.h_sizes[i]) hipHostFree(d.h_sizes[i]);
        d.d_slots[i] = d.d_packed[i] = d.h_slots[i] = nullptr;
        d.d_sizes[i] = d.d_offs[i] = d.h_sizes[i] = nullptr;
    }
    if (d.d_crc) hipFree(d.d_crc);
    if (d.d_hist) hipFree(d.d_hist);
    if (d.d_code) hipFree(d.d_code);
    d.d_crc = d.d_hist = nullptr;
    d.d_code = nullptr;
    d.ready = false;
}

static int write_bgzf_gpu(pg_result *r, const uint8_t *src, const std::vector<std::pair<uint64_t, uint64_t>> &segs_in,
                          uint64_t total, uint32_t row, const char *gz_path, const char *gzi_path) {
    static const unsigned char EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0x00, 0x42, 0x43,
                                                0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0};
    pg_ctx *ctx = r->ctx;
    const uint64_t nblocks = (total + 65279) / 65280;
    std::vector<PaySeg> segs;
    uint64_t l = 0;
    for (auto &sg : segs_in) {
        segs.push_back({l, sg.first});
        l += sg.second;
    }
    segs.push_back({total, 0});
    FILE *f = fopen(gz_path, "wb");
    if (!f) return fail(PG_E_IO, "cannot open %s for writing", gz_path);
    pg_ctx::DfSet *D = df_acquire(ctx);
    DevBuf<PaySeg> d_segs;
    Event done[2], copied[2];
    Stream cs;
    hipError_t e = cs.create();
    auto ok = [&](hipError_t x) {
        if (e == hipSuccess) e = x;
        return e == hipSuccess;
    };
    if (!D->ready) {
        ok(hipMalloc(reinterpret_cast<void **>(&D->d_crc), CRC_TAB_WORDS * 4));
        ok(hipMalloc(reinterpret_cast<void **>(&D->d_hist), DF_HIST_WORDS * 4));
        ok(hipMalloc(&D->d_code, DF_CODE_BYTES));
        for (int i = 0; i < 2; ++i) {
            ok(hipMalloc(reinterpret_cast<void **>(&D->d_slots[i]), (size_t)DF_BATCH * 65536));
            ok(hipMalloc(reinterpret_cast<void **>(&D->d_packed[i]), (size_t)DF_BATCH * 65536));
            ok(hipMalloc(reinterpret_cast<void **>(&D->d_sizes[i]), (size_t)DF_BATCH * 4));
            ok(hipMalloc(reinterpret_cast<void **>(&D->d_offs[i]), (size_t)(DF_BATCH + 1) * 4));
            ok(hipHostMalloc(reinterpret_cast<void **>(&D->h_slots[i]), (size_t)DF_BATCH * 65536, 0));   // packed blocks
            ok(hipHostMalloc(reinterpret_cast<void **>(&D->h_sizes[i]), (size_t)(DF_BATCH + 1) * 4, 0));  // their offsets
        }
        if (e == hipSuccess) {
            ok(hipMemcpyAsync(D->d_crc, crc_tables_host(), CRC_TAB_WORDS * 4, hipMemcpyHostToDevice, cs.get()));
            ok(hipStreamSynchronize(cs.get()));
        }
        D->ready = e == hipSuccess;
        if (!D->ready) df_free_buffers(*D);  // never keep half a set: the next call would overwrite (leak) its pointers
    }
    ok(d_segs.alloc(segs.size()));
    for (int i = 0; i < 2; ++i) {
        ok(done[i].create(hipEventDisableTiming));
        ok(copied[i].create(hipEventDisableTiming));
    }
    if (e == hipSuccess) {
        ok(hipMemcpyAsync(d_segs.get(), segs.data(), segs.size() * sizeof(PaySeg), hipMemcpyHostToDevice, cs.get()));
        ok(hipStreamWaitEvent(cs.get(), r->ev[r->ev_epi ? 3 : 1], 0));
    }
    // ONE Huffman code for the file, from a sample of its blocks (pg_deflate.hip)
    if (e == hipSuccess && nblocks) ok(launch_deflate_code(cs.get(), src, d_segs.get(), (uint32_t)segs.size() - 1, total, row, D->d_hist, D->d_code));
    std::vector<uint64_t> coffs, uoffs;
    uint64_t cpos = 0;
    int rc = PG_OK;
    // per batch: compress into slots, pack the finished blocks back to back, bring home the offsets first
    // (they say how many packed bytes to fetch), then the bytes
    auto issue = [&](uint64_t b0, int slot) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(DF_BATCH, nblocks - b0);
        hipError_t x = hipMemsetAsync(D->d_slots[slot], 0, (size_t)nb * 65536, cs.get());
        if (x == hipSuccess)
            x = launch_row_deflate(cs.get(), src, d_segs.get(), (uint32_t)segs.size() - 1, total, b0, nb, row, D->d_crc, D->d_code, D->d_slots[slot],
                                   D->d_sizes[slot], getenv("PG_DEFLATE_FORCE_STORED") ? (uint32_t)atoi(getenv("PG_DEFLATE_FORCE_STORED")) : 0u, D->d_offs[slot], D->d_packed[slot]);
        if (x == hipSuccess)
            x = hipMemcpyAsync(D->h_sizes[slot], D->d_offs[slot], (size_t)(nb + 1) * 4, hipMemcpyDeviceToHost, cs.get());
        if (x == hipSuccess) x = hipEventRecord(done[slot].get(), cs.get());
        return x;
    };
    if (e == hipSuccess && nblocks) ok(issue(0, 0));
    int slot = 0;
    for (uint64_t b0 = 0; e == hipSuccess && rc == PG_OK && b0 < nblocks; b0 += DF_BATCH, slot ^= 1) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(DF_BATCH, nblocks - b0);
        if (!ok(hipEventSynchronize(done[slot].get()))) break;
        const uint32_t *offs = D->h_sizes[slot];
        const uint32_t bytes = offs[nb];
        if (bytes < 26u * nb || bytes > nb * 65536ull) {
            rc = fail(PG_E_IO, "GPU deflate produced %u bytes for %u blocks", bytes, nb);
            break;
        }
        if (!ok(hipMemcpyAsync(D->h_slots[slot], D->d_packed[slot], bytes, hipMemcpyDeviceToHost, cs.get()))) break;
        if (!ok(hipEventRecord(copied[slot].get(), cs.get()))) break;
        if (b0 + DF_BATCH < nblocks && !ok(issue(b0 + DF_BATCH, slot ^ 1))) break;  // the next batch runs behind the copy
        if (!ok(hipEventSynchronize(copied[slot].get()))) break;
        for (uint32_t i = 0; i < nb; ++i) {
            coffs.push_back(cpos + offs[i]);
            uoffs.push_back((b0 + i) * 65280ull);
        }
        if (fwrite(D->h_slots[slot], 1, bytes, f) != bytes) {
            rc = fail(PG_E_IO, "short write to BGZF file");
            break;
        }
        cpos += bytes;
    }
    if (e != hipSuccess) rc = fail(PG_E_HIP, "pg_result_write_bgzf (GPU deflate): %s", hipGetErrorString(e));
    if (cs.get()) hipStreamSynchronize(cs.get());
    df_release(ctx, D);
    const std::string keep = rc ? g_err : std::string();
    if (!rc && fwrite(EOF_BLOCK, 1, sizeof EOF_BLOCK, f) != sizeof EOF_BLOCK) rc = fail(PG_E_IO, "short write of BGZF EOF block");
    if (fclose(f) != 0 && !rc) rc = fail(PG_E_IO, "fclose failed on BGZF file");
    if (!rc && gzi_path) {
        FILE *g = fopen(gzi_path, "wb");
        if (!g) rc = fail(PG_E_IO, "cannot open %s", gzi_path);
        else {
            const uint64_t ng = coffs.empty() ? 0 : coffs.size() - 1;
            bool good = fwrite(&ng, 8, 1, g) == 1;
            for (size_t i = 1; good && i < coffs.size(); ++i) good = fwrite(&coffs[i], 8, 1, g) == 1 && fwrite(&uoffs[i], 8, 1, g) == 1;
            if (fclose(g) != 0) good = false;
            if (!good) rc = fail(PG_E_IO, "short write to .gzi");
        }
    }
    if (!keep.empty()) g_err = keep;
    return rc;
}

// ---------------------------------------------------------------------------
// device rows -> BGZF file: D2H through two pinned buffers on a private stream while the previous
// buffer is being deflated by the writer's threads.  Safe to call from a worker thread while the
// context's streams keep running other results.
// ---------------------------------------------------------------------------
extern "C" int pg_result_write_bgzf(pg_result *r, int step, const char *gz_path, const char *gzi_path, int level,
                                    int nthreads) {
    PG_API_BEGIN
    if (!r) return fail(PG_E_INVALID, "pg_result_write_bgzf: NULL argument");
    return pg_result_write_bgzf_range(r, step, 0, (uint32_t)r->ad.size(), gz_path, gzi_path, level, nthreads);
    PG_API_END
}

extern "C" int pg_result_write_bgzf_range(pg_result *r, int step, uint32_t first_contig, uint32_t ncontigs,
                                          const char *gz_path, const char *gzi_path, int level, int nthreads) {
    PG_API_BEGIN
    if (!r || !gz_path) return fail(PG_E_INVALID, "pg_result_write_bgzf: NULL argument");
    if ((uint64_t)first_contig + ncontigs > r->ad.size())
        return fail(PG_E_INVALID, "contigs %u..%u out of range", first_contig, first_contig + ncontigs);
    if (int e = check_step(r, step)) return e;
    if (!r->ev_ok) return fail(PG_E_INVALID, "pg_anchor_run has not been called on this result");
    if (step == 100 && (r->flags & PG_ANCHOR_ROWS_ONLY) && !r->ev_epi)
        return fail(PG_E_INVALID, "rows-only result: bitmap.100 needs pg_rows_epilogue first");
    if (int e = use_device(r->ctx)) return e;
    // the payload is the contigs' segments back to back (their device buffers are padded apart)
    const uint8_t *src = step == 1 ? r->d_out1 : r->d_out100;
    const uint32_t nbytes_row = (r->N + 7) / 8;
    std::vector<std::pair<uint64_t, uint64_t>> segs;  // (device offset, length)
    uint64_t total = 0;
    for (size_t i = first_contig; i < (size_t)first_contig + ncontigs; ++i) {
        const uint64_t len = (step == 1 ? (uint64_t)r->ad[i].nkmers : r->nrows100[i]) * nbytes_row;
        if (len) segs.emplace_back(step == 1 ? r->ad[i].out_off : r->ad[i].out100_off, len);
        total += len;
    }
    // level -2: compress on the GPU (k_row_deflate), the host only writes the blocks
    if (level == -2 && nbytes_row < 256) return write_bgzf_gpu(r, src, segs, total, nbytes_row, gz_path, gzi_path);
    if (nthreads < 1) nthreads = 1;
    pg_bgzf *w = nullptr;
    if (level >= 0) level |= nbytes_row == 1 ? PG_BGZF_RLE : (nbytes_row < 256 ? PG_BGZF_ROWS(nbytes_row) : 0);
    if (int e = pg_bgzf_open(gz_path, level, nthreads, &w)) return e;
    const size_t chunk = (size_t)512 * 65280;  // 32 MiB: 512 BGZF blocks, shared out one by one among the threads
    PinBuf<uint8_t> pin[2];
    Event done[2];
    Stream cs;
    int rc = PG_OK;
    hipError_t e = cs.create();
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = pin[i].alloc(std::min<uint64_t>(chunk, std::max<uint64_t>(total, 1)), 0);
        if (e == hipSuccess) e = done[i].create(hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipStreamWaitEvent(cs.get(), r->ev[r->ev_epi ? 3 : 1], 0);
    if (e == hipSuccess) {
        size_t seg = 0;
        uint64_t seg_pos = 0;  // cursor of the next byte to fetch
        auto issue = [&](uint64_t off, int b) {  // payload bytes [off, off+n) -> pin[b]
            const uint64_t n = std::min<uint64_t>(chunk, total - off);
            hipError_t x = hipSuccess;
            uint64_t got = 0;
            while (got < n && x == hipSuccess) {
                const uint64_t take = std::min<uint64_t>(n - got, segs[seg].second - seg_pos);
                x = hipMemcpyAsync(pin[b].get() + got, src + segs[seg].first + seg_pos, take, hipMemcpyDeviceToHost, cs.get());
                got += take;
                seg_pos += take;
                if (seg_pos == segs[seg].second) {
                    ++seg;
                    seg_pos = 0;
                }
            }
            if (x == hipSuccess) x = hipEventRecord(done[b].get(), cs.get());
            return x;
        };
        uint64_t off = 0;
        int b = 0;
        if (total) e = issue(0, 0);
        while (e == hipSuccess && off < total) {
            const uint64_t n = std::min<uint64_t>(chunk, total - off);
            e = hipEventSynchronize(done[b].get());
            if (e != hipSuccess) break;
            if (off + n < total) {
                e = issue(off + n, b ^ 1);
                if (e != hipSuccess) break;
            }
            if ((rc = pg_bgzf_write(w, pin[b].get(), n))) break;
            off += n;
            b ^= 1;
        }
    }
    if (e != hipSuccess) rc = fail(PG_E_HIP, "pg_result_write_bgzf: %s", hipGetErrorString(e));
    if (cs.get()) hipStreamSynchronize(cs.get());
    const std::string keep = rc ? g_err : std::string();
    const int rc2 = pg_bgzf_close(w, rc ? nullptr : gzi_path);
    if (rc) g_err = keep;
    return rc ? rc : rc2;
    PG_API_END
}

// ---------------------------------------------------------------------------
// BGZF inflated on the GPU (pg_inflate.hip): the host finds the blocks (BSIZE / ISIZE, or the .gzi), uploads their
// compressed bytes piece by piece and k_bgzf_inflate writes the payload into device memory through a segment map.
// ---------------------------------------------------------------------------
static constexpr uint64_t INF_PIECE_BYTES = 64ull << 20;  // compressed bytes per launch
static constexpr uint32_t INF_PIECE_BLOCKS = 1u << 18;

static const char *inf_what(uint32_t code) {
    switch (code) {
    case INF_E_HEADER: return "bad header";
    case INF_E_TYPE: return "reserved block type";
    case INF_E_STORED: return "stored block LEN / NLEN mismatch";
    case INF_E_CODES: return "over-subscribed or incomplete Huffman code";
    case INF_E_SYMBOL: return "invalid Huffman symbol";
    case INF_E_DISTANCE: return "distance reaches back past the start of the output";
    case INF_E_OVERRUN: return "output overruns ISIZE";
    case INF_E_INPUT: return "deflate data overruns BSIZE";
    case INF_E_ISIZE: return "ISIZE mismatch";
    case INF_E_CRC: return "CRC32 mismatch";
    default: return "malformed";
    }
}

// the gzip header of a BGZF block at p (avail bytes from there): header length, BSIZE + 1, ISIZE.  0 when well formed
static bool bgzf_header(const uint8_t *p, uint64_t avail, uint32_t *hlen, uint32_t *csize, uint32_t *isize) {
    if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return false;
    const uint32_t xlen = p[10] | (p[11] << 8);
    if (12ull + xlen > avail) return false;
    uint32_t bsize = 0;
    bool found = false;
    for (uint32_t i = 12; i + 4 <= 12 + xlen;) {
        const uint32_t slen = p[i + 2] | (p[i + 3] << 8);
        if (p[i] == 'B' && p[i + 1] == 'C' && slen == 2 && i + 6 <= 12 + xlen) {
            bsize = p[i + 4] | (p[i + 5] << 8);
            found = true;
        }
        i += 4 + slen;
    }
    if (!found) return false;
    *hlen = 12 + xlen;
    *csize = bsize + 1;
    if (*csize < *hlen + 8 + 2 || *csize > avail) return false;
    const uint8_t *f = p + *csize - 4;
    *isize = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
    return *isize <= 65536;
}

// blocks[] (coff relative to comp; file offset = file_base + coff) -> d_dst through segs, in launches of whole pieces
static int inflate_blocks(pg_ctx *ctx, const uint8_t *comp, uint64_t file_base, std::vector<InflBlock> &blocks,
                          const std::vector<PaySeg> &segs, uint8_t *d_dst) {
    if (blocks.empty()) return PG_OK;
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> d_comp, d_status, d_crc;
    DevBuf<InflBlock> d_blocks;
    DevBuf<PaySeg> d_segs;
    uint64_t span_max = 0;
    size_t nb_max = 0;
    for (size_t b0 = 0, b1; b0 < blocks.size(); b0 = b1) {  // piece geometry first: one allocation for every piece
        for (b1 = b0 + 1; b1 < blocks.size() && b1 - b0 < INF_PIECE_BLOCKS &&
                          blocks[b1].coff + blocks[b1].csize - blocks[b0].coff <= INF_PIECE_BYTES; ++b1) {
        }
        span_max = std::max<uint64_t>(span_max, blocks[b1 - 1].coff + blocks[b1 - 1].csize - blocks[b0].coff);
        nb_max = std::max(nb_max, b1 - b0);
    }
    hipError_t e = d_comp.alloc((span_max + 3) / 4 + 4);
    if (e == hipSuccess) e = d_blocks.alloc(nb_max);
    if (e == hipSuccess) e = d_status.alloc(nb_max);
    if (e == hipSuccess) e = d_crc.alloc(CRC_TAB_WORDS);
    if (e == hipSuccess) e = d_segs.alloc(segs.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_crc.get(), crc_tables_host(), CRC_TAB_WORDS * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_segs.get(), segs.data(), segs.size() * sizeof(PaySeg), hipMemcpyHostToDevice, st);
    std::vector<uint32_t> status;
    int rc = PG_OK;
    for (size_t b0 = 0, b1; e == hipSuccess && rc == PG_OK && b0 < blocks.size(); b0 = b1) {
        for (b1 = b0 + 1; b1 < blocks.size() && b1 - b0 < INF_PIECE_BLOCKS &&
                          blocks[b1].coff + blocks[b1].csize - blocks[b0].coff <= INF_PIECE_BYTES; ++b1) {
        }
        const uint64_t c0 = blocks[b0].coff, span = blocks[b1 - 1].coff + blocks[b1 - 1].csize - c0;
        const uint32_t nb = (uint32_t)(b1 - b0);
        std::vector<InflBlock> piece(blocks.begin() + b0, blocks.begin() + b1);
        for (auto &b : piece) b.coff -= c0;
        status.resize(nb);
        e = hipMemcpyAsync(d_comp.get(), comp + c0, span, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_blocks.get(), piece.data(), nb * sizeof(InflBlock), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_status.get(), 0, (size_t)nb * 4, st);
        if (e == hipSuccess)
            e = launch_bgzf_inflate(st, d_comp.get(), (span + 3) / 4, d_blocks.get(), nb, d_segs.get(), (uint32_t)segs.size() - 1, d_dst,
                                    d_crc.get(), d_status.get());
        if (e == hipSuccess) e = hipMemcpyAsync(status.data(), d_status.get(), (size_t)nb * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        for (uint32_t i = 0; i < nb; ++i)
            if (status[i]) {
                rc = fail(PG_E_FORMAT, "BGZF block at file offset %llu: %s", (unsigned long long)(file_base + blocks[b0 + i].coff),
                          inf_what(status[i]));
                break;
            }
    }
    if (e != hipSuccess) rc = fail(PG_E_HIP, "BGZF inflate: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int pg_bgzf_inflate(pg_ctx *ctx, const void *comp_, uint64_t comp_bytes, uint32_t nblocks, const uint64_t *coffs,
                               const uint64_t *roffs, void *d_out, uint64_t out_bytes, uint64_t *raw_bytes) {
    PG_API_BEGIN
    if (!ctx || (comp_bytes && !comp_) || (!coffs && roffs)) return fail(PG_E_INVALID, "pg_bgzf_inflate: bad arguments");
    const uint8_t *comp = static_cast<const uint8_t *>(comp_);
    std::vector<InflBlock> blocks;
    uint64_t roff = 0;
    if (!coffs) {  // walk BSIZE / ISIZE through the whole buffer
        for (uint64_t off = 0; off < comp_bytes;) {
            InflBlock b{};
            if (!bgzf_header(comp + off, comp_bytes - off, &b.hlen, &b.csize, &b.isize))
                return fail(PG_E_FORMAT, "BGZF block at file offset %llu: bad header", (unsigned long long)off);
            b.coff = off;
            b.roff = roff;
            roff += b.isize;
            off += b.csize;
            blocks.push_back(b);
        }
    } else {
        if (coffs[nblocks] > comp_bytes) return fail(PG_E_INVALID, "pg_bgzf_inflate: block offsets beyond the buffer");
        for (uint32_t i = 0; i < nblocks; ++i) {
            InflBlock b{};
            if (coffs[i + 1] < coffs[i] || !bgzf_header(comp + coffs[i], coffs[i + 1] - coffs[i], &b.hlen, &b.csize, &b.isize) ||
                b.csize != coffs[i + 1] - coffs[i])
                return fail(PG_E_FORMAT, "BGZF block at file offset %llu: bad header", (unsigned long long)coffs[i]);
            b.coff = coffs[i];
            if (roffs) {  // the caller's raw offsets: the device checks the footer's ISIZE against them
                if (roffs[i + 1] < roffs[i] || roffs[i + 1] - roffs[i] > 65536)
                    return fail(PG_E_FORMAT, "BGZF block at file offset %llu: ISIZE mismatch", (unsigned long long)coffs[i]);
                b.isize = (uint32_t)(roffs[i + 1] - roffs[i]);
                roff = roffs[i];
            }
            b.roff = roff;
            roff += b.isize;
            blocks.push_back(b);
        }
    }
    if (roff > out_bytes) return fail(PG_E_INVALID, "pg_bgzf_inflate: %llu payload bytes do not fit %llu", (unsigned long long)roff,
                                      (unsigned long long)out_bytes);
    if (roff && !d_out) return fail(PG_E_INVALID, "pg_bgzf_inflate: NULL output");
    if (int x = use_device(ctx)) return x;
    std::vector<PaySeg> segs = {{0, 0}, {roff, 0}};
    if (int x = inflate_blocks(ctx, comp, 0, blocks, segs, static_cast<uint8_t *>(d_out))) return x;
    if (raw_bytes) *raw_bytes = roff;
    return PG_OK;
    PG_API_END
}

extern "C" int pg_result_inflate_bgzf(pg_result *r, int step, const char *gz_path, const char *gzi_path, uint32_t first_contig,
                                      uint32_t ncontigs, uint64_t file_row0) {
    PG_API_BEGIN
    if (!r || !gz_path) return fail(PG_E_INVALID, "pg_result_inflate_bgzf: NULL argument");
    if ((uint64_t)first_contig + ncontigs > r->ad.size())
        return fail(PG_E_INVALID, "contigs %u..%u out of range", first_contig, first_contig + ncontigs);
    if (int e = check_step(r, step)) return e;
    if (r->flags & PG_ANCHOR_COLUMNS_ONLY) return fail(PG_E_INVALID, "the result has no row buffer");
    const uint64_t nbytes = (r->N + 7) / 8;
    // the payload range of the contigs and where each one's rows live in the result
    std::vector<PaySeg> segs;
    uint64_t row = file_row0;
    for (uint32_t c = 0; c < first_contig; ++c) row += step == 1 ? r->ad[c].nkmers : r->nrows100[c];
    for (uint32_t c = first_contig; c < first_contig + ncontigs; ++c) {
        segs.push_back({row * nbytes, step == 1 ? r->ad[c].out_off : r->ad[c].out100_off});
        row += step == 1 ? r->ad[c].nkmers : r->nrows100[c];
    }
    const uint64_t R0 = segs.empty() ? row * nbytes : segs[0].lstart, R1 = row * nbytes;
    segs.push_back({R1, 0});
    FILE *f = fopen(gz_path, "rb");
    if (!f) return fail(PG_E_IO, "cannot open %s", gz_path);
    std::unique_ptr<FILE, int (*)(FILE *)> fguard(f, fclose);
    fseeko(f, 0, SEEK_END);
    const uint64_t fsize = (uint64_t)ftello(f);
    // where to start: the last block at or before R0 (the .gzi: u64 n, then n x (compressed, raw) of blocks 1..n)
    uint64_t cpos = 0, rpos = 0;
    std::vector<std::pair<uint64_t, uint64_t>> gzi;
    if (gzi_path) {
        FILE *g = fopen(gzi_path, "rb");
        if (!g) return fail(PG_E_IO, "cannot open %s", gzi_path);
        uint64_t n = 0;
        bool good = fread(&n, 8, 1, g) == 1 && n < (1ull << 32);
        if (good) {
            gzi.resize(n);
            for (uint64_t i = 0; good && i < n; ++i) good = fread(&gzi[i].first, 8, 1, g) == 1 && fread(&gzi[i].second, 8, 1, g) == 1;
        }
        fclose(g);
        if (!good) return fail(PG_E_FORMAT, "%s: truncated .gzi", gzi_path);
        for (size_t i = 1; i < gzi.size(); ++i)
            if (gzi[i].first <= gzi[i - 1].first || gzi[i].second < gzi[i - 1].second)
                return fail(PG_E_FORMAT, "%s: offsets not increasing at entry %zu", gzi_path, i);
        auto it = std::upper_bound(gzi.begin(), gzi.end(), R0, [](uint64_t v, const std::pair<uint64_t, uint64_t> &p) { return v < p.second; });
        if (it != gzi.begin()) {
            --it;
            cpos = it->first;
            rpos = it->second;
        }
    }
    if (int x = use_device(r->ctx)) return x;
    if (int x = join_result(r)) return x;
    uint8_t *dst = step == 1 ? r->d_out1 : r->d_out100;
    PinBuf<uint8_t> h;
    if (h.alloc(INF_PIECE_BYTES, hipHostMallocDefault) != hipSuccess)
        return fail(PG_E_HIP, "pg_result_inflate_bgzf: no pinned staging buffer");
    size_t gi = 0;  // next .gzi entry to compare the walk with
    int rc = PG_OK;
    uint64_t prev_coff = UINT64_MAX;
    while (rc == PG_OK && rpos < R1) {
        if (cpos >= fsize) return fail(PG_E_FORMAT, "%s ends at payload byte %llu, before byte %llu", gz_path, (unsigned long long)rpos,
                                       (unsigned long long)R1);
        const uint64_t want = std::min<uint64_t>(INF_PIECE_BYTES, fsize - cpos);
        if (fseeko(f, (off_t)cpos, SEEK_SET) != 0 || fread(h.get(), 1, want, f) != want) return fail(PG_E_IO, "short read of %s", gz_path);
        std::vector<InflBlock> blocks;
        uint64_t off = 0;
        while (off < want && rpos < R1) {
            InflBlock b{};
            if (!bgzf_header(h.get() + off, want - off, &b.hlen, &b.csize, &b.isize)) {
                if (want - off < 65536 + 8 && cpos + want < fsize) break;  // the block continues in the next piece
                return fail(PG_E_FORMAT, "BGZF block at file offset %llu: bad header", (unsigned long long)(cpos + off));
            }
            // the walk against the .gzi: a block it lists must start at the raw offset it gives
            while (gi < gzi.size() && gzi[gi].first < cpos + off) ++gi;
            if (gi < gzi.size() && gzi[gi].first == cpos + off && gzi[gi].second != rpos)
                return fail(PG_E_FORMAT, "BGZF block at file offset %llu: ISIZE mismatch (the .gzi places the next block at %llu)",
                            (unsigned long long)(prev_coff == UINT64_MAX ? cpos + off : prev_coff), (unsigned long long)gzi[gi].second);
            b.coff = off;
            b.roff = rpos;
            prev_coff = cpos + off;
            rpos += b.isize;
            off += b.csize;
            if (rpos > R0) blocks.push_back(b);  // (blocks wholly before the range: walked, not inflated)
        }
        if (off == 0) return fail(PG_E_FORMAT, "BGZF block at file offset %llu: bad header", (unsigned long long)cpos);
        rc = inflate_blocks(r->ctx, h.get(), cpos, blocks, segs, dst);
        cpos += off;
    }
    if (rc) return rc;
    // the rows are there: readers of the result (pg_result_window_stats, ...) may go
    if (int x = next_events(r, false)) return x;
    HIP_TRY(hipEventRecord(r->ev[0], r->ctx->stream));
    HIP_TRY(hipEventRecord(r->ev[1], r->ctx->stream));
    r->ev_ok = true;
    r->rows_valid = true;
    return PG_OK;
    PG_API_END
}
