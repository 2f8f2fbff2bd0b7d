// pg_kernels.h — launch wrappers of the gfx950 kernels (see pg_kernels.hip)
#pragma once
#include "pg_device.h"

#include "pg_blocks_link.h"
#include "pg_genotype_host.h"
#include "pg_select_host.h"

namespace pg {

// Positions per wave-tile.  1024 since round 4: a wave spends a twelfth of a 512-position tile's time before its first
// batch (descriptor and sequence loads, one after the other) and a fifth in the overflow drain behind its last, both
// per TILE — tools/phase_timing.py — and with twice the positions the drain's batches are twice as dense: configs[1]
// 4.19 -> 4.01 ms, 27 x 160 Mb +6 %, the probe of 64 x 160 Mb -10 %.  2048 needs the queue cut to 128 entries to keep
// 32 waves per CU in LDS, and loses more to early drains than it saves (profiles/r4_ab_tile.txt).
#ifndef PG_PROBE_TILE
#define PG_PROBE_TILE 1024
#endif
#ifndef PG_PROBE_MAXRUN
#define PG_PROBE_MAXRUN 16
#endif
constexpr int PROBE_TILE = PG_PROBE_TILE;      // k-mer positions per wave-tile (k_probe) / per block (k_epilogue)
constexpr int PROBE_MAXRUN = PG_PROBE_MAXRUN;  // table lines staged in LDS per step of a 64-lane batch
// bit columns of the genome-sharded mode (k_probe's ROWMODE 3 in pg_anchor.hip, k_cols_* in pg_rows.hip)
constexpr int COLS_G = 8;  // genomes per block in columns mode
constexpr uint32_t TILE_SLOTS = PROBE_TILE / 64;  // u64 column words per genome and tile (a slot = 64 positions)
static_assert(PROBE_TILE % 512 == 0, "the column kernels take a tile in units of 512 positions");
#ifndef PG_PROBE_STAGED_LEVELS
#define PG_PROBE_STAGED_LEVELS 2
#endif
constexpr int PROBE_STAGED_LEVELS = PG_PROBE_STAGED_LEVELS;  // LDS-staged overflow levels; beyond: lanes chase inline
#ifndef PG_PROBE_QCAP
#define PG_PROBE_QCAP 320  // (entries of six bytes — group, position: with the 1024-position tile's sequence words 5104 bytes of LDS per wave, 32 waves per CU;
                           // the 192 ten-byte entries before them took the same 1920 bytes)
#endif
constexpr int PROBE_QCAP = PG_PROBE_QCAP;      // per-tile LDS overflow queue (a batch starts with at most QCAP - 64 entries queued: beyond, the tile drains early)

// which row bytes a sub-table writes: low nb0 bytes of mask word 0 at column col0, low nb1 bytes
// of mask word 1 at col0+4; words: 1 = rows are a whole number of 32-bit words, so a full mask word
// goes out as one aligned store; 2 = two-byte rows, one aligned 16-bit store; 3 = whole rows of 3/5/6/7 bytes in two byte-aligned stores;
// 0 = byte stores
struct RowCols {
    uint32_t col0, nb0, nb1, words;
};

// one packed contig of a seqset (offsets in 32-base words, shared by both planes)
struct SeqDesc {
    uint64_t seq_off;
    uint64_t nwords;
    uint64_t len;
};

// per-contig output geometry of one anchor run
struct AnchorDesc {
    uint64_t out_off;     // byte offset into the bitmap.1 buffer (16-byte aligned)
    uint64_t out100_off;  // byte offset into the bitmap.100 buffer
    uint64_t bin_off;     // first row of this contig in the bins buffer
    uint32_t nkmers;
    uint32_t binlen;
    uint32_t tile0;  // index of the contig's first tile in the launch
    uint32_t nbins;
};

hipError_t launch_table_init(hipStream_t st, const SubTable &t);
// bytes [off, off+len) of a FASTA text are sequence lines of record rec (len <= 4096, never
// crossing an absolute multiple of 4096)
struct TextChunk {
    uint64_t off;
    uint32_t len, rec;
};
hipError_t launch_text_pack(hipStream_t st, const uint8_t *d_text, const TextChunk *d_chunks, uint64_t nchunks,
                            const uint64_t *d_rec_chunk0, uint32_t nrec, uint32_t *d_counts, uint64_t *d_base,
                            uint64_t *d_rec_len, const SeqDesc *sd, uint64_t *seqw, uint32_t *nmw, uint32_t *has_n);
// header lines of a FASTA text on the device ('>' at offset 0 or behind a line feed), unordered: count[0] of them, the first cap in d_out
hipError_t launch_text_headers(hipStream_t st, const uint8_t *d_text, uint64_t nbytes, uint64_t *d_out, uint32_t cap, uint32_t *d_count);
hipError_t launch_seq_tailmask(hipStream_t st, const SeqDesc *sd, uint32_t n, uint64_t *seqw, uint32_t *nmw);
// packed contigs gathered into another seqset's planes: job i copies nwords words of both planes and the contig's flag
struct SeqCopy {
    const uint64_t *src_seqw;
    const uint32_t *src_nmw;
    const uint32_t *src_has_n;  // (this contig's flag)
    uint64_t src_off, dst_off, nwords;
};
hipError_t launch_seq_gather(hipStream_t st, const SeqCopy *jobs, uint32_t n, uint64_t max_words, uint64_t *seqw, uint32_t *nmw,
                             uint32_t *has_n);
hipError_t launch_pack(hipStream_t st, const void *d_ascii, uint64_t len, uint64_t *seqw, uint32_t *nmw,
                       uint64_t nwords, uint32_t *has_n);
hipError_t launch_sketch(hipStream_t st, int k, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                         uint64_t nkmers, uint32_t *regs);
// ... of all contigs of a seqset in one launch: jobs[j] = (contig, chunk number) — positions [chunk, chunk + 1) x SKETCH_JOB
constexpr uint32_t SKETCH_JOB = 1u << 16;
hipError_t launch_sketch_set(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, uint32_t *regs);
// MinHash candidates of a seqset (pg_minhash.hip): canonical 21-mers (mash's default k) hashed with MurmurHash3_x64_128;
// h1 <= limit goes to cand (slots >= cap only counted in *count).  jobs[j] = (contig, chunk): BASES [chunk, chunk + 1) x
// MINHASH_JOB — every contig with a base has jobs (*bases += its ACGT bases), the k-mers starting there are hashed
constexpr int MINHASH_K = 21;
constexpr uint32_t MINHASH_JOB = 1u << 16;
hipError_t launch_minhash(hipStream_t st, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                          const uint32_t *nmw, const uint32_t *has_n, uint64_t limit, uint32_t seed, uint64_t *cand, uint64_t cap,
                          unsigned long long *count, unsigned long long *bases);
hipError_t launch_insert_seq(hipStream_t st, const SubTable &t, int w, uint32_t bits, int k,
                             const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                             uint64_t nkmers, unsigned long long *counters, uint32_t max_probe, int count_mode = 0);
// the wave-cooperative build (pg_anchor.hip: k_insert_tile); tables of 128-byte lines only (8 slots, or the split layout)
hipError_t launch_insert_tiles(hipStream_t st, const SubTable &t, int w, uint32_t bits, int count_mode, const uint64_t *seqw,
                               const uint32_t *nmw, const uint32_t *has_n, const SeqDesc *sd, const uint32_t *tile0,
                               uint32_t ncontigs, uint32_t ntiles, unsigned long long *counters, uint32_t max_probe);
// Each .hip file is one code object, loaded by the HIP runtime when the first of its kernels is launched — for the anchor
// kernels' file ≈ 5 ms, which used to land on the first genome's insert.  pg_ctx_create calls these instead.
hipError_t preload_table_kernels();
hipError_t preload_anchor_kernels();
hipError_t preload_rows_kernels();
hipError_t preload_deflate_kernels();
// first tile of every contig (+ the total) of a launch over all contigs of a seqset, computed on the device
hipError_t launch_tile0(hipStream_t st, const SeqDesc *sd, uint32_t n, uint32_t k, uint32_t tile, uint32_t *tile0);
hipError_t launch_count_spill(hipStream_t st, const SubTable &t, unsigned long long *counters);
hipError_t launch_merge_min(hipStream_t st, const SubTable &src, const SubTable &dst, int w, uint32_t bits,
                            uint32_t min_count, unsigned long long *counters, uint32_t max_probe);
hipError_t launch_insert_keys(hipStream_t st, const SubTable &t, int w, const uint64_t *keys,
                              const uint32_t *vals, uint64_t n, unsigned long long *counters,
                              uint32_t max_probe);
// records [first_record, first_record + nrec) of a KMC suffix file (resident at `rec`) into group word w
hipError_t launch_import_kmc(hipStream_t st, const SubTable &t, int w, const uint8_t *rec, uint64_t first_record, uint64_t nrec,
                             const uint64_t *lut, uint64_t nlut, uint32_t prefixes_per_bin, uint32_t suffix_bytes,
                             uint32_t counter_bytes, uint32_t min_count, uint32_t max_count, unsigned long long *counters,
                             uint32_t max_probe, uint32_t phase = 2, uint32_t dense_above = 0);
hipError_t launch_rehash(hipStream_t st, const SubTable &src, const SubTable &dst,
                         unsigned long long *counters, uint32_t max_probe, uint32_t ngenomes);
hipError_t launch_export(hipStream_t st, const SubTable &t, int w, uint64_t *keys, uint32_t *vals,
                         uint64_t cap, unsigned long long *count);
hipError_t launch_counters(hipStream_t st, const SubTable &t, int w, int k, const uint64_t *seqw,
                           const uint32_t *nmw, const uint32_t *has_n, uint64_t nkmers, uint32_t *out);
// Fused statistics (round 6): a k_probe launch that is handed these buffers ends every tile of a contig whose bins are at least
// a tile long (AnchorDesc::binlen >= PROBE_TILE: a tile then touches at most two bins) by reading its finished rows back —
// while they are still in the L2 / Infinity Cache, not from HBM — and leaves, per tile:
//   tile_hist[tile][hw]   hw = N + 1 words = 2 (N + 1) u16 counters: (bin of the row relative to the tile's first: 0 / 1) x (popcount 0..N)
//   tile_cs[tile][csw]    csw = 16 * ceil(nbytes / 4) words: word 16 w + e = rows of the tile holding genome 32 w + e (low half) and
//                         genome 32 w + e + 16 (high half)
// and the tile's 1-in-100 rows in out100 (NULL: another step, k_lowres copies them).  k_tile_reduce sums the tiles' counters into
// the bins and the per-contig column sums: the statistics pass's re-read of every row from HBM (k_epilogue*) is gone.  Contigs
// with shorter bins are left to that pass, launched over their tile ranges only.  Replaces the popcount / histogram / 1-in-100
// part of the reference's scatter loop (cpp/anchor.cpp:156-183) and the column sums of index.py:1051.
struct FuseArgs {
    uint8_t *out100;
    uint32_t *tile_hist;
    uint32_t *tile_cs;
    uint32_t ngenomes, hw, csw;
};
constexpr uint32_t fuse_hist_words(uint32_t ngenomes) { return ngenomes + 1u; }
constexpr uint32_t fuse_cs_words(uint32_t ngenomes) { return 16u * ((((ngenomes + 7u) / 8u) + 3u) / 4u); }
// rows the fused instantiations exist for: 2..8 bytes; 9..16 bytes (the inline and split layouts) only in a -DPG_FUSE_WIDE=1
// build — held to the 64 vector and 80 scalar registers of eight waves per SIMD their tile end spills, and the probe of 65 /
// 128 genomes takes 11.0 / 20.7 ms instead of 4.4 / 11.4 (profiles/r6f_ab_fuse.txt).  One-byte rows keep their bit-sliced pass.
#ifndef PG_FUSE_WIDE
#define PG_FUSE_WIDE 0
#endif
constexpr bool fuse_rows_ok(uint32_t nbytes) { return nbytes >= 2u && nbytes <= (PG_FUSE_WIDE ? 16u : 8u); }
hipError_t launch_anchor(hipStream_t st, const TableDesc &T, const uint64_t *seqw, const uint32_t *nmw,
                         const uint32_t *has_n, const SeqDesc *sd, const AnchorDesc *ad,
                         const uint32_t *tile_contig, const uint32_t *sched, uint32_t tile_base, uint32_t ntiles, uint8_t *out1,
                         uint64_t out1_bytes, uint32_t columns_width = 0, const FuseArgs *fuse = nullptr);
// the tiles' counters (FuseArgs) of tiles [0, ntiles) into bins / colsums (atomic adds: both zeroed by the caller)
hipError_t launch_tile_reduce(hipStream_t st, const FuseArgs &fo, const AnchorDesc *ad, const uint32_t *tile_contig, uint32_t ntiles,
                              uint32_t *bins, unsigned long long *colsums, uint32_t want_colsums);
// genome-sharded exchange over the tiles [tile_base, tile_base + ntiles) of a result (a contig range)
hipError_t launch_cols_extract(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                               uint32_t tile_base, uint32_t ntiles, const uint8_t *out1, uint32_t g0, uint32_t width, void *dst);
hipError_t launch_cols_merge(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                             uint32_t tile_base, uint32_t ntiles, uint8_t *out1, const void *src, uint32_t part0,
                             uint32_t nparts, uint64_t part_words, uint32_t per, uint32_t accumulate);
// the rows of n_old genomes of one result (all of its ntiles tiles) + nparts column blocks of `per` genomes, indexed by those
// tiles -> the rows of n_new genomes of another result from contig dst_first_contig on (contigs of the same nkmers)
hipError_t launch_rows_append(hipStream_t st, uint32_t n_old, uint32_t n_new, const AnchorDesc *src_ad, const uint32_t *src_tile_contig,
                              uint32_t ntiles, const uint8_t *src_rows, const AnchorDesc *dst_ad, uint32_t dst_first_contig,
                              uint8_t *dst_rows, const void *cols, uint32_t nparts, uint64_t part_words, uint32_t per);
// destination bit j = source bit sel[j] of the rows of n_old genomes of one result (all of its ntiles tiles) -> the rows of n_new
// genomes of another result from contig dst_first_contig on (contigs of the same nkmers); segs: select_segments(sel) on the device
hipError_t launch_rows_select(hipStream_t st, uint32_t n_old, uint32_t n_new, const AnchorDesc *src_ad, const uint32_t *src_tile_contig,
                              uint32_t ntiles, const uint8_t *src_rows, const AnchorDesc *dst_ad, uint32_t dst_first_contig,
                              uint8_t *dst_rows, const SelSeg *segs, uint32_t nseg, uint32_t need);
// every step-th row of bitmap.1 -> low-resolution bitmap (steps other than 100)
hipError_t launch_lowres(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                         uint32_t ntiles, const uint8_t *out1, uint8_t *outlow, uint32_t step);
// GPU-side BGZF compression of a payload (pg_deflate.hip): the payload is the concatenation of
// segments of device memory; segs[nseg] is a sentinel with lstart = total
struct PaySeg {
    uint64_t lstart, doff;
};
// (a thread of k_row_deflate takes DF_CHUNK_BYTES of a block; crc_tabs: 1024 words of CRC-32 slicing-by-four tables, then
// DF_CRC_LEVELS sets of 4 x 256: set j = the register after DF_CHUNK_BYTES * 2^j more zero bytes, by each of its four bytes)
constexpr uint32_t DF_CHUNK_BYTES = 68, DF_CRC_LEVELS = 10, DF_CRC_TAB_WORDS = 1024 + DF_CRC_LEVELS * 1024;
constexpr uint32_t DF_CODE_BYTES = 2048, DF_HIST_WORDS = 288, DF_SAMPLE_BLOCKS = 512;
// one Huffman code per file: symbol counts of up to DF_SAMPLE_BLOCKS blocks -> code + block header in `code` (DF_CODE_BYTES)
hipError_t launch_deflate_code(hipStream_t st, const uint8_t *base, const PaySeg *segs, uint32_t nseg, uint64_t total, uint32_t row,
                               uint32_t *hist, void *code);
hipError_t launch_row_deflate(hipStream_t st, const uint8_t *base, const PaySeg *segs, uint32_t nseg, uint64_t total,
                              uint64_t first_block, uint32_t nblocks, uint32_t row, const uint32_t *crc_tabs, const void *code,
                              uint8_t *slots, uint32_t *sizes, uint32_t force_stored, uint32_t *offs, uint8_t *packed);
// GPU-side BGZF inflate (pg_inflate.hip): block i = bytes [coff, coff + csize) of the compressed buffer, its deflate data
// behind an hlen-byte gzip header, isize payload bytes that belong at payload offset roff; segs map the payload to device
// memory as above (bytes outside [segs[0].lstart, segs[nseg].lstart) are not written).  status[i] (zeroed by the caller)
// receives an INF_E_* code when block i is malformed.
struct InflBlock {
    uint64_t coff, roff;
    uint32_t hlen, csize, isize, pad;
};
enum : uint32_t {
    INF_E_HEADER = 1, INF_E_TYPE, INF_E_STORED, INF_E_CODES, INF_E_SYMBOL, INF_E_DISTANCE, INF_E_OVERRUN, INF_E_INPUT,
    INF_E_ISIZE, INF_E_CRC
};
hipError_t launch_bgzf_inflate(hipStream_t st, const uint32_t *comp, uint64_t comp_words, const InflBlock *blocks, uint32_t nblocks,
                               const PaySeg *segs, uint32_t nseg, uint8_t *dst, const uint32_t *crc_tabs, uint32_t *status);
hipError_t launch_window_stats(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint64_t nrows, uint32_t nwin,
                               uint32_t pieces, const uint64_t *starts, const uint64_t *ends, unsigned long long *hist,
                               unsigned long long *cs);
// masked per-bin column sums (pg_bins.hip): bin i = sampled rows [starts[i], ends[i]) of the rows at rows + base[i], sampled
// row j being row j * stride; keep: ceil(N / 32) words (bits past N zero).  cs ([nbins][N]) and kept ([nbins]) are zeroed
// by the caller and accumulated into.
hipError_t launch_bin_colsums(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, uint32_t nbins,
                              uint32_t pieces, const uint64_t *base, const uint64_t *starts, const uint64_t *ends,
                              const uint32_t *keep, uint32_t omit_fixed, unsigned long long *cs, unsigned long long *kept);
// pair counts (pg_pairs.hip): window i = sampled rows [starts[i], ends[i]) of the rows at rows + base[i], as the bins above;
// pairs ([nwin][N][N]) is zeroed by the caller and accumulated into: the entries on and above the diagonal — the caller
// mirrors them into the lower triangle.  1 <= N <= PAIRS_MAX_GENOMES.
constexpr uint32_t PAIRS_MAX_GENOMES = 512;
hipError_t launch_pair_counts(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, uint32_t nwin,
                              uint32_t pieces, const uint64_t *base, const uint64_t *starts, const uint64_t *ends,
                              unsigned long long *pairs);
// shared distinct k-mer counts of a table (pg_tablestats.hip): one pass over every slot of t, whatever its layout.  pairs
// ([N][N]: k-mers held by both genomes, the entries on and above the diagonal — the caller mirrors them), occ ([N + 1]: k-mers
// held by exactly n genomes), priv ([N]: k-mers of genome g alone) and nkeys (the slots counted) are zeroed by the caller and
// accumulated into.  1 <= N <= PAIRS_MAX_GENOMES, N <= 32 t.W.
hipError_t launch_table_pair_counts(hipStream_t st, const SubTable &t, uint32_t ngenomes, unsigned long long *pairs,
                                    unsigned long long *occ, unsigned long long *priv, unsigned long long *nkeys);
// pattern runs (pg_find.hip): a sampled row matches iff popcount(row & have) >= min_have and popcount(row & lack) <= max_lack
// (have / lack: ceil(N / 32) words each, bits at and past N zero).  Window i = sampled rows [starts[i], ends[i]) of the rows at
// rows + base[i], as the bins above; chunk c = {window, first sampled row}: the FIND_CHUNK sampled rows from there, cut at its
// window's end, a window's chunks consecutive and in order.  One block per chunk; no block waits for another.
//   offs == NULL  count: counts[c] = {matching rows, run starts, run ends, 0} of chunk c
//   offs != NULL  emit: offs[c] = {starts, ends} of all chunks before c; the sampled row numbers of the run starts / the
//                 exclusive run ends go to run_start / run_end from there on (entries at or past `total` are never written)
// 1 <= N <= FIND_MAX_GENOMES.
constexpr uint32_t FIND_CHUNK = 4096;  // sampled rows per chunk, a multiple of 256
constexpr uint32_t FIND_MAX_GENOMES = 4096;
hipError_t launch_find_runs(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, const uint64_t *base,
                            const uint64_t *starts, const uint64_t *ends, const uint2 *chunks, uint32_t nchunks,
                            const uint32_t *have, const uint32_t *lack, uint32_t min_have, uint32_t max_lack, uint4 *counts,
                            const ulonglong2 *offs, uint64_t total, uint32_t *run_start, uint32_t *run_end);
// pattern spectrum (pg_patterns.hip): the key of a sampled row = its bits for the `nselected` (1 to 64) genomes of `select`
// (ceil(N / 32) words, bits at and past N zero), in ascending column order; low_columns: they are columns 0..nselected-1.
// Windows (base, ends) and chunks as above, PATTERN_CHUNK sampled rows each.  keys / counts: the global table of `slots`
// (a power of two, >= 2 * cap) entries, keys all-ones (= empty), counts zero; ctr[4] zero: {slots claimed, rows whose key found
// the table full, rows whose key is the all-ones word (nselected = 64: never in the table), 0}.  ctr[0] <= cap and ctr[1] == 0
// afterwards: the table holds every other key with its rows.  Otherwise it holds nothing of use.  1 <= N <= PATTERN_MAX_GENOMES.
constexpr uint32_t PATTERN_CHUNK = 8192;  // sampled rows per chunk, a multiple of 256
constexpr uint32_t PATTERN_MAX_GENOMES = 4096;
hipError_t launch_pattern_counts(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, const uint64_t *base,
                                 const uint64_t *ends, const uint2 *chunks, uint32_t nchunks, const uint32_t *select,
                                 uint32_t nselected, bool low_columns, uint64_t cap, unsigned long long *keys,
                                 unsigned long long *counts, uint64_t slots, unsigned long long *ctr);
// absence runs (pg_gaps.hip): per column g of `select` (ceil(N / 32) words, bits at and past N zero) the maximal runs of sampled
// rows WITHOUT bit g.  Windows (base, ends) and chunks as above, GAPS_CHUNK sampled rows each; one block per chunk, no block
// waits for another.  A run with a present row on both sides inside its chunk is closed there: hist ([nwin][N][maxlen + 1],
// zeroed by the caller) gets 1 at min(rows, maxlen); when min_len <= rows and (max_len == 0 or rows <= max_len) nsel[window]
// gets 1 and, with cap != 0, one record {window, g, first sampled row, rows} goes to recs at the cursor while that is below cap
// (the cursor counts on; a chunk takes it once for the records it collected in LDS).
// absent ([nwin][N], zeroed) gets the chunk's absent rows; edges[chunk * N + g] = {head, tail}: the absent rows from the chunk's
// first row on / up to its last row, both the chunk's rows when no row is present (the caller stitches them: pg_gaps_host.h).
// Nothing is written for a column outside `select`.  1 <= N <= GAPS_MAX_GENOMES, 1 <= maxlen <= GAPS_MAX_MAXLEN.
constexpr uint32_t GAPS_CHUNK = 4096;  // sampled rows per chunk, a multiple of 256
constexpr uint32_t GAPS_MAX_GENOMES = 512, GAPS_MAX_MAXLEN = 4096;
constexpr uint32_t GAPS_LDS_BINS = 6144;  // N * (maxlen + 1) up to here: the chunk's spectrum is kept in LDS (24 KiB)
hipError_t launch_absence_runs(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, uint32_t stride, const uint64_t *base,
                               const uint64_t *ends, const uint2 *chunks, uint32_t nchunks, const uint32_t *select,
                               uint32_t maxlen, uint32_t min_len, uint32_t max_len, uint32_t *hist, unsigned long long *absent,
                               uint2 *edges, unsigned long long *nsel, unsigned long long *cursor, uint64_t cap, uint4 *recs);
// presence profile (pg_profile.hip): per column g what a window's hits, runs, longest run, first / end and covered bases are folded
// from.  Windows (base, ends) and chunks as above at stride 1, PROFILE_CHUNK rows each; one block per chunk, no block waits for
// another, no atomics.  partial[(chunk * N + g) * 2 + {0, 1}] = {hits, runs, longest, first} {end, gapsum, head, tail}, chunk-
// relative (ProfilePartial, pg_profile_host.h, where the caller stitches them); zeros for a column outside `select` (ceil(N / 32)
// words, bits at and past N zero).  allnone[chunk] = the chunk's rows with every selected column's bit / with none: the caller
// launches nothing for an empty selection.  1 <= N <= PROFILE_MAX_GENOMES, k >= 1.
constexpr uint32_t PROFILE_CHUNK = 4096;  // rows per chunk, a multiple of 256
constexpr uint32_t PROFILE_MAX_GENOMES = 512;
hipError_t launch_presence_profile(hipStream_t st, uint32_t ngenomes, const uint8_t *rows, const uint64_t *base,
                                   const uint64_t *ends, const uint2 *chunks, uint32_t nchunks, const uint32_t *select, uint32_t k,
                                   uint4 *partial, uint2 *allnone);
// synteny (pg_synteny.hip): a position table of `nslots` (a power of two) 16-byte slots {u64 key, u32 word of side 0, u32 word of
// side 1}, every byte 0xFF when empty.  A word = pos << 1 | rc: pos the global base offset of the k-mer in its side's contigs laid
// end to end (off[c] = the bases before contig c), rc = 1 iff the reverse complement is the canonical strand.  jobs[j] =
// (contig, chunk): k-mer positions [chunk, chunk + 1) x SYNTENY_JOB of a contig of at least k bases.  A lane walks at most
// max_probe slots; flags[0] (zeroed by the caller) becomes nonzero when an insert gave up.
//   insert  the field of `side` of every valid k-mer's key: its word when the side holds the key once, POS_MULTI beyond
//   mates   mates[koff[c] + p] for position p of contig c of side 0's sequences: word of side 1 ^ own rc when the key's field of
//           side 0 is this position and that of side 1 a position, NO_MATE otherwise; *nmated (zeroed) += the mated positions
constexpr uint32_t POS_SLOT_BYTES = 16, POS_EMPTY = 0xFFFFFFFFu, POS_MULTI = 0xFFFFFFFEu, NO_MATE = 0xFFFFFFFFu;
constexpr uint32_t SYNTENY_JOB = 1u << 14;
hipError_t launch_pos_insert(hipStream_t st, int k, uint32_t side, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs,
                             const uint32_t *off, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, void *slots,
                             uint64_t nslots, uint32_t max_probe, unsigned long long *flags);
hipError_t launch_pos_mates(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint32_t *off,
                            const uint32_t *koff, const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n,
                            const void *slots, uint64_t nslots, uint32_t max_probe, uint32_t *mates, unsigned long long *nmated);
// runs of mates: contigs[c] = {first entry of contig c in mates, its entries}; chunk = {contig, first position}: the MATE_CHUNK
// positions from there, cut at the contig's end, a contig's chunks consecutive and in order.  Position j continues its
// predecessor's run iff both are mated and mates[j] == mates[j - 1] + 2 (even words: strand +) or - 2 (odd words: strand -).
//   offs == NULL  count: counts[c] = {mated positions, run starts, run ends, 0} of chunk c
//   offs != NULL  emit: offs[c] = {starts, ends} of all chunks before c; the positions of the run starts (with their mate
//                 words) / the exclusive run ends go to run_start (run_mate) / run_end from there on (entries at or past
//                 `total` are never written)
constexpr uint32_t MATE_CHUNK = 4096;  // positions per chunk, a multiple of 256
hipError_t launch_mate_runs(hipStream_t st, const uint32_t *mates, const uint2 *contigs, const uint2 *chunks, uint32_t nchunks,
                            uint4 *counts, const ulonglong2 *offs, uint64_t total, uint32_t *run_start, uint32_t *run_end,
                            uint32_t *run_mate);
// runs of hits (pg_locate.hip; the definitions are there): the sequences sd / seqw / nmw / has_n streamed through a position table
// whose side 1 holds the queries.  chunk = {contig, first position}: the LOCATE_CHUNK k-mer positions from there, cut at the
// contig's end, a contig's chunks consecutive and in order; every contig named holds at least k bases and at most 2^32 - 1
// k-mer positions.  counts, offs, total and the three run arrays as launch_mate_runs takes them (counts[c] = {hits, run starts,
// run ends, 0}); positions are contig-relative.
constexpr uint32_t LOCATE_CHUNK = 4096;  // positions per chunk, a multiple of 256
hipError_t launch_hit_runs(hipStream_t st, int k, const SeqDesc *sd, const uint2 *chunks, uint32_t nchunks, const uint64_t *seqw,
                           const uint32_t *nmw, const uint32_t *has_n, const void *slots, uint64_t nslots, uint32_t max_probe,
                           uint4 *counts, const ulonglong2 *offs, uint64_t total, uint32_t *run_start, uint32_t *run_end,
                           uint32_t *run_hit);
// blocks of runs (pg_blocks.hip; the definitions are there): run_start / run_end / run_mate as launch_mate_runs emits them,
// contigs[c] = {first run of contig c of A, its runs}, chunk = {contig, first run inside it}: the RUN_CHUNK runs from there, a
// contig's chunks consecutive and in order.  boff: the nb ascending offsets of B's contigs (for the same-contig condition).
//   offs == NULL  count: counts[c] = the BlockChunkCount of chunk c (its first kept run undecided)
//   offs != NULL  emit: offs[c] from blocks_stitch (pg_blocks_host.h); out = 10 planes of `total` words: start, mate_first and
//                 the three sums in front of every block's first run, then end, mate_last and the sums behind its last run
//                 (entries at or past `total` are never written)
hipError_t launch_run_blocks(hipStream_t st, const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate,
                             const uint2 *contigs, const uint2 *chunks, uint32_t nchunks, const uint64_t *boff, uint32_t nb,
                             uint32_t min_run, uint32_t max_gap, uint32_t max_shift, BlockChunkCount *counts,
                             const BlockChunkOffs *offs, uint64_t total, uint32_t *out);
// the links of those blocks as variants of B against A (pg_variants.hip; the definitions are there): runs, contigs, chunks and boff
// as launch_run_blocks takes them (nb = ncb + 1 offsets, the first 0), offs = blocks_stitch's (the carried predecessor of every
// chunk), the two sides' descriptors and planes.  1 <= k <= 32, max_gap <= VARIANTS_MAX_GAP.
//   voffs == NULL  count: counts[c] = the VariantChunkCount of chunk c
//   voffs != NULL  emit: voffs[c] = the records of all chunks before c; out32 = 6 planes of `total` words (posA, lenA, posB, lenB,
//                  info, mismatches), out64 = 2 planes (the A allele, the B allele in A's orientation); entries at or past `total`
//                  are never written
hipError_t launch_link_variants(hipStream_t st, const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate,
                                const uint2 *contigs, const uint2 *chunks, uint32_t nchunks, const uint64_t *boff, uint32_t nb,
                                uint32_t k, uint32_t min_run, uint32_t max_gap, uint32_t max_shift, const BlockChunkOffs *offs,
                                const SeqDesc *sdA, const uint64_t *seqwA, const uint32_t *nmwA, const SeqDesc *sdB, uint32_t ncb,
                                const uint64_t *seqwB, const uint32_t *nmwB, VariantChunkCount *counts, const uint64_t *voffs,
                                uint64_t total, uint32_t *out32, uint64_t *out64);
// copy number (pg_copies.hip; the definitions are there): a count table of `nslots` (a power of two, at most COPIES_MAX_SLOTS)
// 8-byte keys, EMPTY_KEY when free, and beside it counter planes of nslots u32 each.  jobs[j] = (contig, chunk): k-mer positions
// [chunk, chunk + 1) x COPIES_JOB of a contig of at least k bases.  A lane walks at most max_probe slots.
//   insert   claims a slot for every valid k-mer's key; ctr[0] (zeroed by the caller) becomes nonzero when an insert gave up,
//            ctr[1] += the keys newly claimed
//   count    plane[slot] += 1 for every valid window whose key is in the table (which it only reads); *hits (zeroed) += them
//   profile  chunk = (contig, chunk number): the COPIES_CHUNK positions from there, cut at the contig's end.  Per plane g of
//            planes[g * nslots + slot], g < nplanes: partial[(chunk * nplanes + g) * COPIES_BINS + c] = the chunk's valid positions
//            with min(depth, COPIES_BINS - 1) == c; valid_partial[chunk] = its valid positions; depth != NULL: depth[g *
//            depth_stride + koff[contig] + p] = min(depth, COPIES_DEPTH_MAX), COPIES_DEPTH_INVALID at an invalid position
constexpr uint32_t COPIES_BINS = 64, COPIES_CHUNK = 4096, COPIES_JOB = 1u << 14;
constexpr uint32_t COPIES_DEPTH_MAX = 65534, COPIES_DEPTH_INVALID = 65535;
constexpr uint64_t COPIES_MAX_SLOTS = 1ull << 31;  // a slot number and the two marks of k_copy_profile fit 32 bits
hipError_t launch_copy_insert(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                              const uint32_t *nmw, const uint32_t *has_n, unsigned long long *keys, uint64_t nslots,
                              uint32_t max_probe, unsigned long long *ctr);
hipError_t launch_copy_count(hipStream_t st, int k, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys, uint64_t nslots,
                             uint32_t max_probe, uint32_t *plane, unsigned long long *hits);
hipError_t launch_copy_profile(hipStream_t st, int k, const SeqDesc *sd, const uint2 *chunks, uint32_t nchunks, const uint64_t *koff,
                               const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys,
                               uint64_t nslots, uint32_t max_probe, const uint32_t *planes, uint32_t nplanes, uint32_t *partial,
                               uint32_t *valid_partial, uint16_t *depth, uint64_t depth_stride);
// allele ranges against the count table (pg_genotype.hip; the definitions are there).  pieces[i] = windows [p0, p0 + n) of a contig
// of sd, 1 <= n <= ALLELE_PIECE, all below the contig's len - k + 1 (pg_genotype_host.h cuts them); at most 2^31 - 1 pieces, four
// to a block.  The count table as launch_copy_insert / launch_copy_profile take it.
//   insert   claims a slot for the key of every piece window that exists; ctr as launch_copy_insert's
//   support  own, other, sample: three planes of nslots counters; partial[i] = piece i's {windows | inf << 16 | seen << 32, depth};
//            min_count >= 1.  No atomics.
hipError_t launch_allele_insert(hipStream_t st, int k, const SeqDesc *sd, const AllelePiece *pieces, uint32_t npieces, const uint64_t *seqw,
                                const uint32_t *nmw, const uint32_t *has_n, unsigned long long *keys, uint64_t nslots,
                                uint32_t max_probe, unsigned long long *ctr);
hipError_t launch_allele_support(hipStream_t st, int k, const SeqDesc *sd, const AllelePiece *pieces, uint32_t npieces,
                                 const uint64_t *seqw, const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys,
                                 uint64_t nslots, uint32_t max_probe, const uint32_t *own, const uint32_t *other, const uint32_t *sample,
                                 uint32_t min_count, AllelePartial *partial);
// FASTQ text to the ASCII of one contig (pg_fastq.hip; the definitions are there): `text` is readable, and zero past nbytes, up to
// ntiles * FASTQ_TILE + 16 bytes, ntiles = ceil(nbytes / FASTQ_TILE).
//   scan  sums[tile] per tile (k_fastq_scan), then bases[tile] = {first output byte, first line number} and summary[3] = {line
//         feeds L, the number of the first malformed line below 4 (L / 4) or ~0, output bytes of the whole text} (k_fastq_offsets)
//   join  limit = 4 (L / 4) != 0: the output bytes of the lines below `limit` to out (never at or past out_cap; nbytes always
//         suffices), fin[2] = {len, consumed}
constexpr uint32_t FASTQ_TILE = 4096;
struct FastqTileSum {
    uint32_t nlf, out[4], nbad[4], firstbad[4], pad[3];  // out, nbad, firstbad: by the line number & 3 of the tile's first byte
};
hipError_t launch_fastq_scan(hipStream_t st, const uint8_t *text, uint64_t nbytes, uint32_t ntiles, FastqTileSum *sums, ulonglong2 *bases,
                             uint64_t *summary);
hipError_t launch_fastq_join(hipStream_t st, const uint8_t *text, uint64_t nbytes, uint32_t ntiles, const ulonglong2 *bases, uint64_t limit,
                             uint8_t *out, uint64_t out_cap, uint64_t *fin);
// the sample's column joined with finished rows (pg_place.hip; the definitions are there): windows (base, ends) and chunks as for
// the presence profile at stride 1, PLACE_CHUNK rows each, wcontig[window] = its contig in sd; row r of a contig is the k-mer at
// its bases [r, r + k), and every chunk lies within the contig's len - k + 1 positions.  The count table and `plane` as
// launch_copy_profile takes them.  One block per chunk, no block waits for another, no atomics: partial[chunk * N + g] = {col,
// both}, vh[chunk] = {valid, held}.  1 <= N <= PROFILE_MAX_GENOMES, min_count >= 1.
constexpr uint32_t PLACE_CHUNK = 4096;  // rows per chunk, a multiple of 256
hipError_t launch_sample_agree(hipStream_t st, uint32_t ngenomes, int k, const uint8_t *rows, const uint64_t *base, const uint64_t *ends,
                               const uint2 *chunks, uint32_t nchunks, const uint32_t *wcontig, const SeqDesc *sd, const uint64_t *seqw,
                               const uint32_t *nmw, const uint32_t *has_n, const unsigned long long *keys, uint64_t nslots,
                               uint32_t max_probe, const uint32_t *plane, uint32_t min_count, uint2 *partial, uint2 *vh);
// a sample screened against the pan table (pg_screen.hip; the definitions are there).  `plane`: one byte per slot of t, the byte
// of line l, slot s at l * t.slots + s, 4-byte aligned and readable up to the next multiple of 4 bytes.
//   mark    jobs[j] = (contig, piece): k-mer positions [piece, piece + 1) x SCREEN_JOB of a contig of at least t.k bases.  The byte
//           of every valid window's slot += 1, saturating at SCREEN_DEPTH_MAX; the table is only read.  ctr (zeroed by the caller):
//           ctr[0] += the valid windows, ctr[1] += those whose key t holds
//   screen  one pass over every slot of t whose key is below TOMB_KEY, M = its mask cut to N bits, d = its byte.  out (zeroed by
//           the caller, accumulated into): distinct [N], seen [N] (bit g, and d >= min_count), private [N] (only bit g),
//           private_seen [N], occ [N + 1] (by popcount), seen_occ [N + 1], depth_hist [SCREEN_BINS] (by min(d, SCREEN_BINS - 1)),
//           core_depth_hist [SCREEN_BINS] (the same of keys with all N bits), nkeys [1] — screen_out_words(N) words.
//           1 <= N <= PAIRS_MAX_GENOMES, N <= 32 t.W, 1 <= min_count <= SCREEN_DEPTH_MAX
constexpr uint32_t SCREEN_BINS = 64, SCREEN_DEPTH_MAX = 255, SCREEN_JOB = 1u << 14;
__host__ __device__ __forceinline__ size_t screen_out_words(uint32_t N) { return (size_t)4 * N + 2 * ((size_t)N + 1) + 2 * SCREEN_BINS + 1; }
hipError_t launch_table_mark(hipStream_t st, const SubTable &t, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, uint8_t *plane, unsigned long long *ctr);
hipError_t launch_table_screen(hipStream_t st, const SubTable &t, uint32_t ngenomes, const uint8_t *plane, uint32_t min_count,
                               unsigned long long *out);
// what a sample holds that the pan table does not (pg_novel.hip; the definitions are there).  The novel table: `nslots` (a power of
// two, at most COPIES_MAX_SLOTS) 8-byte keys, EMPTY_KEY when free, and nslots u32 depths beside them.  A lane walks at most
// max_probe slots.
//   count  jobs[j] = (contig, piece): k-mer positions [piece, piece + 1) x NOVEL_JOB of a contig of at least t.k bases; t is only
//          read.  A valid window whose key t lacks claims the key's slot and adds 1 to its depth.  ctr (zeroed by the caller):
//          ctr[0] += the valid windows, ctr[1] += those whose key t holds, ctr[2] += the keys newly claimed, ctr[3] += the claims
//          that gave up (none while the caller keeps keys + positions <= nslots / 2)
//   grow   every key of the old table claimed in the new one (nslots >= 2 old_slots, all EMPTY_KEY, depths zero) with its depth;
//          flag[0] (zeroed) becomes nonzero when a claim gave up
//   scan   offs == NULL  count: out (zeroed, accumulated into) = nkeys, solid (depth >= min_count), solid_windows (the sum of the
//                        solid depths), depth_hist [NOVEL_BINS] by min(depth, NOVEL_BINS - 1) — NOVEL_SCAN_WORDS words;
//                        block_solid[b] = the solid keys of slots [b, b + 1) x novel_scan_per_block(nslots), b < novel_scan_blocks(nslots)
//          offs != NULL  emit: offs[b] = the solid keys of all blocks before b; the solid keys and their depths in slot order to
//                        out_keys / out_depth (entries at or past cap are never written)
//   runs   chunk = {contig, first position}: the NOVEL_CHUNK k-mer positions from there, cut at the contig's end, a contig's
//          chunks consecutive and in order; every contig named holds at least t.k bases and at most 2^32 - 1 k-mer positions.
//          offs == NULL  count: counts[c] = {valid windows, run starts, run ends, novel windows} of chunk c
//          offs != NULL  emit: offs[c] = {starts, ends} of all chunks before c; the contig-relative positions of the run starts
//                        (with left_held) / the exclusive run ends (with right_held) from there on (entries at or past `total`
//                        are never written)
constexpr uint32_t NOVEL_BINS = 64, NOVEL_JOB = 1u << 14, NOVEL_CHUNK = 4096, NOVEL_SCAN_SLOTS = 4096, NOVEL_SCAN_WORDS = 3 + NOVEL_BINS;
#ifndef PG_NOVEL_SCAN_BLOCKS
#define PG_NOVEL_SCAN_BLOCKS 2048  // (a power of two; tools/novel_rate.py --lib measures another: profiles/novel_rate.txt)
#endif
constexpr uint32_t NOVEL_SCAN_BLOCKS = PG_NOVEL_SCAN_BLOCKS;  // blocks of a scan of a large table: every block ends in atomics on the same few words of `out`
// the consecutive slots one block of the scan takes: a multiple of NOVEL_SCAN_SLOTS, about nslots / NOVEL_SCAN_BLOCKS (at most 2^20)
__host__ __device__ __forceinline__ uint64_t novel_scan_per_block(uint64_t nslots) {
    const uint64_t per = (nslots + NOVEL_SCAN_BLOCKS - 1) / NOVEL_SCAN_BLOCKS;
    return (per + NOVEL_SCAN_SLOTS - 1) / NOVEL_SCAN_SLOTS * NOVEL_SCAN_SLOTS;
}
__host__ __device__ __forceinline__ uint32_t novel_scan_blocks(uint64_t nslots) {
    const uint64_t per = novel_scan_per_block(nslots);
    return (uint32_t)((nslots + per - 1) / per);
}
hipError_t launch_novel_count(hipStream_t st, const SubTable &t, const SeqDesc *sd, const uint2 *jobs, uint32_t njobs, const uint64_t *seqw,
                              const uint32_t *nmw, const uint32_t *has_n, unsigned long long *keys, uint32_t *depth, uint64_t nslots,
                              uint32_t max_probe, unsigned long long *ctr);
hipError_t launch_novel_grow(hipStream_t st, const unsigned long long *old_keys, const uint32_t *old_depth, uint64_t old_slots,
                             unsigned long long *keys, uint32_t *depth, uint64_t nslots, uint32_t max_probe, unsigned long long *flag);
hipError_t launch_novel_scan(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t min_count,
                             unsigned long long *out, uint32_t *block_solid, const uint64_t *offs, uint64_t cap,
                             unsigned long long *out_keys, uint32_t *out_depth);
hipError_t launch_novel_runs(hipStream_t st, const SubTable &t, const SeqDesc *sd, const uint2 *chunks, uint32_t nchunks, const uint64_t *seqw,
                             const uint32_t *nmw, const uint32_t *has_n, uint4 *counts, const ulonglong2 *offs, uint64_t total,
                             uint32_t *run_start, uint32_t *run_end, uint8_t *left_held, uint8_t *right_held);
// the solid keys of a novel table compacted into unitigs (pg_unitigs.hip; the definitions are there).  links and marks: two byte
// planes of max(nslots, 4) bytes beside the table, which is only read; 2 <= k <= 32; the blocks are those of the scan.
//   links       links[s] = the link byte of a solid slot, 0 of every other
//   links_emit  offs[b] = the solid keys of all blocks before b (the scan's count pass): the solid keys and their link bytes in slot
//               order to out_keys / out_links (entries at or past cap are never written)
//   walk        circular false: the linear round; true: the circular one, over the nodes that the linear round's emit pass left
//               without a mark.  bound: the nodes a walk may pass (the solid keys; the nodes not covered).  flag[0] (zeroed)
//               becomes nonzero when a walk reached its bound or the planes contradict the table.
//               offs == NULL  count: counts[b] = {the block's winners, their nodes}; marks takes the winning sides
//               offs != NULL  emit: offs[b] = {the unitigs, the bases} in front of the block's; offsets, kmers, depth_sum and
//                             circular of unitig u < cap_unitigs, base i < cap_bases (ASCII) — nothing at or past a cap is written;
//                             the linear round marks the nodes its winners pass
//   drop        NULL, or a third byte plane of max(nslots, 4) bytes: a slot whose byte is set is no node for any of these.  links:
//               block_nodes (NULL: not wanted) takes every block's nodes.
//   clean       one round of tip clipping and bubble popping over the link plane of the current nodes: sets the drop bytes of what
//               it drops (by 32-bit atomic OR) and counts[4 b ..] = block b's {tips, their nodes, bubbles, their nodes};
//               1 <= tip_kmers, bubble_kmers <= UNITIG_CLEAN_MAX_KMERS, 1 <= ratio_milli <= 999
constexpr uint32_t UNITIG_CLEAN_MAX_KMERS = 1024, UNITIG_CLEAN_MAX_ROUNDS = 64;
hipError_t launch_unitig_links(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                               uint32_t min_count, int k, uint8_t *links, const uint8_t *drop = nullptr, uint32_t *block_nodes = nullptr);
hipError_t launch_unitig_clean(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                               uint32_t min_count, int k, const uint8_t *links, uint8_t *drop, uint32_t tip_kmers, uint32_t bubble_kmers,
                               uint32_t ratio_milli, uint64_t *counts, uint32_t *flag);
hipError_t launch_unitig_links_emit(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, const uint8_t *links, uint64_t nslots,
                                    uint32_t min_count, const uint64_t *offs, uint64_t cap, unsigned long long *out_keys, uint8_t *out_links,
                                    const uint8_t *drop = nullptr);
hipError_t launch_unitig_walk(hipStream_t st, const unsigned long long *keys, const uint32_t *depth, uint64_t nslots, uint32_t max_probe,
                              uint32_t min_count, int k, const uint8_t *links, uint8_t *marks, bool circular, uint64_t bound, ulonglong2 *counts,
                              const ulonglong2 *offs, uint64_t cap_unitigs, uint64_t cap_bases, uint64_t *offsets, uint32_t *kmers,
                              uint64_t *depth_sum, uint8_t *circ_out, uint8_t *bases, uint32_t *flag, const uint8_t *drop = nullptr);
// exact k nearest neighbours among the rows of X (n x D float32, row-major; pg_knn.hip): tile i = four words {row0, nrows,
// lo, hi} — query rows [row0, row0 + nrows), nrows <= threads, search rows [lo, hi) — and a block of `threads` (64 or 256)
// threads takes one tile.  idx / d2 ([n][K]) get every query row's K entries sorted by (d2, row), (-1, +inf) where the
// segment has fewer than K rows.  1 <= K <= KNN_MAX_K, 1 <= D <= KNN_MAX_COLS; rows of up to KNN_REG_COLS columns are held
// in registers.
constexpr uint32_t KNN_MAX_K = 32, KNN_MAX_COLS = 4096, KNN_REG_COLS = 128;
hipError_t launch_knn_rows(hipStream_t st, const float *X, uint32_t D, uint32_t K, const uint32_t *tiles, uint32_t ntiles,
                           uint32_t threads, int32_t *idx, float *d2);
hipError_t launch_rows_epilogue(hipStream_t st, uint32_t ngenomes, const AnchorDesc *ad, const uint32_t *tile_contig,
                                uint32_t ntiles, const uint8_t *out1, uint8_t *out100, uint32_t *bins,
                                unsigned long long *colsums, uint32_t flags, const uint2 *d_ranges = nullptr,
                                uint32_t nranges = 0, uint32_t range_tiles = 0);

}  // namespace pg
