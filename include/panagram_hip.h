/*
 * panagram_hip.h — C-ABI of libpanagram_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the `panagram index` anchor hot path.  Each entry point
 * names the reference interface it replaces (paths relative to the reference
 * repo kjenike/panagram).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every function returns 0 on success, <0 (PG_E_*) on failure;
 *     pg_last_error() returns a thread-local, human-readable message.
 *   - handles are opaque; the library owns all device memory behind them.
 *   - host output buffers are allocated by the caller.
 *   - all work of a context is enqueued on ONE HIP stream (pg_ctx_set_stream), except that
 *     pg_anchor_run puts its statistics pass on a library-owned side stream, event-ordered
 *     behind the probe kernels so that it overlaps the next result's probes; every function
 *     that reads a result makes the main stream wait for that pass first.
 *     Functions documented "async" do not synchronise.
 *   - a context is not re-entrant; different contexts are independent.
 *
 * Bit/byte conventions (identical to the reference):
 *   nbytes = ceil(ngenomes/8) (cpp/anchor.cpp:34, index.py:484); genome g of a
 *   position = byte g/8, bit g%8 of its row (index.py:824-825); a row is the
 *   concatenation over 32-genome groups ("bitvec DBs", index.py:391-401) of the
 *   low n bytes of that group's u32 mask (cpp/anchor.cpp:139-164).
 */
#ifndef PANAGRAM_HIP_H
#define PANAGRAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_E_INVALID (-1)   /* bad argument */
#define PG_E_HIP (-2)       /* HIP runtime error (no GPU, OOM, launch failure) */
#define PG_E_FORMAT (-3)    /* ill-formed KMC database */
#define PG_E_CAPACITY (-4)  /* table cannot grow further */
#define PG_E_IO (-5)        /* file I/O (BGZF writer) */
#define PG_E_INTERNAL (-6)  /* the library contradicts itself (a bounded walk did not end): a bug, never the caller's fault */

typedef struct pg_ctx pg_ctx;
typedef struct pg_table pg_table;
typedef struct pg_seqset pg_seqset;
typedef struct pg_result pg_result;
typedef struct pg_bgzf pg_bgzf;

/* thread-local message of the last failing call on this thread */
const char *pg_last_error(void);
/* library version string, e.g. "panagram_hip 0.2 gfx950" */
const char *pg_version(void);
/* k-mer positions per tile: the unit of a launch, of pg_result_coschedule's pieces and of the bit-column blocks
 * (pg_tile_positions() / 8 bytes per tile and genome — one u64 per 64 positions; 128 bytes with today's tiles of 1024.
 * Size buffers with pg_result_columns_bytes / pg_result_columns_bytes_range, never with a constant) */
uint32_t pg_tile_positions(void);

/* ---- context ---------------------------------------------------------- */
/* One context per GPU / per process rank.  Fails with PG_E_HIP when no
 * gfx950-class device is visible: there is NO CPU fallback in this library. */
int pg_ctx_create(int device_id, pg_ctx **out);
/* *_destroy calls may come in any order (garbage-collected callers cannot promise one): a handle
 * with live dependants — a context with tables / seqsets, a table or seqset with results — is
 * retired at once for the caller but freed only when its last dependant is destroyed.  Destroy
 * each handle exactly once and do not use it afterwards. */
int pg_ctx_destroy(pg_ctx *ctx);
/* give back device memory the context keeps for reuse (row buffers of destroyed results: freeing and
 * re-allocating tens of GB per batch of anchors costs seconds) */
int pg_ctx_trim(pg_ctx *ctx);
/* device memory free for new tables / results (cached row buffers counted as free), and the device's total */
int pg_ctx_mem_info(pg_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
/* page-locked host memory for the buffers a caller hands to the library (ownership: "caller allocates all host
 * buffers, ideally pinned"): a FASTA image read straight into one goes up by DMA instead of through the runtime's staging
 * copy of pageable memory, and re-used it costs no page faults per file (Index.load_inputs: index.py:922-930's reading of
 * the sample files).  Free with pg_host_free, any time before the context is destroyed. */
int pg_host_alloc(pg_ctx *ctx, uint64_t nbytes, void **out);
int pg_host_free(pg_ctx *ctx, void *p);
/* adopt an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; NULL is
 * HIP's legacy default stream, which is what torch's default stream is); use_own != 0
 * restores the context's own non-blocking stream instead. */
int pg_ctx_set_stream(pg_ctx *ctx, void *hip_stream, int use_own);
int pg_ctx_synchronize(pg_ctx *ctx);
/* plain device buffers (zeroed; memset is async on the context's stream) for callers without an allocator of their
 * own: the genome-sharded pipeline's exchange buffers in a single-process run */
int pg_device_alloc(pg_ctx *ctx, uint64_t bytes, void **out);
int pg_device_memset(pg_ctx *ctx, void *ptr, int value, uint64_t bytes);
int pg_device_free(pg_ctx *ctx, void *ptr);

/* ---- pan-kmer table: replaces the merged KMC "bitvec" databases --------
 * Reference: KMCdb::KMCdb opens root/kmc/bitvec{i} with CKMCFile::OpenForRA
 * (cpp/anchor.cpp:21-35); Genome._load_kmc (index.py:847-863).
 * ONE GPU-resident open-addressed table whatever the genome count, in 128-byte lines: up to 64 genomes 8 slots
 * {u64 key, u32 mask, u32 mask}; 65..96 genomes 6 bare keys followed by their 12-byte mask blocks (inline layout);
 * more: 16 bare keys, the mask words in a second array (split layout).  Home line = hash of the k-mer's minimizer;
 * key = canonical k-mer (2k-bit integer, first base most significant), value = the group's u32
 * one-hot-OR mask(s).  k in 1..32.  One writer at a time: the calls that add keys (insert_*, load_kmc1,
 * rehash) serialise on a per-table lock; lookups (pg_anchor_run ...) must not overlap them. */
int pg_table_create(pg_ctx *ctx, int k, int ngenomes, uint64_t expected_keys, pg_table **out);
/* the same with the table's density chosen by the caller: keys_per_line (1 .. 6.4) keys per 128-byte line of 8 slots instead
 * of the library's 3 (a load of keys_per_line / 8 in the layouts of more than 64 genomes, whose lines hold 6 or 16 keys), for a
 * known expected_keys (> 0).  SPARSER (1.5): what Index.build_table asks for where HBM is plentiful — fewer keys outside their
 * home lines, k_probe 3-8 % faster for twice the table bytes (profiles/r6k2_density_sweep.txt, r6q_wide_density.txt).  DENSER:
 * the genome-sharded mode's block
 * tables (BASELINE configs[4]) — a denser table holds the union of TWO genomes' k-mers in one GPU's HBM, the
 * job takes half the passes over the anchors' positions, and a pass against 3.4-4.5 keys per line is 5-25 % slower, not 100 %
 * (profiles/r6g_config5_blocks.txt).  The table is not grown back to 3 keys per line while it fills.  The reference has one
 * density: KMC's sorted suffix arrays (call site cpp/anchor.cpp:28-31).
 * With up to 8 genomes the table takes the byte-mask lines (two halves of seven bare keys and seven mask bytes per 128-byte line,
 * pg_table_stats reports 14 slots per line; keys_per_line and the table's bytes mean what they did; mask
 * values handed in through pg_table_insert_keys / pg_table_load_kmc keep their low 8 bits, the genomes the table has).
 * PG_BYTEMASK_LAYOUT=0 in the environment, read at every creation, keeps the 8-slot lines. */
int pg_table_create_dense(pg_ctx *ctx, int k, int ngenomes, uint64_t expected_keys, double keys_per_line, pg_table **out);
/* device bytes pg_table_create_dense would allocate (host only; the planner's arithmetic) */
int pg_table_bytes_for_dense(int k, int ngenomes, uint64_t expected_keys, double keys_per_line, uint64_t *bytes);
/* device bytes pg_table_create would allocate for that many keys (host only): lets the caller decide between one
 * replicated table and the genome-sharded mode before allocating anything */
int pg_table_bytes_for(int k, int ngenomes, uint64_t expected_keys, uint64_t *bytes);
int pg_table_destroy(pg_table *tbl);
/* empty the table, keeping its allocation and geometry (async): the genome-sharded mode builds its genome blocks'
 * tables one after the other in the same memory */
int pg_table_clear(pg_table *tbl);

/* k-mer set construction from sequence, replacing `kmc -ci1 -fm` +
 * `kmc_tools transform set_counts` + `kmc_tools complex -ocsum`
 * (workflow/Snakefile:54-110, index.py:407-426): every canonical k-mer of every
 * contig of `seqs` gets bit genome_idx%32 set in group genome_idx/32.
 * Grows the table as needed.  Synchronises. */
int pg_table_insert_seqset(pg_table *tbl, int genome_idx, const pg_seqset *seqs);
/* bits only: bit genome_idx goes into the k-mers of `seqs` that the table ALREADY holds, no key is added.  Building the
 * table from the genomes a process anchors (pg_table_insert_seqset) and updating it with all the others gives every
 * look-up of the anchor step (cpp/anchor.cpp:148: the k-mers of the anchor FASTA itself) the answer the table of all
 * genomes gives, in a fraction of its memory.  Synchronises. */
int pg_table_update_seqset(pg_table *tbl, int genome_idx, const pg_seqset *seqs);
/* same with KMC's -ci<min_count> cut-off: only canonical k-mers occurring at least min_count times
 * in the seqset enter the table (the reference counts FASTQ samples with -ci2,
 * workflow/Snakefile:88-89; min_count <= 1 is pg_table_insert_seqset) */
int pg_table_insert_seqset_min(pg_table *tbl, int genome_idx, const pg_seqset *seqs, uint32_t min_count);

/* bulk insert of (canonical key, u32 counter) pairs into group db_idx; counters
 * of equal keys are OR-ed.  Host pointers.  Synchronises. */
int pg_table_insert_keys(pg_table *tbl, int db_idx, const uint64_t *keys,
                         const uint32_t *counters, uint64_t n);

/* load a real KMC database as group db_idx: the images of X.kmc_pre / X.kmc_suf (host memory; a read-only
 * memory map of the files is fine, they are only read once, chunk by chunk).  Both layouts
 * CKMCFile::OpenForRA accepts (cpp/anchor.cpp:29, index.py:859-860): KMC1 (kmc_version 0: kmc_tools output,
 * SURVEY.md Appendix A) and KMC2 (kmc_version 0x200: what `kmc` itself writes, workflow/Snakefile:101-104 —
 * one prefix LUT per signature bin).  The records are turned into table inserts on the GPU (k_import_kmc);
 * counters outside the header's [min_count,max_count] read as 0 as in KMC.  Returns PG_E_FORMAT on an
 * ill-formed database instead of silently yielding zeros like the reference.  pg_table_load_kmc1 is the same
 * function under its first name. */
int pg_table_load_kmc(pg_table *tbl, int db_idx, const void *pre, size_t pre_len,
                      const void *suf, size_t suf_len);
int pg_table_load_kmc1(pg_table *tbl, int db_idx, const void *pre, size_t pre_len,
                       const void *suf, size_t suf_len);
/* k-mer length of a KMC database from its .kmc_pre image (host only) */
int pg_kmc_kmer_length(const void *pre, size_t pre_len, uint32_t *k);

/* statistics: distinct keys, slot capacity, bucket count, bytes, summed over sub-tables */
int pg_table_stats(pg_table *tbl, uint64_t *nkeys, uint64_t *nslots, uint64_t *nbuckets,
                   uint64_t *bytes);
/* Shared distinct k-mer counts of the pan-genome, read off the table in one pass over its slots (k_table_pair_counts):
 * pairs[a*ngenomes + b] = distinct canonical k-mers held by both genome a and genome b — the full symmetric matrix, its
 * diagonal the distinct k-mers of each genome; occ[n], n = 0..ngenomes, = distinct k-mers held by exactly n genomes
 * (occ[ngenomes] is the core; occ[0] counts slots that hold a key and no bit, and is reported as found); priv[g] = k-mers
 * of genome g alone; *nkeys = the keys counted.  occ, priv and nkeys may be NULL.  The reference's `mash triangle` step
 * (workflow/Snakefile:124-149) ESTIMATES each pair's Jaccard index from a sketch at mash's k = 21; beside it this is the
 * exact index pairs[a][b] / (pairs[a][a] + pairs[b][b] - pairs[a][b]) at the table's own k, with the core / shell / private
 * breakdown the sketch cannot give.  One restriction: the result describes the k-mers THE TABLE WAS BUILT FROM — a table
 * that was fed the anchor genomes' k-mers only answers for those k-mers, not for the genomes.  1 to 512 genomes
 * (PG_E_INVALID beyond); runs on the context's stream behind the table's last writer; synchronises. */
int pg_table_pair_counts(pg_table *tbl, uint64_t *pairs, uint64_t *occ, uint64_t *priv, uint64_t *nkeys);
/* Distinct canonical k-mers of a set of inputs before a table exists (HyperLogLog, 2^16 registers,
 * standard error 0.4 %): sizes pg_table_create's expected_keys, so the table is neither re-hashed
 * while it grows nor held twice in HBM.  Replaces nothing in the reference (KMC is only given a memory cap:
 * panagram/workflow/Snakefile:101 -m{config[kmc][memory]}); pg_sketch_registers exposes the
 * 65536 register values for parity with the CPU restatement. */
typedef struct pg_sketch pg_sketch;
int pg_sketch_create(pg_ctx *ctx, int k, pg_sketch **out);
int pg_sketch_add_seqset(pg_sketch *sk, const pg_seqset *seqs);
int pg_sketch_estimate(pg_sketch *sk, uint64_t *distinct);
int pg_sketch_registers(pg_sketch *sk, uint8_t *out65536);
/* sketches merge by register-wise maximum: the estimate for 65536 register values held by the caller (host only,
 * no device needed) — the distinct k-mers of any union of inputs whose registers were kept; and a sketch emptied
 * for the next input */
int pg_sketch_estimate_registers(const uint8_t *regs65536, uint64_t *distinct);
int pg_sketch_reset(pg_sketch *sk);
int pg_sketch_destroy(pg_sketch *sk);

/* MinHash sketch of a sample (genome_dist.tsv): the s smallest distinct h1 of MurmurHash3_x64_128(seed) over the ASCII
 * bytes of its canonical k-mers (k = 21, the lexicographically smaller of a k-mer and its reverse complement, k-mers
 * with a base other than ACGT skipped) — the sketch of the reference workflow's `mash sketch -s 10000`
 * (panagram/workflow/Snakefile:124-149).  The GPU hashes every k-mer and keeps those below a threshold tau as
 * candidates, tau = 2^64 * min(1, 4 s / expected_distinct) (expected_distinct 0: the seqset's k-mer positions); fewer
 * than s distinct candidates below tau < 2^64 reruns with 4 tau, more candidates than the buffer holds with a 4x
 * buffer.  tau / capacity other than 0 replace the automatic choices (tests: both fallbacks).  Several seqsets added
 * make one sketch (their union); bases: the ACGT bases added; passes: the kernel launches since create / reset. */
typedef struct pg_minhash pg_minhash;
int pg_minhash_create(pg_ctx *ctx, int k, uint32_t s, uint32_t seed, uint64_t tau, uint64_t capacity, pg_minhash **out);
int pg_minhash_add_seqset(pg_minhash *mh, const pg_seqset *seqs, uint64_t expected_distinct);
/* the sketch, ascending, into hashes (room for s): *count values */
int pg_minhash_result(pg_minhash *mh, uint64_t *hashes, uint32_t *count, uint64_t *bases, uint32_t *passes);
int pg_minhash_reset(pg_minhash *mh);
int pg_minhash_destroy(pg_minhash *mh);
/* host only (no device): every pair i < j of n sketches — sketch i = hashes[offsets[i], offsets[i + 1]), ascending —
 * in the order (0,1) (0,2) .. (0,n-1) (1,2) ..: mash's merge (common / denom of the s smallest of the union), the
 * distance -ln(2J / (1 + J)) / k (J = common / denom; 1 when nothing is shared, at most 1) and, when bases (ACGT bases
 * per sample) is not NULL, the p-value P[Binomial(denom, r) >= common] of mash's model (pvalue may be NULL) */
int pg_minhash_distances(const uint64_t *hashes, const uint64_t *offsets, uint32_t n, uint32_t s, int k, const uint64_t *bases,
                         double *dist, double *pvalue, uint32_t *common, uint32_t *denom);

/* re-hash into the smallest table whose mean occupancy is <= keys_per_bucket keys per 128 bytes;
 * also settles the minimizer length for the keys actually present */
int pg_table_rehash(pg_table *tbl, double keys_per_bucket);
/* as of the last pg_table_rehash: fraction of keys outside their home line, slots per line */
int pg_table_spill(const pg_table *tbl, double *fraction, uint32_t *slots);
/* the same fraction measured NOW, on the table as it stands (one pass over its lines): a table built in place and never
 * re-hashed — what Index.run() anchors against — has no "last re-hash".  Diagnostic; no reference counterpart. */
int pg_table_measure_spill(pg_table *tbl, double *fraction);
/* export group db_idx as (key, counter) pairs, unsorted; *n receives the count
 * (call with keys==NULL to query).  Lets the caller write a KMC1 database the
 * reference can open. */
int pg_table_export(pg_table *tbl, int db_idx, uint64_t *keys, uint32_t *counters,
                    uint64_t cap, uint64_t *n);
int pg_table_k(const pg_table *tbl);
int pg_table_ngenomes(const pg_table *tbl);
/* tuning knob with no reference counterpart: the table places a k-mer by its minimizer
 * (smallest canonical m-mer); m is picked from k, the key count and the genome length
 * (at creation from expected_keys; again from the length of the first sequence set inserted into the
 * empty table, and at pg_table_rehash; the environment variable PG_TABLE_WMAX=3..8 caps the window k-m+1 the
 * library chooses — 4 suits genomes dominated by one young high-copy repeat family).  set_minimizer pins m for
 * an EMPTY table: 0 = hash the k-mer itself, else k >= 20 and 3 <= k-m+1 <= 8. */
int pg_table_minimizer(const pg_table *tbl);
int pg_table_set_minimizer(pg_table *tbl, int m);
/* the minimizer length the library would choose (pure host arithmetic, no device needed): k, the expected key count
 * (0: unknown), the k-mer positions of the first sequence set (0: unknown), the widest window allowed (3..8; 0: the
 * PG_TABLE_WMAX / default cap), the genome count (0: unknown; more than 64 = the split layout).  What it encodes — window cost against merged minimizer groups — is measured in
 * profiles/r4b_m_sweep.txt; no reference counterpart (KMC's own signature length is fixed at 9, kmc_file.h). */
int pg_minimizer_length(int k, uint64_t expected_keys, uint64_t first_len, int wmax, int ngenomes);
/* How the table will be PROBED decides the window too: `coscheduled` = the number of anchor genomes one launch anchors side
 * by side (pg_result_coschedule*; 0: not known, taken as several — what pg_minimizer_length assumes; 1: one genome per
 * launch, no partner: a single-anchor `panagram index` (index.py:1012, one Snakemake job per anchor), `run_anchor` with one
 * FASTA (cpp/anchor.cpp:217-223 with argc == 5), a py_kmc_api-style GetCountersForRead caller (index.py:934-935)).  Without a
 * partner every table line comes from HBM and the launch's time follows the lines per position, which a wider window
 * lowers (profiles/r5_m_sweep_pergenome.txt).  pg_table_set_coscheduled tells an EMPTY table (before
 * the first insert / load); pg_minimizer_length_for is the rule itself. */
int pg_table_set_coscheduled(pg_table *tbl, int anchors);
int pg_minimizer_length_for(int k, uint64_t expected_keys, uint64_t first_len, int wmax, int ngenomes, int coscheduled);
/* ... and the table's DENSITY (round 6): in a table created sparser than the library's 3 keys per line (pg_table_create_dense with
 * keys_per_line < 3) merged minimizer groups cost less — a group that outgrows its home line finds the next lines empty more often —
 * and the rule may take the wider window: configs[1] m = 15 at 1.25 keys per line, 16 at 3 (profiles/r6n_m_sweep_roomy.txt,
 * r6p_lines_roomy_m.txt).  A table applies the rule with its own density; this is the rule itself (host arithmetic). */
int pg_minimizer_length_dense(int k, uint64_t expected_keys, uint64_t first_len, int wmax, int ngenomes, int coscheduled,
                              double keys_per_line);

/* ---- sequences: 2-bit packed contigs resident in HBM -------------------
 * Reference: the FASTA record strings handed to write_bits / _write_bitmap
 * (cpp/anchor.cpp:77-100, index.py:1044-1046).  A seqset holds the contigs of
 * one FASTA, each packed 2 bits/base (A=0 C=1 G=2 T=3, case-insensitive) plus a
 * 1 bit/base "not ACGT" plane; packing runs on the GPU. */
int pg_seqset_create(pg_ctx *ctx, uint32_t ncontigs, const uint64_t *lens, pg_seqset **out);
int pg_seqset_destroy(pg_seqset *s);
/* upload + pack contig `idx` from host ASCII (async w.r.t. the host only after
 * the internal staging copy; synchronises the stream before returning) */
int pg_seqset_load_host(pg_seqset *s, uint32_t idx, const char *ascii, uint64_t len);
/* pack contig `idx` from ASCII already in device memory (16-byte aligned); async */
int pg_seqset_load_dev(pg_seqset *s, uint32_t idx, const void *d_ascii, uint64_t len);
uint64_t pg_seqset_total_kmers(const pg_seqset *s, int k);
/* FASTA text (a whole file image in host memory) -> seqset: replaces the line-based parse of
 * KMCdb::anchor_fasta (cpp/anchor.cpp:77-100) and Genome.iter_fasta (index.py:922-930).  A line
 * starting with '>' opens a record whose id is the header up to the first white space; the other
 * lines are joined with all white space removed (the Python path's Bio.SeqIO behaviour; the C++
 * path differs only in keeping '\r').  The host only locates the header lines; the GPU strips the
 * line breaks and packs.  Text before the first header is ignored.  Synchronises. */
int pg_seqset_from_fasta(pg_ctx *ctx, const void *text, uint64_t nbytes, pg_seqset **out);
/* FASTQ text (host memory, starting at the first byte of a record) -> a seqset of ONE contig, on the GPU: the sequence lines of all
 * complete records joined by a single 'N', so that no k-mer window spans two reads and every kernel that streams a seqset runs on
 * reads without a descriptor per read.  What read_fastq_joined of panagram_amd/index.py does with a Python split of the whole file.
 * Records are four lines each, as kmc -fq assumes; MULTI-LINE FASTQ (a sequence wrapped over several lines) IS NOT SUPPORTED.  Only
 * the line count decides what a line is: quality lines may begin with '@' or '+'.
 *   *nreads    the complete records: (line feeds in the text) / 4
 *   *consumed  the offset just past the line feed that ends the last complete record (0 without one); the bytes from there on — a
 *              torn record — contribute nothing and are not checked: hand them in again in front of the next batch
 *   *out       one contig, its name "": per complete record the bytes of line 1 without the line feed and without a '\r' right
 *              before it, an 'N' between two records (also around an empty sequence line); packed as every seqset is (lower case
 *              folded, every byte outside ACGT an N).  Without a complete record (consumed == 0, zero bytes of text included) the
 *              contig has length 0.
 * PG_E_INVALID, and no seqset: a complete record whose line 0 does not begin with '@' or whose line 2 does not begin with '+' (the
 * message names the record number of one of them); 2^43 bytes of text or more.  k_fastq_scan over tiles of 4096 bytes (line feeds,
 * and output bytes and malformed lines for each of the four line phases a tile may start in), k_fastq_offsets (the tiles' scan),
 * k_fastq_join (the ASCII, in device memory), k_pack; no tile waits for another, no global atomics.  Synchronises. */
int pg_seqset_from_fastq(pg_ctx *ctx, const void *text, uint64_t nbytes, pg_seqset **out, uint64_t *nreads, uint64_t *consumed);
/* one seqset holding the contigs of all `sets`, in order (packed planes copied device to device):
 * lets ONE result anchor every anchor genome of a pangenome, see pg_result_coschedule */
int pg_seqset_concat(pg_ctx *ctx, const pg_seqset *const *sets, uint32_t nsets, pg_seqset **out);
/* the same from contig ranges: contigs first_contig[i] .. first_contig[i]+ncontigs[i]-1 of sets[i], in order (a set may
 * appear several times): the genome-sharded pipeline lays the anchors' contigs out chunk group by chunk group, so
 * that one launch covers the homologous pieces of every anchor */
int pg_seqset_concat_ranges(pg_ctx *ctx, const pg_seqset *const *sets, const uint32_t *first_contig,
                            const uint32_t *ncontigs, uint32_t nsets, pg_seqset **out);
/* a seqset of n PIECES of src's contigs: piece i = bases [start[i], start[i] + len[i]) of contig contig[i] (packed planes
 * copied device to device; start[i] must be a multiple of 32).  The contig-sharded multi-GPU mode cuts long chromosomes
 * into pieces with a k-1 base overlap, so that a piece's k-mer positions are rows [start, start + len - k + 1) of the
 * whole contig's bitmap (cpp/anchor.cpp:127 cuts its chunks the same way); record ids become "<id>:<start>" */
int pg_seqset_slice(pg_ctx *ctx, const pg_seqset *src, uint32_t n, const uint32_t *contig, const uint64_t *start,
                    const uint64_t *len, pg_seqset **out);
uint32_t pg_seqset_ncontigs(const pg_seqset *s);
/* record id ("" unless parsed from FASTA; owned by the seqset) and length in bases of contig idx */
int pg_seqset_contig(const pg_seqset *s, uint32_t idx, const char **name, uint64_t *len);
/* all contigs at once: lens[ncontigs] (may be NULL) and the names, each followed by a NUL, into names[names_cap] (may be
 * NULL); *names_bytes = the bytes the names take.  (A call per contig costs the interpreter 1.6 us: a quarter of a
 * second for an assembly of 20 000 contigs times eight genomes.) */
int pg_seqset_describe(const pg_seqset *s, uint64_t *lens, char *names, uint64_t names_cap, uint64_t *names_bytes);
/* diagnostic: contig idx back as len ASCII bytes — ACGT upper case, 'N' for every byte the
 * packing treats as "not ACGT" (what GetCountersForRead's window test sees); synchronises */
int pg_seqset_unpack(const pg_seqset *s, uint32_t idx, char *out);

/* ---- anchoring ---------------------------------------------------------
 * Reference: KMCdb::write_bits (cpp/anchor.cpp:112-195) per contig =
 * Genome._write_bitmap + bin_bitsum + paircount sums (index.py:949-969,
 * 1048-1051, 1169-1183).  For every k-mer position of every contig: the
 * nbytes-byte presence row (bitmap.1), every row whose contig-relative index is
 * a multiple of 100 (bitmap.100), the per-bin popcount histogram (N+1 counters
 * per bin; bin length 200000 or nkmers/100) and per-genome column sums. */
#define PG_ANCHOR_COLSUMS 1u   /* also accumulate per-genome column sums */
#define PG_ANCHOR_COLUMNS_ONLY 4u /* (with ROWS_ONLY) no row buffer: the result only emits bit columns (pg_anchor_run_columns_range) */
#define PG_ANCHOR_ROWS_ONLY 2u /* genome-sharded mode: pg_anchor_run writes only the bitmap.1 rows (this
                                * GPU's genomes' bits); after the rows of all GPUs have been combined in
                                * place (RCCL) pg_rows_epilogue derives the rest */
int pg_result_create(pg_table *tbl, const pg_seqset *seqs, uint32_t flags, pg_result **out);
/* the same with the Python path's parameters (index.py:101-106, 1169-1172; cpp/anchor.cpp:114-118,169-176
 * hard-codes 100 / 200000 / 100): the low-resolution bitmap keeps every lowres_step-th row (bitmap.<lowres_step>;
 * "bitmap100" / step 100 in the calls below then mean that bitmap), bins are max_bin_len positions long unless the
 * contig would get fewer than min_bin_count of them (then nkmers / min_bin_count) */
int pg_result_create_ex(pg_table *tbl, const pg_seqset *seqs, uint32_t flags, uint32_t lowres_step,
                        uint64_t max_bin_len, uint32_t min_bin_count, pg_result **out);
/* a result WITHOUT a table: an ngenomes-wide row buffer over the contigs of `seqs` (zeroed) that is filled
 * through pg_result_merge_columns_range and finished with pg_rows_epilogue — the writer's side of the
 * genome-sharded mode, where no single GPU holds a table of all genomes */
int pg_result_create_rows(pg_ctx *ctx, int k, int ngenomes, const pg_seqset *seqs, uint32_t flags, uint32_t lowres_step,
                          uint64_t max_bin_len, uint32_t min_bin_count, pg_result **out);
int pg_result_destroy(pg_result *r);
/* run the anchor kernels for all contigs of the result's seqset; async */
int pg_anchor_run(pg_result *r);
/* PG_ANCHOR_ROWS_ONLY results: probe contigs first_contig .. first_contig+ncontigs-1 only (bitmap.1 rows, no
 * statistics); async.  The unit of the genome-sharded pipeline: probe a chunk, extract its columns, exchange them
 * while the next chunk is probed. */
int pg_anchor_run_range(pg_result *r, uint32_t first_contig, uint32_t ncontigs);
/* the same, emitting the contig range's compact bit columns (`width` genomes wide, the layout of
 * pg_result_extract_columns_range) STRAIGHT from the probe into d_dst — no rows are written or read back.  For the
 * narrow block tables of the genome-sharded mode: pg_result_columns_direct() says whether the result's table
 * qualifies (up to 8 genomes, width in ngenomes..8); config 5 — one genome per GPU — does.  A result created with
 * PG_ANCHOR_COLUMNS_ONLY allocates no row buffer at all and only takes this call.  async */
int pg_result_columns_direct(const pg_result *r, uint32_t width);
int pg_anchor_run_columns_range(pg_result *r, uint32_t first_contig, uint32_t ncontigs, uint32_t width, void *d_dst);
/* HIP-event durations of the last pg_anchor_run on this result, measured on the context's
 * stream: the probe kernels (k_probe, one per sub-table) and the statistics kernel
 * (k_epilogue; 0 in rows-only mode).  Synchronises on the run's last event. */
int pg_result_timing(pg_result *r, float *probe_ms, float *epilogue_ms);
/* mean durations over EVERY run since pg_result_timing_reset (each run records into events of its own, nothing
 * is waited for between runs): what a benchmark quotes as its average launch.  nruns = probe launches counted. */
int pg_result_timing_reset(pg_result *r);
int pg_result_timing_mean(pg_result *r, double *probe_ms, double *epilogue_ms, uint32_t *nruns);
/* Fused statistics (round 6, an opt-in experiment: PG_FUSE_STATS=1 in the environment): a pg_anchor_run over rows of 2..8
 * bytes ends every tile INSIDE k_probe with the tile's popcount histogram, column sums and 1-in-100 rows — what
 * cpp/anchor.cpp:156-183 does in its scatter loop — read back from the rows while the cache still holds them; a small kernel
 * adds the tiles' counters up (k_tile_reduce) and the statistics pass (k_epilogue*) only visits contigs whose bins are
 * shorter than a tile.  The outputs are the same bytes either way (tests/test_gpu_parity.py); the default stays the pass over
 * every row, which is faster.  *n = whole runs of this result that took the fused path so far (0: none did —
 * not asked for, one-byte rows, rows wider than 8 bytes, several sub-tables, no contig with long enough bins, no memory for the
 * tiles' counters: 2-6 % of the rows).  No reference counterpart: a diagnostic for tests and bench.py. */
int pg_result_fused_runs(const pg_result *r, uint32_t *n);
/* Genome-sharded exchange (union of tables > one GPU's HBM): rank i owns genomes
 * [i*per, (i+1)*per) and its PG_ANCHOR_ROWS_ONLY rows hold only their bits.  extract writes the
 * compact block of bit columns of genomes [g0, g0+width) — pg_result_columns_bytes(width) bytes,
 * one u64 per genome per 64 positions — into device memory; the blocks of all ranks, all-gathered
 * over RCCL/xGMI into one buffer (nparts blocks of equal size, block i = genomes from i*per), are
 * merged back into full rows by merge.  Both are asynchronous on the context's stream. */
uint64_t pg_result_columns_bytes(const pg_result *r, uint32_t width);
int pg_result_extract_columns(pg_result *r, uint32_t g0, uint32_t width, void *d_dst);
int pg_result_merge_columns(pg_result *r, const void *d_src, uint32_t nparts, uint32_t per);
/* the same over a contig range (the pipeline's chunk): the block then holds only that range's tiles.  merge:
 * the nparts blocks are genome blocks part0 .. part0+nparts-1 of `per` genomes each; accumulate != 0 ORs their bits
 * into the rows (blocks arriving pass by pass — more genome blocks than GPUs), 0 writes the rows whole.
 * part_stride_bytes: distance between consecutive blocks in d_src (0: the range's own block size) — larger when the
 * range is a slice of a bigger exchanged chunk (d_src then points at the slice inside the first block). */
uint64_t pg_result_columns_bytes_range(const pg_result *r, uint32_t width, uint32_t first_contig, uint32_t ncontigs);
int pg_result_extract_columns_range(pg_result *r, uint32_t g0, uint32_t width, uint32_t first_contig, uint32_t ncontigs,
                                    void *d_dst);
int pg_result_merge_columns_range(pg_result *r, const void *d_src, uint32_t part0, uint32_t nparts, uint32_t per,
                                  uint32_t first_contig, uint32_t ncontigs, int accumulate, uint64_t part_stride_bytes);
/* Appending genomes to finished rows (no reference counterpart: to add a genome the reference re-runs its whole
 * workflow).  src holds the rows of N_old genomes — e.g. read back from bitmap.1.gz (pg_result_inflate_bgzf) — and
 * d_cols nparts column blocks of `per` genomes each in the layout of pg_result_extract_columns_range /
 * pg_anchor_run_columns_range over src's contigs (part_stride_bytes apart; 0: the block's own size).  dst, a result of
 * N_new genomes with N_old <= N_new <= N_old + nparts*per, gets its rows of contigs dst_first_contig .. dst_first_contig
 * + n - 1 (n = src's contigs; they must have the same k-mer counts as dst's, PG_E_INVALID otherwise) written whole in one
 * pass: bits below N_old copied, genome j of block i as bit N_old + i*per + j, bits at and past N_new zero.  Bits at and
 * past N_old in the source's last byte are ignored.  Finish with pg_rows_epilogue.  Asynchronous on the context's stream. */
int pg_result_append_columns_range(pg_result *dst, uint32_t dst_first_contig, const pg_result *src, const void *d_cols,
                                   uint32_t nparts, uint32_t per, uint64_t part_stride_bytes);
/* Selecting genomes out of finished rows (no reference counterpart: to drop or reorder samples the reference re-runs its
 * whole workflow).  src holds the rows of N_old genomes — e.g. read back from bitmap.1.gz (pg_result_inflate_bgzf) — and
 * sel, a host array, nsel distinct column numbers below N_old in any order.  dst, a result of N_new = nsel genomes, gets its
 * rows of contigs dst_first_contig .. dst_first_contig + n - 1 (n = src's contigs; they must have the same k-mer counts as
 * dst's, PG_E_INVALID otherwise) written whole in one pass: bit j = src's bit sel[j], bits at and past N_new zero.  Bits at
 * and past N_old in the source's last byte are ignored.  PG_E_INVALID, with nothing launched, also for nsel == 0 or
 * != N_new, an entry >= N_old or given twice, src == dst, a source that holds no rows.  Finish with pg_rows_epilogue.
 * Asynchronous on the context's stream (sel is read before the call returns). */
int pg_result_select_columns_range(pg_result *dst, uint32_t dst_first_contig, const pg_result *src, const uint32_t *sel,
                                   uint32_t nsel);
/* bitmap.100 rows, bin histograms and column sums from the (combined) bitmap.1 rows in the
 * result's device buffer; async.  Same outputs as the fused pg_anchor_run path. */
int pg_rows_epilogue(pg_result *r);
/* geometry of contig idx: k-mer count, bitmap.100 row count, bin count, bin length */
int pg_result_contig_info(const pg_result *r, uint32_t idx, uint64_t *nkmers, uint64_t *nrows100,
                          uint32_t *nbins, uint32_t *binlen);
/* copy contig idx's outputs to host (any pointer may be NULL); synchronises.
 *   bitmap1:   nkmers  * nbytes bytes        bitmap100: nrows100 * nbytes bytes
 *   bins:      nbins * (ngenomes+1) u32      (row b covers [b*binlen, ...)) */
/* statistics of nwin row windows [starts[i], ends[i]) (clipped to the contig) of contig idx's
 * bitmap.<step> rows in HBM: hist[i*(ngenomes+1) + c] = rows of the window with popcount c,
 * colsums[i*ngenomes + g] = rows with genome g's bit (colsums may be NULL).  One kernel for the
 * reference's per-gene occupancy tabulation (index.py:1055-1064), bin_bitsum with any bin length
 * (index.py:1169-1183) and bitmap_to_bins / paircount bins (index.py:438-449).  Synchronises. */
int pg_result_window_stats(pg_result *r, uint32_t idx, int step, uint32_t nwin, const uint64_t *starts,
                           const uint64_t *ends, uint64_t *hist, uint64_t *colsums);
/* masked per-bin column sums of the introgression caller's binning step (call_introgressions.py: bitmap_to_bins):
 * bin i = SAMPLED rows [starts[i], ends[i]) of contig contig[i]'s bitmap.<step> rows in HBM, sampled row j being row
 * j * stride.  Per row: if none of the keep_words bits is set (ceil(ngenomes / 32) words, bits past ngenomes ignored; NULL:
 * no mask), they are ORed in (--rmu); then with omit_fixed a row whose ngenomes bits are all set is dropped (--rmf).
 * cs_out[i*ngenomes + g] = rows left holding genome g's bit, kept_out[i] = rows left.  Every sampled row must lie inside
 * its contig.  One launch for all bins (k_bin_colsums); synchronises. */
int pg_result_bin_colsums(pg_result *r, int step, uint32_t stride, uint32_t nbins, const uint32_t *contig,
                          const uint64_t *starts, const uint64_t *ends, const uint32_t *keep_words, int omit_fixed,
                          uint64_t *cs_out, uint64_t *kept_out);
/* pair counts of the genomes over windows of rows, the one matrix behind the viewer's tree of the genomes over a region
 * (panagram/view.py:751-764: create_tree runs linkage(bitmap.T, "ward", "euclidean") on a sample of the region's rows):
 * window i = SAMPLED rows [starts[i], ends[i]) of contig contig[i]'s bitmap.<step> rows in HBM, sampled row j being row
 * j * stride.  pairs_out[(i*ngenomes + a)*ngenomes + b] = rows of window i holding both genome a's and genome b's bit — the
 * full symmetric matrix; its diagonal are the column sums, and pairs[a][a] + pairs[b][b] - 2 pairs[a][b] is the Hamming
 * distance of the two genomes' columns, whose square root is the Euclidean distance linkage computes.  Bits past ngenomes
 * in a row's last byte are ignored.  Every sampled row must lie inside its contig; at most 512 genomes (PG_E_INVALID
 * beyond).  One launch for all windows (k_pair_counts); synchronises. */
int pg_result_pair_counts(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                          const uint64_t *starts, const uint64_t *ends, uint64_t *pairs_out);
/* presence/absence pattern runs: where are the rows that THESE genomes hold and THOSE genomes lack (scripts/query_index.py's
 * "custom" branch: np.flatnonzero((kmers[:,0]==1) & (kmers[:,1]==0) & ...) on a chromosome unpacked on the host)?
 * The rule: have_words / lack_words are two sets of genomes as ceil(ngenomes / 32) words each (bit g of a set = bit g % 32 of
 * word g / 32; NULL: the empty set; bits at and past ngenomes are ignored, in the masks and in a row's last byte).  A row
 * matches iff popcount(row & have) >= min_have and popcount(row & lack) <= max_lack: min_have = |have|, max_lack = 0 is the
 * reference's expression, other thresholds are quorum rules; min_have > |have| matches nothing, min_have = 0 with an empty lack
 * set every row.
 * Runs: window i = SAMPLED rows [starts[i], ends[i]) of contig contig[i]'s bitmap.<step> rows in HBM, sampled row j being row
 * j * stride.  A run is a maximal range [a, b) of consecutive sampled rows of a window that all match; the window's edges cut
 * runs, and no row outside the window is read.  nruns_out[i] / matched_out[i] = the runs and the matching sampled rows of
 * window i, *total_out = the sum of nruns_out.
 * Capacity: the counts are always computed.  If *total_out > cap, or cap == 0, the call returns PG_OK with the counts filled
 * and writes nothing to run_start / run_end (which may then be NULL when cap == 0): call again with arrays of *total_out
 * entries.  Otherwise their first *total_out entries are the runs' first sampled rows and exclusive ends, as sampled row
 * numbers of their contig, sorted by (window, start) — window i's runs behind those of the windows before it — and the same on
 * every call.  Every sampled row must lie inside its contig; 1 to 4096 genomes (PG_E_INVALID otherwise, before anything is
 * launched).  Two launches of k_find_runs (count, then emit; one when nothing is emitted) over chunks of 4096 sampled rows, no
 * atomics; synchronises. */
int pg_result_find_runs(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                        const uint64_t *starts, const uint64_t *ends,
                        const uint32_t *have_words, const uint32_t *lack_words, uint32_t min_have, uint32_t max_lack,
                        uint64_t cap, uint32_t *run_start, uint32_t *run_end,
                        uint64_t *nruns_out, uint64_t *matched_out, uint64_t *total_out);
/* presence/absence pattern spectrum: WHICH patterns occur in these rows, and how many rows does each hold (query_bitmap followed
 * by DataFrame.value_counts(), the table behind an UpSet plot or a core / shell / private breakdown — the question to settle
 * before pg_result_find_runs is asked where one pattern's rows are)?
 * The selection: select_words is a set of 1 to 64 genomes as ceil(ngenomes / 32) words (bit g of the set = bit g % 32 of word
 * g / 32; bits at and past ngenomes are ignored, in the words and in a row's last byte); NULL: all ngenomes genomes.  A row's key
 * is a 64-bit word: bit i of the key is the row's bit for the i-th selected genome, in ascending column order.
 * Windows as in pg_result_find_runs: window i = SAMPLED rows [starts[i], ends[i]) of contig contig[i]'s bitmap.<step> rows in HBM,
 * sampled row j being row j * stride; no row outside a window is read.  The result is ONE spectrum over all windows of the call:
 * for every distinct key the number of sampled rows, over all windows, that have it (a row that two windows cover counts twice).
 * *rows_out = the sampled rows of all windows, always written.
 * Capacity: the rows are reduced into a hash table of max(1024, the next power of two >= 2 * cap) slots in HBM.  If no more than
 * cap distinct keys occur, *exceeded_out = 0, *ndistinct_out = their number, and the first *ndistinct_out entries of keys_out /
 * counts_out are the spectrum sorted by key ascending — the same on every call; counts_out sums to *rows_out.  Otherwise
 * *exceeded_out = 1, nothing is written to the arrays (which may be NULL when cap == 0), *ndistinct_out is unspecified and the
 * call still returns PG_OK: call again with a larger cap.  Which of the two happens depends on the rows alone, never on the run.
 * No window, or only empty ones: zero patterns, not exceeded.
 * PG_E_INVALID before anything is launched: no genome or more than 64 selected (NULL on a result of more than 64 genomes
 * included), a sampled row outside its contig, more than 4096 genomes, cap > 2^30.  One launch of k_pattern_counts over chunks
 * of 8192 sampled rows (equal neighbouring rows are counted as one run; LDS and global atomics on integers); synchronises. */
int pg_result_pattern_counts(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                             const uint64_t *starts, const uint64_t *ends, const uint32_t *select_words,
                             uint64_t cap, uint64_t *keys_out, uint64_t *counts_out,
                             uint64_t *ndistinct_out, uint64_t *rows_out, int *exceeded_out);
/* absence runs: where, and how, does each genome differ from the anchor (Index.query_bitmap's frame with a per-column
 * np.diff of the padded absence vector, every column of it, none of it read back)?  Row r of bitmap.1 is the k-mer at anchor
 * bases [r, r + k): one substituted base in genome g clears k consecutive rows of g's column, an insertion k - 1, a deletion of
 * d bases k - 1 + d, so the LENGTHS of the runs of absent rows of a column are a variant signal.
 * Windows as in pg_result_find_runs: window i = SAMPLED rows [starts[i], ends[i]) of contig contig[i]'s bitmap.<step> rows in HBM,
 * sampled row j being row j * stride; no row outside a window is read.  select_words: the genomes to follow, as ceil(ngenomes /
 * 32) words (bit g = bit g % 32 of word g / 32; bits at and past ngenomes are ignored, in the words and in a row's last byte);
 * NULL: all of them.  Everything below is zero for a genome outside the selection.
 * A run of genome g is a maximal range of consecutive sampled rows of a window without g's bit.  It is CLOSED when a present
 * row of the window bounds it on both sides; the (at most two) runs that touch the window's edges are open.
 *   hist_out[(i*ngenomes + g)*(maxlen+1) + L]  closed runs of L rows; bin maxlen holds L >= maxlen, bin 0 stays 0
 *   absent_out[i*ngenomes + g]                 absent sampled rows
 *   edge_out[(i*ngenomes + g)*2 + {0, 1}]      absent rows from the window's first row on / up to its last row: the open
 *                                              runs; both the window's rows when no row of it is present
 *   nruns_out[i]                               closed runs selected for emission: min_len <= L, and L <= max_len unless
 *                                              max_len is 0; *total_out = their sum
 * Capacity, as pg_result_find_runs: the counts above are always computed.  If *total_out > cap, or cap == 0, the call returns
 * PG_OK and writes nothing to run_genome / run_start / run_rows (which may then be NULL when cap == 0): call again with arrays
 * of *total_out entries.  Otherwise their first *total_out entries are the selected runs — genome, first sampled row of the
 * contig, rows — sorted by (window, genome, first row), window i's nruns_out[i] runs behind those of the windows before it,
 * and the same on every call.
 * PG_E_INVALID before anything is launched: fewer than 1 or more than 512 genomes, maxlen outside 1..4096, min_len < 1, a sampled
 * row outside its contig.  One launch of k_absence_runs over chunks of 4096 sampled rows (every row read once, all columns
 * followed together; integer atomics), the chunks' edges stitched on the host; synchronises. */
int pg_result_absence_runs(pg_result *r, int step, uint32_t stride, uint32_t nwin, const uint32_t *contig,
                           const uint64_t *starts, const uint64_t *ends, const uint32_t *select_words,
                           uint32_t maxlen, uint32_t min_len, uint32_t max_len,
                           uint64_t cap, uint32_t *run_genome, uint32_t *run_start, uint32_t *run_rows,
                           uint64_t *hist_out, uint64_t *absent_out, uint64_t *edge_out,
                           uint64_t *nruns_out, uint64_t *total_out);
/* presence profile: WHICH genomes carry a sequence, and how completely?  The question a query sequence that is not in the index
 * asks once its k-mers have been anchored against the table of every sample (a PG_ANCHOR_ROWS_ONLY result over the queries as
 * contigs; panagram_amd/search.py), reduced to six numbers per window and genome instead of pg_result_absence_runs' spectrum.
 * Window i = rows [starts[i], ends[i]) of contig contig[i]'s bitmap.1 rows in HBM (step 1, stride 1), n = ends[i] - starts[i];
 * no row outside a window is read or counted.  k is the result's own k: row j of the window is the k-mer at the window's bases
 * [j, j + k), and the window spans n + k - 1 bases.  select_words: the genomes to follow, as ceil(ngenomes / 32) words (bit g =
 * bit g % 32 of word g / 32; bits at and past ngenomes are ignored, in the words and in a row's last byte); NULL: all of them.
 * For a selected genome g, p[0..n) being its bit in each row of the window:
 *   profile_out[(i*ngenomes + g)*6 + 0]  hits     rows with the bit set
 *   profile_out[(i*ngenomes + g)*6 + 1]  runs     maximal runs of consecutive set rows
 *   profile_out[(i*ngenomes + g)*6 + 2]  longest  rows of the longest such run (0 if none)
 *   profile_out[(i*ngenomes + g)*6 + 3]  first    window-relative index of the first set row
 *   profile_out[(i*ngenomes + g)*6 + 4]  end      one past the last set row; first = end = 0 when hits == 0
 *   profile_out[(i*ngenomes + g)*6 + 5]  covered  |union over p[j] = 1 of [j, j + k)|: the bases of the window's n + k - 1 that
 *                                                 lie in at least one held k-mer.  A substituted base clears k rows but leaves one
 *                                                 base uncovered, so covered / (n + k - 1) reads as an identity where hits / n
 *                                                 does not.
 * With L running over the runs of absent rows that lie between two set rows of the window:
 *   covered = hits + sum of min(k - 1, L) + (k - 1 if hits > 0),   runs = #L + (1 if hits > 0).
 * Per window, over the selected genomes, when at least one is selected:
 *   rows_out[i*2 + 0]  all   rows in which every selected genome's bit is set
 *   rows_out[i*2 + 1]  none  rows in which no selected genome's bit is set
 * Every output for a genome outside the selection is 0; an empty selection, or an empty window (starts[i] == ends[i]), gives
 * zeros.
 * PG_E_INVALID before anything is launched: a NULL argument, fewer than 1 or more than 512 genomes, a window outside its contig,
 * n + k - 1 >= 2^32, a result without readable rows.  One launch of k_presence_profile over chunks of 4096 rows (every row read
 * once, all columns followed together; no atomics), then one download of the chunks' partials, which the host stitches;
 * synchronises. */
int pg_result_presence_profile(pg_result *r, uint32_t nwin, const uint32_t *contig,
                               const uint64_t *starts, const uint64_t *ends, const uint32_t *select_words,
                               uint32_t *profile_out, uint32_t *rows_out);
/* synteny: WHERE in genome B does the k-mer at a position of genome A lie?  The bitmap rows say whether B holds it; nothing in
 * the reference says where (scripts/pairwise_comp.py stops at per-genome column sums).  These calls work on two sequence sets,
 * the sides A (0) and B (1), and on these definitions:
 *   position  of a k-mer of a side: the global base offset of its first base in the concatenation of the side's contigs (the
 *             offset of contig c = the lengths of the contigs before it).  Windows holding a non-ACGT byte do not exist, contigs
 *             shorter than k have none.
 *   key, rc   the canonical k-mer, and rc = 1 when the forward value is greater than the reverse complement's (a reverse-
 *             complement palindrome: rc = 0).
 *   unique    a key is unique in a side when exactly one valid window of the side has it, on either strand.
 *   mate      position i of A has a mate iff its key is unique in A and unique in B: the word posB << 1 | (rcA xor rcB) — strand
 *             0 is +, 1 is - — and 0xFFFFFFFF for no mate.
 *   run       a maximal range [a, b) of consecutive k-mer positions of ONE contig of A whose mates have one strand and whose posB
 *             advances by +1 per position on +, by -1 on -.  Contig edges of A cut runs.
 * A position table holds, per distinct canonical k-mer, one position field per side in 16-byte slots in HBM; the number of slots
 * is the power of two at or above 2 * capacity_keys.  capacity_keys = the k-mer positions of both sides always suffices.
 * PG_E_INVALID: k outside 1..32, capacity_keys outside 1..2^32.  A table is used by one host thread at a time and is destroyed
 * before its context. */
typedef struct pg_postable pg_postable;
int pg_postable_create(pg_ctx *ctx, int k, uint64_t capacity_keys, pg_postable **out);
int pg_postable_destroy(pg_postable *pt);
/* every valid k-mer of seqs into the field of `side` (0 or 1): its position when the side holds the key once, a MULTI mark
 * beyond — the same whatever order the GPU took them in.  Each side is inserted once (PG_E_INVALID: a second time, a side's bases
 * above 2^31 - 1, before anything is launched).  Probing is bounded: a key that finds no slot makes the call return
 * PG_E_CAPACITY, and the table answers PG_E_CAPACITY from then on — destroy it and create a larger one.  One launch of
 * k_pos_insert; synchronises. */
int pg_postable_insert_seqset(pg_postable *pt, int side, const pg_seqset *seqs);
/* the mate word of every k-mer position of seqsA, which must be the sequence set inserted as side 0: a position whose key's
 * field of side 0 is not that very position has no mate.  mates_out: pg_seqset_total_kmers(seqsA, k) entries, the contigs'
 * positions back to back — a host pointer, or NULL: the array then only stays in HBM with the table (pg_synteny_segments reads
 * it there).  *nmated = the positions with a mate.  One launch of k_pos_mates; synchronises. */
int pg_postable_mates(pg_postable *pt, const pg_seqset *seqsA, uint32_t *mates_out, uint64_t *nmated);
/* the runs of an array of mate words on the host: ncontigs contigs of nkmers[c] entries each, back to back (at most 2^31 - 1 in
 * all: PG_E_INVALID beyond).  Entry j continues the run of entry j - 1 of its contig iff neither is 0xFFFFFFFF and mates[j] ==
 * mates[j - 1] + 2 (even words) or mates[j - 1] - 2 (odd words), in exact arithmetic.  nruns_per_contig[c] = the runs of contig c,
 * *total = their sum.
 * Capacity, as pg_result_find_runs: the counts are always computed.  If *total > cap, or cap == 0, the call returns PG_OK with the
 * counts filled and writes nothing to the four run arrays (which may then be NULL when cap == 0): call again with arrays of
 * *total entries.  Otherwise their first *total entries are the runs — contig, first position and exclusive end as k-mer
 * positions of that contig, the mate word of the first position — sorted by (contig, start), the same on every call.
 * Two launches of k_mate_runs (count, then emit; one when nothing is emitted) over chunks of 4096 positions, no atomics;
 * synchronises. */
int pg_mate_runs(pg_ctx *ctx, const uint32_t *mates, uint32_t ncontigs, const uint64_t *nkmers, uint64_t cap,
                 uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint32_t *run_mate,
                 uint64_t *nruns_per_contig, uint64_t *total);
/* all of it in one call: a table for both sides' k-mer positions, both inserts, the mates of A and their runs — the mates array
 * never leaves HBM.  Outputs and capacity as pg_mate_runs, over the contigs of seqsA (nruns_per_contig: one entry per contig of
 * seqsA); *nmated = the positions of A with a mate = the sum of the runs' lengths.  PG_E_INVALID before anything is launched: k
 * outside 1..32, a side of more than 2^31 - 1 bases, a sequence set of another context. */
int pg_synteny_segments(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint64_t cap,
                        uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint32_t *run_mate,
                        uint64_t *nruns_per_contig, uint64_t *total, uint64_t *nmated);
/* the HIP-event times, in milliseconds, of the kernels of this host thread's last pg_synteny_segments: ms_out[5] = k_pos_insert of
 * A, of B, k_pos_mates, k_mate_runs counting, k_mate_runs emitting (0 where a kernel did not run) — what tools/synteny_rate.py
 * reports. */
int pg_synteny_last_timing(float *ms_out);
/* blocks: the runs chained across substitutions and small insertions and deletions, on the GPU, so that only the blocks leave HBM.
 * With a run's n = end - start, strand = mate & 1, b = mate >> 1, the B position of its last k-mer bl = b + (n - 1) on strand 0,
 * b - (n - 1) on strand 1, and ml = bl << 1 | strand:
 *   kept         a run with n >= min_run; dropped runs do not exist for anything below.
 *   predecessor  of a kept run j: the nearest kept run i before it in the same contig of A.
 *   link i -> j  dA = start_j - (end_i - 1); dB = b_j - bl_i on strand 0, bl_i - b_j on strand 1 (signed, 64-bit).  It exists iff the
 *                strands agree, 1 <= dA <= max_gap, 1 <= dB <= max_gap, |dA - dB| <= max_shift, and the global B positions bl_i and
 *                b_j lie in the same contig of B.  A link is shifted when dA != dB.  (A substitution: dA = dB = k + 1; L bases
 *                inserted in B: dA = k, dB = k + L; d bases deleted from B: dA = k + d, dB = k.)
 *   block        a maximal chain of kept runs, each linked to its predecessor: contig of A, start of its first run, end of its
 *                last, mate_first = the first run's mate word, mate_last = the last run's ml, kmers = the sum of n, runs = their
 *                number, shifted = its shifted links.  B's positions are monotone inside a block: its B range in bases is
 *                [mate_first >> 1, (mate_last >> 1) + k) on strand 0, [mate_last >> 1, (mate_first >> 1) + k) on strand 1.
 * With min_run = 1 and max_gap = 1 the blocks are exactly the runs.
 * pg_run_blocks takes the runs from host arrays (nruns of them over ncontigsA contigs, as pg_mate_runs returns them) and the
 * lengths of B's ncontigsB contigs.  nblocks_per_contig[c] = the blocks of contig c of A, *total = their sum.  Capacity as
 * pg_mate_runs: the counts are always filled; nothing is written to the eight block arrays when cap == 0 (they may then be NULL) or
 * *total > cap; otherwise their first *total entries are the blocks, sorted by (contig, start), the same on every call.
 * PG_E_INVALID, before anything is launched: runs not sorted by (contig, start) or overlapping, a contig >= ncontigsA, end <= start,
 * a mate of 0xFFFFFFFF, a run whose B positions leave [0, sum(lensB)), min_run < 1, max_gap outside 1..2^31 - 1, max_shift above
 * 2^31 - 1, more than 2^31 - 1 runs.  Two launches of k_run_blocks (count, then emit; one when nothing is emitted) over chunks of
 * 4096 runs with a stitch of the chunks' edges on the host between them, no atomics; synchronises. */
int pg_run_blocks(pg_ctx *ctx, const uint32_t *run_contig, const uint32_t *run_start, const uint32_t *run_end,
                  const uint32_t *run_mate, uint64_t nruns, uint32_t ncontigsA, uint32_t ncontigsB, const uint64_t *lensB,
                  uint32_t min_run, uint32_t max_gap, uint32_t max_shift, uint64_t cap,
                  uint32_t *blk_contig, uint32_t *blk_start, uint32_t *blk_end, uint32_t *blk_mate_first, uint32_t *blk_mate_last,
                  uint32_t *blk_kmers, uint32_t *blk_runs, uint32_t *blk_shifted, uint64_t *nblocks_per_contig, uint64_t *total);
/* all of it in one call: table, both inserts, mates, the runs counted and emitted into HBM only, the blocks counted, stitched and
 * emitted — neither the mates nor the runs are downloaded.  Blocks and capacity as pg_run_blocks over the contigs of seqsA and
 * seqsB; *nmated as pg_synteny_segments, *nruns = all runs (kept or not).  PG_E_INVALID as pg_synteny_segments and for the three
 * parameters as pg_run_blocks. */
int pg_synteny_blocks(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint32_t min_run, uint32_t max_gap,
                      uint32_t max_shift, uint64_t cap,
                      uint32_t *blk_contig, uint32_t *blk_start, uint32_t *blk_end, uint32_t *blk_mate_first, uint32_t *blk_mate_last,
                      uint32_t *blk_kmers, uint32_t *blk_runs, uint32_t *blk_shifted, uint64_t *nblocks_per_contig, uint64_t *total,
                      uint64_t *nmated, uint64_t *nruns);
/* the HIP-event times of this host thread's last pg_synteny_blocks: ms_out[7] = the five of pg_synteny_last_timing, then
 * k_run_blocks counting and k_run_blocks emitting (0 where a kernel did not run). */
int pg_synteny_blocks_last_timing(float *ms_out);
/* variants: every link of every block classified, compared base by base on the GPU and emitted with its alleles — the differences
 * of B against A inside the blocks; only the variants leave HBM.  Run, kept, predecessor, link, dA, dB and strand are those of the
 * blocks above.  For a link i -> j write p = end_i - 1, the A position of run i's last k-mer; s = start_j; bl = the B position of
 * run i's last k-mer; b = b_j.  Positions of A are contig-relative, positions of B global, as in the mate words.
 *   overlap     t = max(0, k - min(dA, dB)); min(dA, dB) >= 1, so t <= k - 1.  The two matched flanks overlap by t bases on the
 *               shorter side — an indel inside a short tandem repeat — and the difference is placed at the leftmost place in A
 *               that the flanks allow.
 *   A allele    bases [posA, posA + lenA) of the contig of A, posA = p + k - t, lenA = dA - k + t.  Base posA - 1 always exists,
 *               lies in run i's last matched k-mer, is ACGT and identical in B: the anchor base a VCF indel needs.
 *   B allele    lenB = dB - k + t bases: [bl + k - t, b) on strand 0, [b + k, bl + t) on strand 1; posB is the lowest base of that
 *               range, which lies inside one contig of B (a link requires bl and b in the same contig).  "In A's orientation": as
 *               stored on strand 0, reverse-complemented on strand 1 — A base posA + i faces B base posB + i on strand 0 and the
 *               complement of B base posB + lenB - 1 - i on strand 1.
 *   mismatches  defined only when lenA == lenB: the number of i in [0, lenA) where the facing bases differ or either is non-ACGT.
 *               0 otherwise.
 *   class       0 same: lenA == lenB and mismatches == 0 (lenA == 0 included: the run broke on k-mers that are not unique, not on
 *               a difference) — counted, never emitted; 1 snp: lenA == lenB == 1 and mismatches == 1; 2 mnp: lenA == lenB >= 2 and
 *               mismatches >= 1; 3 ins: lenA == 0 < lenB; 4 del: lenB == 0 < lenA; 5 complex: both positive and unequal.
 *   N flag      either allele range holds a non-ACGT base.
 *   record      one per link of class != 0: contig of A, posA, lenA, posB, lenB, info = strand | class << 1 | code of A base
 *               posA - 1 << 4 | N flag << 6, mismatches, and two 64-bit words holding the first min(len, 32) bases of the A allele
 *               and of the B allele in A's orientation: 2 bits per base, base i at bits 2i and 2i + 1 (the seqset's own packing),
 *               the unused high bits zero.
 * Records are sorted by (contig of A, run j), which is (contig, posA), the same on every call.
 * Invariant: for every block, A's bases from the first run's start to the last run's end + k - 1, with each emitted record's A
 * allele replaced by its B allele in A's orientation, are exactly B's range of the block, reverse-complemented on strand 1.
 * pg_run_variants is pg_run_blocks's sibling: the runs from host arrays, ncontigsA and B's contig lengths from the seqsets.
 * class_counts[6] (the links of every class), *links (all links, class 0 included) and *total (the records) are always filled.
 * Capacity as pg_run_blocks: nothing is written to the nine record arrays when cap == 0 (they may then be NULL) or *total > cap.
 * PG_E_INVALID, before anything is launched: as pg_run_blocks, and k outside 1..32, a run whose k-mers' bases leave its contig of A
 * (end + k - 1 > its length) or do not lie inside one contig of B, max_gap above 65536 (a lane compares the gap's bases, 32 per
 * step).  The blocks' count pass and stitch, then two launches of k_link_variants (count, then emit; one when nothing is emitted)
 * with a scan of the chunks' records on the host between them, no atomics; synchronises. */
int pg_run_variants(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, const uint32_t *run_contig,
                    const uint32_t *run_start, const uint32_t *run_end, const uint32_t *run_mate, uint64_t nruns,
                    uint32_t min_run, uint32_t max_gap, uint32_t max_shift, uint64_t cap,
                    uint32_t *var_contig, uint32_t *var_posA, uint32_t *var_lenA, uint32_t *var_posB, uint32_t *var_lenB,
                    uint32_t *var_info, uint32_t *var_mismatches, uint64_t *var_alleleA, uint64_t *var_alleleB,
                    uint64_t *class_counts, uint64_t *links, uint64_t *total);
/* all of it in one call: table, both inserts, mates, runs (into HBM only), the blocks counted and stitched, the variants counted
 * and emitted — neither mates nor runs nor blocks are downloaded.  Records, counts and capacity as pg_run_variants; *nmated and
 * *nruns as pg_synteny_blocks, *nblocks = the blocks.  PG_E_INVALID as pg_synteny_blocks, and max_gap above 65536. */
int pg_synteny_variants(pg_ctx *ctx, int k, const pg_seqset *seqsA, const pg_seqset *seqsB, uint32_t min_run, uint32_t max_gap,
                        uint32_t max_shift, uint64_t cap,
                        uint32_t *var_contig, uint32_t *var_posA, uint32_t *var_lenA, uint32_t *var_posB, uint32_t *var_lenB,
                        uint32_t *var_info, uint32_t *var_mismatches, uint64_t *var_alleleA, uint64_t *var_alleleB,
                        uint64_t *class_counts, uint64_t *links, uint64_t *total, uint64_t *nmated, uint64_t *nruns,
                        uint64_t *nblocks);
/* the HIP-event times of this host thread's last pg_synteny_variants: ms_out[9] = the seven of pg_synteny_blocks_last_timing (the
 * blocks' emit pass does not run: 0), then k_link_variants counting and k_link_variants emitting. */
int pg_synteny_variants_last_timing(float *ms_out);
/* locate: WHERE in a genome do query sequences lie — chromosome, range, strand, every copy?  The mates above demand a k-mer that
 * occurs once on BOTH sides and cost a word per position of the streamed side; these calls demand it of the queries alone, stream
 * a genome of any size through the table and write only runs.  They work on a position table whose side 1 holds the queries Q
 * (pg_postable_insert_seqset(pt, 1, Q); side 0 stays empty and is ignored) and on these definitions:
 *   hit word  of k-mer position p of contig c of a streamed sequence set G: defined when the window is valid and the side-1 field w
 *             of its canonical key is a position — the key occurs exactly once in Q.  Then h = w xor rcG = posQ << 1 | (rcG xor
 *             rcQ), posQ global in Q's contigs laid end to end; 0xFFFFFFFF otherwise.  Nothing is required of the key's
 *             multiplicity in G: a key once in Q and three times in G gives three hits.
 *   hit run   the run of the synteny section with hit words in place of mates: a maximal [a, b) of consecutive k-mer positions of
 *             ONE contig of G, each continuing its predecessor by + 2 (even words) or - 2 (odd words).  Contig edges of G cut runs.
 *             For k >= 2 a run cannot span two queries: the global Q positions of neighbouring contigs' k-mers differ by at least k.
 * Positions of G are contig-relative everywhere: the streamed side has no limit on its total, only a single contig is limited, to
 * 2^32 - 1 k-mer positions.  Q keeps the limit of a side, 2^31 - 1 bases.
 * Two limits follow from the definitions.  K-mers that repeat among the queries (overlapping genes, family members given as
 * separate queries) count for nothing: pg_postable_hit_runs on Q itself says how many of a query's k-mers are left.  A query k-mer
 * that is a repeat in the genome yields many short runs there, and so many short blocks.
 * pg_postable_hit_runs: the hit runs of seqsG under the capacity protocol of pg_mate_runs — nruns_per_contig[c], *total (the runs)
 * and *nhits (the positions with a hit = the sum of the runs' lengths) are always filled, and hits_per_contig[c] = the positions of
 * contig c with a hit when it is not NULL; nothing is written to the four run arrays when cap == 0 (they may then be NULL) or
 * *total > cap; otherwise their first *total entries are the runs — contig, first position, exclusive end, hit word of the first
 * position — sorted by (contig, start), the same on every call.  Called with seqsG = Q itself it counts the queries' unique k-mers
 * per query.  It may be called any number of times on one table, with any sequence sets of the table's context.
 * pg_postable_locate: the hit runs kept in HBM, then blocks exactly as pg_run_blocks defines them with A = G and B = Q (the link rule,
 * the same-contig-of-B condition, min_run, max_gap and max_shift unchanged; mate_first / mate_last are hit words): only the blocks
 * leave the GPU.  seqsQ must be the set inserted as side 1 — the table remembers that side's base count and contig count.  Blocks
 * and capacity as pg_run_blocks over the contigs of seqsG; *nhits as above, *nruns = all runs (kept or not).
 * PG_E_INVALID, before anything is launched: a NULL argument, side 1 not inserted, a sequence set of another context, a contig of
 * seqsG of more than 2^32 - 1 k-mer positions, more than 2^31 - 1 chunks of 4096 positions; for pg_postable_locate also a seqsQ
 * that differs from side 1 in bases or contigs and the three parameters as pg_run_blocks.  PG_E_CAPACITY, before anything is
 * launched: the table overflowed.  (One answer cannot come before the count: pg_postable_locate on more than 2^31 - 1 runs is
 * PG_E_CAPACITY.)
 * Two launches of k_hit_runs (count, then emit; one when nothing is emitted) over chunks of 4096 positions — both probe the table,
 * which is only read — then pg_postable_locate's two of k_run_blocks; no atomics; synchronises. */
int pg_postable_hit_runs(pg_postable *pt, const pg_seqset *seqsG, uint64_t cap,
                         uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end, uint32_t *run_hit,
                         uint64_t *nruns_per_contig, uint64_t *hits_per_contig, uint64_t *total, uint64_t *nhits);
int pg_postable_locate(pg_postable *pt, const pg_seqset *seqsG, const pg_seqset *seqsQ, uint32_t min_run, uint32_t max_gap,
                       uint32_t max_shift, uint64_t cap,
                       uint32_t *blk_contig, uint32_t *blk_start, uint32_t *blk_end, uint32_t *blk_hit_first, uint32_t *blk_hit_last,
                       uint32_t *blk_kmers, uint32_t *blk_runs, uint32_t *blk_shifted, uint64_t *nblocks_per_contig, uint64_t *total,
                       uint64_t *nhits, uint64_t *nruns);
/* the HIP-event times of this host thread's last pg_postable_locate: ms_out[4] = k_hit_runs counting, k_hit_runs emitting,
 * k_run_blocks counting, k_run_blocks emitting (0 where a kernel did not run; after pg_postable_hit_runs the first two) — what
 * tools/locate_rate.py reports. */
int pg_locate_last_timing(float *ms_out);
/* copies: HOW OFTEN does a genome hold the k-mer at a position of a target sequence?  Every answer above is about presence (one bit
 * per genome and k-mer) or about k-mers that occur once (the position table); nothing in the reference counts the occurrences of a
 * k-mer along a sequence (scripts/pairwise_comp.py stops at column sums of presence bits).  These calls work on sequence sets —
 * targets T and a genome G — and on these definitions:
 *   depth_G(key)  the valid windows of G, over all its contigs, whose canonical k-mer is key: both strands count, windows holding a
 *                 non-ACGT byte do not exist, contigs shorter than k have none.
 *   d(p)          of k-mer position p of a target contig: depth_G(key(p)); p is invalid when its window is.  Targets are not
 *                 deduplicated: positions with one key read one depth.
 * A count table holds the distinct canonical k-mers of the targets as 8-byte keys in HBM — the number of slots is the power of two
 * at or above 2 * capacity_keys — and beside them nplanes planes of one 32-bit counter per slot, zero at creation: one plane per
 * genome counted.  capacity_keys = the targets' k-mer positions always suffices.  PG_E_INVALID: k outside 1..32, capacity_keys
 * outside 1..2^30, nplanes < 1; PG_E_CAPACITY: no memory for keys and planes.  A table is used by one host thread at a time and is
 * destroyed before its context. */
typedef struct pg_copytable pg_copytable;
int pg_copytable_create(pg_ctx *ctx, int k, uint64_t capacity_keys, uint32_t nplanes, pg_copytable **out);
int pg_copytable_destroy(pg_copytable *ct);
/* the key of every valid k-mer of `targets` into the table; may be called more than once, the keys accumulate (the planes keep what
 * they counted: a key that comes later has missed the genomes counted before).  *distinct = the keys this call added.  Probing is
 * bounded: a key that finds no slot makes the call return PG_E_CAPACITY, and the table answers PG_E_CAPACITY from then on — destroy
 * it and create a larger one.  One launch of k_copy_insert; synchronises. */
int pg_copytable_insert_seqset(pg_copytable *ct, const pg_seqset *targets, uint64_t *distinct);
/* `genome` streamed through the table, which is only read: plane[slot of key] += 1 for every valid window of the genome whose key
 * the table holds — added to what the plane held, exactly, whatever the contention (a homopolymer puts every lane on one
 * counter).  *hits = the windows counted = what this call added to the plane's sum.  PG_E_INVALID before anything is launched: a
 * plane >= nplanes, a genome of more than 2^32 - 1 k-mer positions (the counters are 32 bits).  One launch of k_copy_count;
 * synchronises. */
int pg_copytable_count_seqset(pg_copytable *ct, uint32_t plane, const pg_seqset *genome, uint64_t *hits);
/* every counter of one plane back to zero */
int pg_copytable_clear_plane(pg_copytable *ct, uint32_t plane);
/* the depths along the contigs of `seqs` — any sequence set of the table's context, not only an inserted one: a key the table does
 * not hold reads depth 0 — in planes plane0 .. plane0 + nplanes - 1 (g below counts from plane0).  With n = pg_seqset_ncontigs:
 *   valid_out[t]                   t < n: the valid k-mer positions of contig t
 *   hist_out[(t*nplanes + g)*64 + c]  c < 64: the valid positions of contig t with min(d, 63) == c in plane g (they sum to valid_out[t])
 *   depth_out                      NULL, or nplanes * pg_seqset_total_kmers(seqs, k) entries: [g][the contigs' positions back to
 *                                  back] = min(d, 65534), 65535 at an invalid position
 * PG_E_INVALID before anything is launched: a NULL argument, nplanes < 1 or a range that leaves the table's planes, a sequence set
 * of another context.  Launches of k_copy_profile over chunks of 4096 positions (no block waits for another, no global atomics),
 * the chunks' partial histograms summed on the host in 64 bits; synchronises. */
int pg_copytable_profile(pg_copytable *ct, const pg_seqset *seqs, uint32_t plane0, uint32_t nplanes, uint64_t *hist_out,
                         uint64_t *valid_out, uint16_t *depth_out);
/* place: WHICH of the indexed genomes does an unassembled sample resemble along an anchor?  The sample's reads have been counted into
 * `plane` of a count table that holds the anchor's k-mers (pg_copytable_insert_seqset of `anchor`, pg_copytable_count_seqset of the
 * reads); `rows` holds the anchor's finished bitmap rows.  Window i = rows [starts[i], ends[i]) of contig contig[i] of the result, as
 * for pg_result_presence_profile.  With k the table's k:
 *   row correspondence  row r of contig c is the k-mer at bases [r, r + k) of contig c of `anchor`
 *   validity            row r is valid when that window of the anchor holds no non-ACGT base
 *   sample column       s(r) = 1 when the plane's counter of the row's canonical k-mer is >= min_count; a key the table does not
 *                       hold reads 0, as in pg_copytable_profile
 *   valid_out[i]                 the valid rows of window i
 *   held_out[i]                  the valid rows with s(r) = 1
 *   col_out[i*ngenomes + g]      the valid rows with bit g set
 *   both_out[i*ngenomes + g]     the valid rows with bit g set and s(r) = 1
 * The bits at and past ngenomes in a row's last byte never count; an empty window (starts[i] == ends[i]) gives zeros.
 * PG_E_INVALID before anything is launched: a NULL argument, min_count == 0, a plane >= nplanes, handles of different contexts,
 * fewer than 1 or more than 512 genomes, rows of a k that is not the table's, an anchor whose number of contigs is not the rows', a
 * contig whose row count is not len - k + 1 (0 for len < k), a window outside its contig, a result without readable rows.  Launches
 * of k_sample_agree over chunks of 4096 rows (one lookup and one row read per position, all columns followed together by ballot
 * transpose; no atomics, no block waits for another), the chunks' 32-bit partials summed on the host in 64 bits; synchronises. */
int pg_copytable_sample_agree(pg_copytable *ct, uint32_t plane, uint32_t min_count, const pg_seqset *anchor, pg_result *rows,
                              uint32_t nwin, const uint32_t *contig, const uint64_t *starts, const uint64_t *ends,
                              uint64_t *valid_out, uint64_t *held_out, uint64_t *col_out, uint64_t *both_out);
/* the HIP-event times, in milliseconds, of this host thread's last calls: ms_out[2] = the kernels of the last pg_seqset_from_fastq
 * (scan, offsets, join and pack together), k_sample_agree (all its launches) of the last pg_copytable_sample_agree — what
 * tools/place_rate.py reports. */
int pg_place_last_timing(float *ms_out);
/* the HIP-event times, in milliseconds, of this host thread's last calls: ms_out[3] = k_copy_insert of the last insert, k_copy_count
 * of the last count, k_copy_profile (all its launches) of the last profile — what tools/copies_rate.py reports. */
int pg_copies_last_timing(float *ms_out);
/* genotype: WHICH ALLELE of a variant does a sample carry?  The two calls work on allele ranges of a sequence set instead of whole
 * contigs (pg_genotype.hip).  With k the table's k:
 *   allele range    (contig[i], start[i], len[i]): bases [s, s + l) of that contig, s + l <= the contig's length L; l = 0 is the
 *                   junction between base s - 1 and base s
 *   allele windows  the k-mer positions p of the contig with max(0, s - k + 1) <= p < min(L - k + 1, s + l): every window that
 *                   overlaps the allele — for l = 0 the k - 1 windows that hold both neighbours of the junction; none when L < k,
 *                   none for a junction at s = 0 or s = L; a window holding a non-ACGT base does not exist
 *   informative     an allele window with canonical key K is informative when own[K] == 1 && other[K] == 0 in the planes named:
 *                   the k-mer occurs once in the genome the allele comes from and nowhere in the other; it is seen when also
 *                   sample[K] >= min_count.  A key the table does not hold reads 0 in every plane and is never informative.
 * pg_copytable_insert_ranges puts the keys of the ranges' allele windows into the table: keys accumulate as with
 * pg_copytable_insert_seqset, *distinct = the keys this call added, the same sticky PG_E_CAPACITY, and planes counted before it
 * have missed its keys.  pg_copytable_allele_support reduces three planes along every range: windows_out[i] = the allele windows
 * that exist, inf_out[i] = the informative ones, seen_out[i] = the seen ones, depth_out[i] = the sum of sample[K] over the
 * informative ones, in 64 bits.
 * PG_E_INVALID before anything is launched: a NULL argument with n > 0, a sequence set of another context, a contig number out of
 * range, start + len beyond the contig, a plane >= nplanes, min_count == 0, own_plane == other_plane, more than 2^31 - 1 pieces.
 * n == 0 launches nothing and returns PG_OK.  The host cuts every range's windows into pieces of at most 64, one wave's work
 * (k_allele_insert, k_allele_support: no wave loops over an allele, no block waits for another, the support without atomics); the
 * pieces' partials are summed per range on the host in 64 bits, the piece list going out in slices when the partials exceed the
 * 256 MiB pg_copytable_profile caps itself at.  Both calls synchronise. */
int pg_copytable_insert_ranges(pg_copytable *ct, const pg_seqset *seqs, uint64_t n, const uint32_t *contig, const uint64_t *start,
                               const uint64_t *len, uint64_t *distinct);
int pg_copytable_allele_support(pg_copytable *ct, const pg_seqset *seqs, uint64_t n, const uint32_t *contig, const uint64_t *start,
                                const uint64_t *len, uint32_t own_plane, uint32_t other_plane, uint32_t sample_plane,
                                uint32_t min_count, uint64_t *windows_out, uint64_t *inf_out, uint64_t *seen_out, uint64_t *depth_out);
/* the HIP-event times, in milliseconds, of this host thread's last calls: ms_out[2] = k_allele_insert of the last
 * pg_copytable_insert_ranges, k_allele_support (all its launches) of the last pg_copytable_allele_support — what
 * tools/genotype_rate.py reports. */
int pg_genotype_last_timing(float *ms_out);
/* screen: WHICH of the indexed genomes does a sample hold, and how much of each?  The sample — read sets joined by
 * pg_seqset_from_fastq, or the contigs of an assembly — is streamed through the pan table itself and counted per slot; one pass over
 * the slots joins the counts with the presence masks (pg_screen.hip).  With k the table's k (a sequence set carries none: its
 * windows are cut at the table's), N its genomes:
 *   depth(key)   the valid windows of the sample whose canonical k-mer is key, both strands, summed over every sequence set added
 *                since the screen was created or cleared; it saturates at 255.  Windows holding a non-ACGT byte do not exist,
 *                contigs shorter than k have none.
 * A screen owns one byte per slot of the table, zero at creation, and holds the table as a result does (a destroyed table goes when
 * its last screen does).  The bytes belong to ONE geometry of ONE table: the screen records the table's lines (their address, their
 * number, the slots of a line, the layout) and its key count, and pg_screen_add_seqset / pg_screen_result return PG_E_INVALID once
 * any of them differs — after a re-hash, an insert that added keys, a clear or a regrow behind the handle.  Create a new screen then.
 * The table itself is only read.  PG_E_CAPACITY: no memory for the bytes.  A screen is used by one host thread at a time. */
typedef struct pg_screen pg_screen;
int pg_screen_create(pg_table *tbl, pg_screen **out);
int pg_screen_destroy(pg_screen *s);
/* the byte of the slot of every valid window of `seqs` whose key the table holds += 1, saturating at 255 — exactly, whatever the
 * contention (a homopolymer puts every lane on one byte; a byte's three neighbours in its dword are never touched).  *windows = the
 * valid windows of seqs, *hits = those whose key the table holds.  PG_E_INVALID before anything is launched: a NULL argument, a
 * sequence set of another context, a stale screen.  One launch of k_table_mark; synchronises. */
int pg_screen_add_seqset(pg_screen *s, const pg_seqset *seqs, uint64_t *windows, uint64_t *hits);
/* one pass over the table's slots (those pg_table_pair_counts counts: a key, neither empty nor retired), M = the slot's mask with
 * the bits at and past N cleared, n = popcount(M), d = its depth:
 *   distinct[g]  g < N: the keys with bit g            seen[g]          those of them with d >= min_count
 *   priv[g]      the keys whose only bit is g          priv_seen[g]     those of them with d >= min_count
 *   occ[n]       n <= N: the keys of exactly n genomes seen_occ[n]      those of them with d >= min_count
 *   depth_hist[c]  c < 64: the keys with min(d, 63) == c                core_depth_hist[c]  the same of the keys with n == N
 *   *nkeys       the keys counted
 * Any output may be NULL.  The bytes stay as they are: results at several min_count come from one plane.  PG_E_INVALID before
 * anything is launched: min_count outside 1..255, more than 512 genomes, a stale screen.  One launch of k_table_screen on the
 * context's stream; synchronises. */
int pg_screen_result(pg_screen *s, uint32_t min_count, uint64_t *distinct, uint64_t *seen, uint64_t *priv, uint64_t *priv_seen,
                     uint64_t *occ, uint64_t *seen_occ, uint64_t *depth_hist, uint64_t *core_depth_hist, uint64_t *nkeys);
/* every byte back to zero (the next sample) */
int pg_screen_clear(pg_screen *s);
/* the HIP-event times, in milliseconds, of this host thread's last calls: ms_out[2] = k_table_mark of the last pg_screen_add_seqset,
 * k_table_screen of the last pg_screen_result — what tools/screen_rate.py reports. */
int pg_screen_last_timing(float *ms_out);
/* novel: WHAT does a sample hold that no indexed genome does?  The reverse of the screen: the sample is streamed through the pan
 * table once, and the windows that MISS it are counted in a key table of the sample's own (pg_novel.hip), which is built while the
 * sample streams and grows in front of every sequence set.  With k the table's k:
 *   novel key    the canonical k-mer of a valid window of the sample that the pan table does not hold
 *   depth(key)   the valid windows of the sample with that key, both strands, summed over every sequence set added since the handle
 *                was created or cleared; exact in 32 bits.  solid: depth >= min_count.
 *   novel run    a maximal run [start, end) of consecutive valid k-mer positions of one contig whose keys are all novel; contig
 *                ends and invalid windows cut runs.  left_held = position start - 1 exists, is valid and the pan table holds its
 *                key; right_held the same of position end.
 * A handle owns 12 bytes per slot (an 8-byte key, a 32-bit depth), the power of two at or above 2 capacity_keys slots at creation,
 * and holds the pan table as a screen does: it records the table's geometry and key count and pg_novel_add_seqset, pg_novel_result
 * and pg_novel_keys return PG_E_INVALID once any of them differs (keys filtered by another table answer nothing).  The pan table is
 * only read.  PG_E_INVALID: capacity_keys outside 1..2^30; PG_E_CAPACITY: no memory.  A handle is used by one host thread at a time. */
typedef struct pg_novel pg_novel;
int pg_novel_create(pg_table *tbl, uint64_t capacity_keys, pg_novel **out);
int pg_novel_destroy(pg_novel *nv);
/* every slot free again, the windows counted back to zero (the next sample); the slots stay as many as they have grown to */
int pg_novel_clear(pg_novel *nv);
/* every valid window of `seqs` whose key the pan table lacks: its key claimed in the novel table, its depth += 1 — exactly, whatever
 * the contention.  *windows = the valid windows of seqs, *hits = those whose key the pan table holds, *new_keys = the keys this call
 * claimed.  The call reserves before it launches: when the keys held plus the set's k-mer positions pass half the slots the table
 * is re-hashed on the device into one that holds them at a load of 0.5 at the most (k_novel_grow), so an add never overflows.
 * Before anything is launched, the handle usable afterwards: PG_E_CAPACITY when that takes more than 2^31 slots (2^30 keys and
 * positions: add smaller sequence sets) or the memory is not there; PG_E_INVALID for a NULL argument, a sequence set of another
 * context, a stale handle, or when the windows added so far plus this set's positions pass 2^32 - 1 (the depths are 32 bits).  A
 * claim that gives up all the same makes the handle answer PG_E_CAPACITY until it is cleared.  One launch of k_novel_count;
 * synchronises. */
int pg_novel_add_seqset(pg_novel *nv, const pg_seqset *seqs, uint64_t *windows, uint64_t *hits, uint64_t *new_keys);
/* *nkeys = the novel keys held, *nslots = the slots, *grown = the times the table has grown.  Any output may be NULL. */
int pg_novel_stats(pg_novel *nv, uint64_t *nkeys, uint64_t *nslots, uint64_t *grown);
/* one pass over the slots (k_novel_scan): *nkeys = the novel keys, *solid = those with depth >= min_count, *solid_windows = the sum
 * of their depths, depth_hist[c], c < 64 = the keys with min(depth, 63) == c.  Any output may be NULL; the table stays as it is:
 * results at several min_count come from one table.  PG_E_INVALID: min_count == 0. */
int pg_novel_result(pg_novel *nv, uint32_t min_count, uint64_t *nkeys, uint64_t *solid, uint64_t *solid_windows, uint64_t *depth_hist);
/* the solid keys and their depths, in slot order — the same on every call between two adds, no particular order otherwise: the
 * first min(cap, *n) of them to keys / depths, *n = all of them always (cap 0: only counted). */
int pg_novel_keys(pg_novel *nv, uint32_t min_count, uint64_t cap, uint64_t *keys, uint32_t *depths, uint64_t *n);
/* the novel runs of the contigs of `seqs` against the pan table (k_novel_runs; no handle: the novel table is not touched), sorted by
 * (contig, start): the first min(cap, *nruns) of them to the five arrays, positions contig-relative; *nruns = all of them, *windows
 * = the valid windows of seqs, *novel_windows = those whose key the table lacks = the sum of the runs' lengths — always.
 * PG_E_INVALID before anything is launched: a NULL argument, a sequence set of another context, a contig of more than 2^32 - 1
 * k-mer positions. */
int pg_novel_runs(pg_table *tbl, const pg_seqset *seqs, uint64_t cap, uint32_t *run_contig, uint32_t *run_start, uint32_t *run_end,
                  uint8_t *left_held, uint8_t *right_held, uint64_t *nruns, uint64_t *windows, uint64_t *novel_windows);
/* the HIP-event times, in milliseconds, of this host thread's last calls: ms_out[4] = k_novel_count and k_novel_grow of the last
 * pg_novel_add_seqset (0: it did not grow, or grew an empty table), k_novel_scan of the last pg_novel_result or pg_novel_keys (both
 * passes), k_novel_runs of the last pg_novel_runs (both passes) — what tools/novel_rate.py reports. */
int pg_novel_last_timing(float *ms_out);
/* unitigs: the solid novel k-mers compacted into sequences on the GPU (pg_unitigs.hip).  Over a handle and a min_count, 2 <= k <= 32:
 *   node             a solid novel key.  Keys below min_count and k-mers the pan table holds are not nodes: they cut paths.
 *   oriented k-mer   w: a node's k-mer x or its reverse complement; canon(w) is its node
 *   out(w)           the bases b for which canon(w[1:] + b) is a node;  in(w) = out(rc(w)), complemented
 *   link byte        of node x in the canonical orientation (first base most significant, A < C < G < T): bit b (b < 4) is set when
 *                    canon(x[1:] + b) is a node, bit 4 + b when canon(b + x[:-1]) is a node
 *   compactable edge w -> w': out(w) = {the base that gives w'}, in(w') holds exactly one base, canon(w) != canon(w') (no self-loop,
 *                    no hairpin w -> rc(w)), and neither node is its own reverse complement
 *   unitig           a maximal path w1 .. wn along compactable edges: w1 plus the last base of each further wi, n + k - 1 bases.
 *                    Every node lies in exactly one unitig; a node that is its own reverse complement is a unitig of n = 1.
 *   circular unitig  a component in which every node has a compactable edge on both sides: emitted once, from its smallest key in
 *                    that key's canonical orientation to the right, n nodes and n + k - 1 bases (the last k - 1 repeat the first)
 *   linear unitig    emitted once, by the walk from the end with the smaller key (n = 1: in the canonical orientation): the
 *                    sequence or its reverse complement, whichever that walk spells
 *   depth_sum        the sum of the nodes' depths
 * pg_novel_links: the solid keys and their link bytes, in slot order, under the capacity protocol of pg_novel_keys.
 * pg_novel_unitigs: unitig u < min(cap_unitigs, *nunitigs) has kmers[u] nodes, depth_sum[u], circular[u] (0 / 1) and the bases
 * bases[offsets[u] .. offsets[u] + kmers[u] + k - 1), ASCII; bases at or past cap_bases and entries at or past cap_unitigs are never
 * written (a unitig's bases may be cut).  *nunitigs, *nbases and *ncircular are the full numbers always; caps of 0: only counted.  The
 * linear unitigs stand first, each kind in slot order of its starting node: the same on every call between two adds.  The handle
 * keeps two byte planes of its slots and the walks' counts for the last min_count between a counting and a filling call;
 * pg_novel_add_seqset and pg_novel_clear drop them.  One lane walks one unitig: a unitig of L k-mers costs L dependent memory round
 * trips, a circular one L^2 probes spread over L lanes.  PG_E_INVALID: min_count == 0, k < 2, a stale handle, a NULL argument;
 * PG_E_CAPACITY: no memory for the two planes or the outputs; PG_E_INTERNAL: a walk reached its bound (every walk is bounded by
 * the solid keys, every lookup by the table's probe limit: a wrong plane is an error, never a hang). */
int pg_novel_links(pg_novel *nv, uint32_t min_count, uint64_t cap, uint64_t *keys, uint8_t *links, uint64_t *n);
int pg_novel_unitigs(pg_novel *nv, uint32_t min_count, uint64_t cap_unitigs, uint64_t cap_bases, uint64_t *offsets, uint32_t *kmers,
                     uint64_t *depth_sum, uint8_t *circular, uint8_t *bases, uint64_t *nunitigs, uint64_t *nbases, uint64_t *ncircular);
/* ms_out[3] = the HIP-event times, in milliseconds, of k_unitig_links, of k_unitig_walk's linear round (all its passes) and of its
 * circular round (0: not run), as the handle of this host thread's last pg_novel_links / pg_novel_unitigs call has summed them
 * since its planes were built — the sums are the handle's, two handles used in turn do not mix: a call that builds the planes
 * (another min_count, or the first after an add or a clear) starts from zero, a call that finds them kept adds its passes — a
 * counting call and the filling call behind it read as one.  All 0 behind a call that found no solid key.  What
 * tools/novel_unitigs_rate.py reports. */
int pg_novel_unitigs_last_timing(float *ms_out);
/* Error tips clipped and bubbles popped on the graph of the solid keys at min_count, before it is compacted (pg_unitigs.hip:
 * k_unitig_clean; the header of that file states the rule in full).  With the vocabulary above, over the graph G of the current nodes:
 *   side    the right side of a linear unitig U = w1 .. wn is out(wn), the left side in(w1): DEAD when empty, ATTACHED BY v when it
 *           holds one base and the oriented k-mer v it names is a node outside U that is not its own reverse complement
 *   tip     n <= tip_kmers, one side dead, the other attached by v; S = the other oriented k-mers with an edge into v on that side;
 *           clipped iff S is not empty and depth(attached end node) * 1000 <= ratio_milli * max over S of depth(s).  A unitig dead
 *           on both sides, and a fork whose only sibling is a k-mer the table holds, are never tips.
 *   bubble  n <= bubble_kmers, attached by p on the left and by q on the right; a parallel U' of n' <= bubble_kmers nodes leaves p
 *           by another successor and is attached by the same p and q; with e(X) = min(depth of X's two end nodes), U is popped iff
 *           some parallel U' has e(U) * 1000 <= ratio_milli * e(U').  ratio_milli < 1000: two branches never remove each other, and
 *           an even (heterozygous) bubble stays.
 *   rounds  every round decides on the graph the round before left and drops what it found at once; the rounds stop at the first
 *           that drops nothing, or after max_rounds.  Each is one k_unitig_links pass and one k_unitig_clean pass.
 * stats[5] = {tips clipped, their k-mers, bubbles popped, their k-mers, rounds that dropped something}.  Behind it pg_novel_links and
 * pg_novel_unitigs with the same min_count answer for the cleaned graph — a dropped key is no node: absent from the links, no part
 * of any unitig, a cut in its neighbours' link bytes.  The raw graph comes back with max_rounds == 0, another min_count,
 * pg_novel_add_seqset or pg_novel_clear.  1 <= tip_kmers, bubble_kmers <= 1024; 1 <= ratio_milli <= 999; max_rounds <= 64.
 * PG_E_INVALID: a parameter out of range, min_count == 0, k < 2, a stale handle, a NULL argument; PG_E_CAPACITY: no memory for the
 * three byte planes; PG_E_INTERNAL: the planes contradict the table (every walk is bounded by tip_kmers or bubble_kmers). */
int pg_novel_clean(pg_novel *nv, uint32_t min_count, uint32_t tip_kmers, uint32_t bubble_kmers, uint32_t ratio_milli, uint32_t max_rounds,
                   uint64_t *stats);
/* ms_out[2] = the HIP-event milliseconds of the k_unitig_links passes and of the k_unitig_clean passes of this host thread's last
 * pg_novel_clean (0: not run). */
int pg_novel_clean_last_timing(float *ms_out);
/* exact k nearest neighbours among the rows of a dense float32 matrix, under squared Euclidean distance: the neighbour
 * graph that umap.UMAP(n_neighbors, ...).fit_transform(paircounts) builds first (panagram/index.py:1131-1137: run_umap, on the
 * bins x genomes pair-count matrix of a chromosome or of the whole genome).  X is n x ncols, row-major, a host pointer (a
 * device pointer works too: the copies are hipMemcpyDefault); seg holds nseg + 1 ascending row offsets from 0 to n, and a row
 * of segment s searches the rows [seg[s], seg[s+1]) only, itself included — every chromosome of an anchor in one launch
 * (seg NULL: one segment of all n rows).  idx_out / d2_out are n x k: the global row numbers and distances of each row's k
 * nearest rows, sorted by (d2, row number) ascending — equal distances: the lower row number first; the row itself
 * appears at distance 0 under the same rule — padded with (-1, +inf) where a segment has fewer than k rows.
 * d2(i, j) is EXACTLY the float32 sum over g = 0 .. ncols-1, in that order, of (X[i][g] - X[j][g])^2 with every subtract,
 * multiply and add rounded to float32 (no fused multiply-add).  X must hold no NaN.  1 <= k <= 32, 1 <= ncols <= 4096,
 * n < 2^31: PG_E_INVALID otherwise, before anything is launched.  Staged through the context's stream (k_knn_rows);
 * synchronises. */
int pg_knn_rows(pg_ctx *ctx, const float *X, uint64_t n, uint32_t ncols, uint32_t k, const uint64_t *seg, uint32_t nseg,
                int32_t *idx_out, float *d2_out);
/* stream the whole bitmap.1 (step 1) or bitmap.100 (step 100) payload of the result — every
 * contig, in order — from HBM into a BGZF file + .gzi index (gzi_path may be NULL): D2H through
 * pinned double buffers on a private stream overlapped with multi-threaded deflate.  Replaces
 * bgzf_open/bgzf_write/bgzf_index_dump/bgzf_close of cpp/anchor.cpp:46-55,102-106,167,177.  Waits
 * for the run's kernels; may be called from another host thread than the one enqueueing work.
 * level: a zlib level 0..9 for the host path (Z_RLE for one-byte rows, the library's row-aware
 * encoder for wider ones) — or -2: the BGZF blocks are compressed ON THE GPU (k_row_deflate: one
 * workgroup per 65280-byte block, matches one row back, dynamic Huffman, CRC32), the host only
 * appends the finished blocks to the file (nthreads unused). */
int pg_result_write_bgzf(pg_result *r, int step, const char *gz_path, const char *gzi_path, int level,
                         int nthreads);
/* the same for contigs first_contig .. first_contig+ncontigs-1 only: one anchor genome of a result
 * that spans several (pg_seqset_concat / pg_result_coschedule) */
int pg_result_write_bgzf_range(pg_result *r, int step, uint32_t first_contig, uint32_t ncontigs,
                               const char *gz_path, const char *gzi_path, int level, int nthreads);
/* Launch-order hint for a result over SEVERAL anchor genomes (contig_group[c] = genome of contig
 * c; NULL restores launch order): the reference anchors its FASTAs in parallel threads
 * (cpp/anchor.cpp:217-223); here all of them share one kernel launch whose tiles interleave the
 * genomes piece by piece (piece_tiles tiles, 0 = default), each genome traversed at the same
 * relative pace, so that homologous regions — which need the same table lines — run side by side
 * and the lines are fetched from HBM once instead of once per genome.  Results do not depend on
 * the schedule. */
int pg_result_coschedule(pg_result *r, const uint32_t *contig_group, uint32_t piece_tiles);
/* the same when the genomes do not list their contigs in corresponding order: contig_class[c] names the homology
 * class of contig c (e.g. the chromosome: equal record ids in different FASTAs); the classes are scheduled one after
 * the other, within a class the genomes' contigs side by side as above.  (With shuffled contig order the plain
 * co-schedule degrades to the one-launch-per-genome rate: tools/indel_cosched.py --shuffle-contigs.) */
int pg_result_coschedule_classes(pg_result *r, const uint32_t *contig_group, const uint32_t *contig_class,
                                 uint32_t piece_tiles);
/* the same with the contigs cut into nranges consecutive ranges (range i starts at contig range_first_contig[i];
 * the first at 0) that are scheduled independently: pg_anchor_run_range over one or several whole ranges then
 * follows the schedule too (any other range runs in launch order) */
int pg_result_coschedule_ranges(pg_result *r, const uint32_t *contig_group, uint32_t piece_tiles,
                                const uint32_t *range_first_contig, uint32_t nranges);
/* column sums of contigs idx .. idx+ncontigs-1 (ncontigs x ngenomes u64); pg_result_colsums is
 * their total */
int pg_result_contig_colsums(pg_result *r, uint32_t idx, uint32_t ncontigs, uint64_t *colsums);
int pg_result_download(pg_result *r, uint32_t idx, uint8_t *bitmap1, uint8_t *bitmap100,
                       uint32_t *bins);
/* The small outputs of contigs first .. first+ncontigs-1 in ONE call (an assembly of 20 000 contigs paid 26 us per
 * contig for pg_result_contig_info + pg_result_download): the geometry into four arrays of ncontigs entries each (any
 * may be NULL) and, when bins != NULL, the contigs' bin rows back to back — bins_words must be the sum of
 * nbins[i] * (ngenomes + 1) — in one device-to-host copy; synchronises.  What KMCdb::write_bits accumulates per chunk
 * (cpp/anchor.cpp:179-189), per contig. */
int pg_result_contigs_small(pg_result *r, uint32_t first, uint32_t ncontigs, uint64_t *nkmers, uint64_t *nrows100,
                            uint32_t *nbins, uint32_t *binlen, uint32_t *bins, uint64_t bins_words);
/* per-genome column sums over ALL contigs of the seqset (ngenomes u64); synchronises */
int pg_result_colsums(pg_result *r, uint64_t *colsums);
/* device pointers (for benchmarking / checksums without PCIe traffic) */
int pg_result_device_ptrs(pg_result *r, void **d_bitmap1, uint64_t *bitmap1_bytes,
                          void **d_bitmap100, uint64_t *bitmap100_bytes);

/* one-shot convenience for a single contig held in host memory: upload, pack,
 * anchor, download.  nkmers = len-k+1 (0 and a warning-free no-op when len<k:
 * the reference underflows here, cpp/anchor.cpp:115).  Any output may be NULL. */
int pg_anchor_contig(pg_table *tbl, const char *ascii, uint64_t len, uint8_t *bitmap1,
                     uint8_t *bitmap100, uint32_t *bins, uint64_t *colsums, uint64_t *nkmers);

/* literal equivalent of CKMCFile::GetCountersForRead(seq, vector<uint32>&)
 * (call sites cpp/anchor.cpp:148, index.py:934-935) for group db_idx:
 * out[i] = counter of the canonical k-mer of ascii[i:i+k], 0 if absent or if the
 * window holds a byte outside ACGTacgt.  out has len-k+1 entries. */
int pg_counters_for_read(pg_table *tbl, int db_idx, const char *ascii, uint64_t len,
                         uint32_t *out);

/* ---- BGZF + .gzi writer (host, zlib, multi-threaded) -------------------
 * Reference: htslib bgzf_open/bgzf_index_build_init/bgzf_write/
 * bgzf_index_dump/bgzf_close (cpp/anchor.cpp:46-47,53-54,102-106,167,177) and
 * bgzip.BGZipWriter + `bgzip -rI` (index.py:1035-1037,1091-1094).  Blocks hold
 * <= 65280 uncompressed bytes; X.gzi = u64 n, n x (u64 compressed_off, u64
 * uncompressed_off) for blocks 1..n (read by index.py:793-799).
 * level: zlib level 0..9 (other values: 6), optionally | PG_BGZF_RLE = zlib's Z_RLE strategy
 * (matches at distance 1 only).  For ONE-byte rows (N <= 8) runs of equal rows are byte runs:
 * same compression ratio as the default strategy, 6.6x faster (tools/zstrategy.py); useless for
 * wider rows.  pg_result_write_bgzf adds it by itself for one-byte rows.
 * | PG_BGZF_ROWS(w): the payload is rows of w bytes (2..255): a row-aware DEFLATE encoder (matches
 * "same byte as one row earlier" only, dynamic Huffman per block) replaces zlib's matcher, which
 * runs at ~60 MB/s/core on such data; falls back to zlib per block if its output does not fit.
 * pg_result_write_bgzf uses it for rows wider than one byte. */
#define PG_BGZF_RLE 0x100
#define PG_BGZF_ROWS(w) (((w) & 0xff) << 16)
int pg_bgzf_open(const char *path, int level, int nthreads, pg_bgzf **out);
int pg_bgzf_write(pg_bgzf *w, const void *data, size_t len);
/* writes the EOF block, closes the file and, if gzi_path != NULL, the index */
int pg_bgzf_close(pg_bgzf *w, const char *gzi_path);

/* ---- BGZF inflated on the GPU (k_bgzf_inflate, pg_inflate.hip) -------
 * Reference: the block-by-block host inflate of Bio.bgzf's BgzfReader (index.py:615-651, 827-845) and of
 * `panagram annotate` reading bitmap.1.gz back (index.py:971-1010).  One workgroup inflates one BGZF block: full RFC 1951
 * (stored, fixed and dynamic Huffman blocks, several per member, the empty EOF member), CRC32 and ISIZE checked on the
 * device.  Every input byte is untrusted: a malformed block returns PG_E_FORMAT, pg_last_error() names its file offset
 * (the first bad block), and the context stays usable.
 *
 * pg_bgzf_inflate: whole blocks held in host memory -> d_out (device memory, out_bytes).  coffs / roffs (nblocks + 1 entries
 * each: compressed offsets into comp, payload offsets; roffs may be NULL): block i = comp[coffs[i], coffs[i+1]), its payload
 * at d_out + roffs[i].  coffs == NULL: the blocks are found by walking BSIZE and ISIZE through all comp_bytes (nblocks and
 * roffs unused).  *raw_bytes (may be NULL) = payload bytes written.  Synchronises. */
int pg_bgzf_inflate(pg_ctx *ctx, const void *comp, uint64_t comp_bytes, uint32_t nblocks, const uint64_t *coffs,
                    const uint64_t *roffs, void *d_out, uint64_t out_bytes, uint64_t *raw_bytes);
/* the rows of contigs first_contig .. first_contig+ncontigs-1 of a result (a rows container: pg_seqset_create from lengths +
 * pg_result_create_rows) read back from a bitmap.<step>.gz: the result's contig 0 starts at row file_row0 of the file's
 * payload (0 when the result holds the file's contigs from the first one), so that a long anchor can be read in batches of
 * chromosomes.  gzi_path (may be NULL) says where to start reading; the blocks are walked from there and checked against it.
 * Each contig's rows land at its own place in the (padded) row buffer.  Afterwards pg_result_window_stats works on the rows.
 * Reads the file in pieces of 64 MiB; synchronises. */
int pg_result_inflate_bgzf(pg_result *r, int step, const char *gz_path, const char *gzi_path, uint32_t first_contig,
                           uint32_t ncontigs, uint64_t file_row0);

/* bitsum.bins.tsv as KMCdb::anchor_fasta / write_bits write it (cpp/anchor.cpp:57-69,184-189): the header line
 * "chr\tstart\t0\t1...\tN", then for contig c (numbered from 0) and bin b the line
 * "c\t(b * binlen[c])\tcount_0...\tcount_N"; bins = the contigs' rows back to back, ngenomes + 1 counts each.
 * Host code, no GPU; the text of millions of bins is formatted here rather than row by row in the interpreter. */
int pg_write_bins_tsv(const char *path, uint32_t ngenomes, uint32_t ncontigs, const uint32_t *nbins, const uint32_t *binlen,
                      const uint32_t *bins);

#ifdef __cplusplus
}
#endif
#endif /* PANAGRAM_HIP_H */
