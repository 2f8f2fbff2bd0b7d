// pg_host.h — what the host units of the C-ABI (pg_api.hip, pg_api_*.hip) share: the handle types, the scope guards of
// call-scoped GPU resources, the table's load constants and the helpers one unit calls in another.  Internal to the
// library: every function declared here has hidden visibility, none of it is part of include/panagram_hip.h.
#pragma once
#include "../../include/panagram_hip.h"
#include "pg_kernels.h"
#include "pg_guard.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

using namespace pg;

#define PG_INTERNAL __attribute__((visibility("hidden")))

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(PG_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------
struct pg_ctx {
    int device;
    hipStream_t own_stream;
    hipStream_t stream;
    hipStream_t aux_stream;  // statistics kernels run here, event-ordered behind the probe kernels
    // Handles may be destroyed in any order (a garbage collector frees a dropped object graph in no
    // particular order): an object with live dependants is only marked dead and goes when the last
    // dependant does.
    std::atomic<int> refs{0};
    bool dead = false;
    // staging of the GPU BGZF writer (write_bgzf_gpu): four sets, so that four writer threads can run;
    // allocated at first use, kept — pinning 2 x 64 MiB per file would cost more than the compression
    struct DfSet {
        uint8_t *d_slots[2] = {nullptr, nullptr}, *d_packed[2] = {nullptr, nullptr}, *h_slots[2] = {nullptr, nullptr};
        uint32_t *d_sizes[2] = {nullptr, nullptr}, *d_offs[2] = {nullptr, nullptr}, *h_sizes[2] = {nullptr, nullptr};
        uint32_t *d_crc = nullptr, *d_hist = nullptr;
        void *d_code = nullptr;  // the file's Huffman code and block header (k_df_build_code)
        bool ready = false, busy = false;
    } df[4];
    std::mutex df_mu;
    std::condition_variable df_cv;
    // Row buffers of destroyed results, kept for the next result: hipFree of tens of GB costs about 40 ms per
    // GB on this stack (paid inside the NEXT hipMalloc: tools/malloc_time.py), which a run that anchors its
    // genomes in batches would pay for every batch.  At most two buffers; emptied by pg_ctx_trim, when an
    // allocation fails, and with the context.
    struct RowBuf {
        uint8_t *p;
        uint64_t cap;
    };
    std::vector<RowBuf> row_cache;
    std::mutex row_mu;
};

struct SubHost {
    SubTable d;
    uint64_t count;  // distinct keys
};

struct pg_table {
    pg_ctx *ctx;
    int k, ngenomes, ndbs;
    uint32_t m;  // minimizer length of every sub-table (0 = direct hashing)
    bool m_pinned = false;  // set by pg_table_set_minimizer: re-hashing keeps m
    uint32_t cosched = 0;   // anchor genomes a probe launch will co-schedule (pg_table_set_coscheduled; 0: not told — several)
    uint64_t expected = 0;  // pg_table_create's expected_keys (0: unknown)
    double load0 = 0.375;   // keys per slot the table was created for (TARGET_LOAD; PG_TABLE_KEYS_PER_LINE / pg_table_create_dense: denser)
    uint64_t first_len = 0;  // k-mer positions of the first sequence set inserted into the empty table (settle_minimizer)
    uint64_t max_len = 0;    // ... of the longest one inserted so far (what a re-hash settles m from)
    std::vector<SubHost> subs;
    unsigned long long *d_counters;  // [0] newly claimed, [1] overflow flag
    unsigned long long *h_counters = nullptr;  // pinned landing place of d_counters (read_counters)
    uint32_t *d_tile0 = nullptr;     // first tile of every contig of the seqset being inserted (k_tile0), grown on demand
    size_t tile0_cap = 0;
    double spill = 0;                // keys outside their home line / keys, as of the last pg_table_rehash
    std::atomic<int> refs{0};        // results on this table
    bool dead = false;
    // ONE writer at a time: lane_insert's mask update is a plain read-modify-write that is only safe while every
    // concurrent writer of a word ORs in the same bits (pg_device.h) — i.e. one insert call (one genome, its launches
    // serialised on the context's stream and synchronised before the call returns) at a time.  Every entry point
    // that writes the table holds this lock for its whole duration: a second host thread queues up behind the
    // first instead of racing it, whatever stream the context has been pointed at in between.
    std::mutex write_mu;
};
#define TABLE_WRITER(t) std::lock_guard<std::mutex> writer_guard_((t)->write_mu)

struct pg_seqset {
    pg_ctx *ctx;
    uint32_t n;
    std::vector<SeqDesc> desc;
    uint64_t total_words;
    uint64_t *d_seqw;
    uint32_t *d_nmw;
    uint32_t *d_has_n;
    SeqDesc *d_desc;
    void *d_stage;
    size_t stage_cap;
    std::vector<std::string> names;  // record ids when the seqset was parsed from FASTA text
    std::atomic<int> refs{0};        // results on these sequences
    bool dead = false;
};

struct pg_result {
    pg_ctx *ctx;
    pg_table *tbl;  // NULL for a rows container (pg_result_create_rows): rows arrive through pg_result_merge_columns*
    const pg_seqset *seqs;
    uint32_t N;     // genomes per row (the table's, or the container's own)
    int k;
    uint32_t flags;
    uint32_t lowres_step = 100;  // bitmap.<lowres_step> = every lowres_step-th row (index.py:101-106)
    std::vector<AnchorDesc> ad;
    std::vector<uint64_t> nrows100;
    AnchorDesc *d_ad;
    uint32_t *d_tile_contig;
    uint32_t *d_sched = nullptr;  // optional launch order of the tiles (pg_result_coschedule)
    std::vector<uint32_t> sched_bounds;  // tile indices at which independently scheduled ranges begin / end
    uint32_t ntiles;
    uint8_t *d_out1;
    uint64_t out1_bytes;
    uint64_t out1_cap = 0;  // bytes actually allocated behind d_out1 (it may come out of the context's cache)
    uint8_t *d_out100;
    uint64_t out100_bytes;
    uint32_t *d_bins;
    uint64_t total_bins;
    unsigned long long *d_colsums;
    hipEvent_t ev[4];  // last pg_anchor_run: start / after k_probe (main stream), epilogue start / end (side stream)
    bool ev_ok, ev_epi;
    bool rows_valid = false;  // rows were merged in (pg_result_merge_columns*)
    // HIP-event durations of every pg_anchor_run since the last pg_result_timing_reset: a benchmark
    // averages the launches of all its timed steps, not only the last one
    // (every run records into an event set of its own — ev[] is the latest — so that nothing has to be
    // waited for between steps; sets beyond EV_RING are folded into the sums and recycled)
    struct EvSet {
        hipEvent_t e[4];
        bool probe, epi;  // which of the two intervals (e[0]..e[1] probe, e[2]..e[3] statistics) were recorded
    };
    std::vector<EvSet> ev_hist, ev_free;
    // A whole run goes out as a few CHUNKS of its launch order (slices of the co-schedule), the statistics pass of chunk c
    // on the side stream beside the probe of chunk c+1: the pass reads rows at HBM speed while the probe is busy
    // issuing instructions (run_chunks).  A chunk: schedule slice [s0, s1) and the tile ranges it touches.
    struct Chunk {
        uint32_t s0, s1, r0, nr, tiles;
    };
    std::vector<Chunk> chunks;
    uint2 *d_ranges = nullptr;
    bool chunks_ready = false;
    std::vector<hipEvent_t> chunk_ev;
    size_t hist_skip = 0;  // leading sets of ev_hist from before the last pg_result_timing_reset
    double probe_ms_sum = 0, epi_ms_sum = 0;
    uint32_t probe_runs = 0, epi_runs = 0;
    // Fused statistics (round 6, pg_kernels.h: FuseArgs): k_probe leaves per-tile counters, k_tile_reduce adds them up; the
    // statistics pass then only runs over the tiles of contigs whose bins are shorter than a tile (d_small: their ranges).
    int fuse_state = 0;  // 0: not decided yet, 1: this result's whole runs are fused, -1: they are not (row width, layout, memory)
    uint32_t *d_tile_hist = nullptr, *d_tile_cs = nullptr;
    uint2 *d_small = nullptr;
    uint32_t n_small = 0, small_tiles = 0;
    SelSeg *d_sel = nullptr, *h_sel = nullptr;  // the sel_n segments of the last pg_result_select_columns_range into this result, and their page-locked copy
    size_t sel_cap = 0, sel_n = 0;
    uint32_t fused_runs = 0;  // whole runs that took the fused path (pg_result_fused_runs: tests and bench.py say which path was timed)
};
static constexpr size_t EV_RING = 128;

// Scratch: what lives for one call of one entry point belongs to a scope and goes on every way out of it, an
// exception's included (the firewall of pg_guard.h turns that into an error code; nothing may leak behind it).  What
// outlives the call belongs to a handle above and is freed by its *_free / *_destroy.  A stream is declared AFTER the
// buffers and events it uses: it goes first, and drains before they do.
template <class T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    ~DevBuf() {
        if (p) hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)); }
    hipError_t upload(const std::vector<T> &h, hipStream_t st) {  // alloc, then the host vector's copy enqueued
        const hipError_t e = alloc(h.size());
        return e != hipSuccess ? e : hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    }
    T *get() const { return p; }
};
template <class T>
struct PinBuf {
    T *p = nullptr;
    PinBuf() = default;
    PinBuf(PinBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    ~PinBuf() {
        if (p) hipHostFree(p);
    }
    hipError_t alloc(size_t count, unsigned flags) { return hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), flags); }
    T *get() const { return p; }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream() {
        if (!s) return;
        hipStreamSynchronize(s);
        hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipStream_t get() const { return s; }
};
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~Event() {
        if (ev) hipEventDestroy(ev);
    }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&ev, flags); }
    hipEvent_t get() const { return ev; }
};

// the HIP-event time of one launch, for the *_last_timing calls: armed only where the caller hands in a place for it
struct LaunchTimer {
    float *ms;
    Event a, b;
    explicit LaunchTimer(float *out) : ms(out) {}
    hipError_t start(hipStream_t st) {
        if (!ms) return hipSuccess;
        hipError_t e = a.create(hipEventDefault);
        if (e == hipSuccess) e = b.create(hipEventDefault);
        return e == hipSuccess ? hipEventRecord(a.get(), st) : e;
    }
    hipError_t stop(hipStream_t st) { return ms ? hipEventRecord(b.get(), st) : hipSuccess; }
    void read() {  // (behind the stream's synchronise)
        if (ms && hipEventElapsedTime(ms, a.get(), b.get()) != hipSuccess) *ms = -1.0f;
    }
};

static constexpr uint32_t MAX_PROBE = 512;  // lines an insert may walk before the table is grown
static constexpr double GROW_AT = 0.55;     // grow when keys > GROW_AT * slots
#ifndef PG_INLINE_LAYOUT
#define PG_INLINE_LAYOUT 1
#endif
static constexpr double TARGET_LOAD = 0.375; // load right after growing (3 keys per 8-slot line)
static constexpr double HARD_LOAD = 0.85;   // worst-case guard before a batch

// The windows of one window query (pg_result_bin_colsums, _pair_counts, _find_runs, _pattern_counts), as gather_windows
// leaves them: per window the device byte offset of its contig's rows and [start, end) in sampled rows.
struct Windows {
    uint32_t n = 0;
    uint64_t longest = 0;      // sampled rows of the longest window
    std::vector<uint64_t> se;  // [3 n]: the offsets, the starts, the ends
    DevBuf<uint64_t> d_se;
    hipError_t upload(hipStream_t st) { return d_se.upload(se, st); }
    const uint64_t *base() const { return d_se.get(); }
    const uint64_t *starts() const { return d_se.get() + n; }
    const uint64_t *ends() const { return d_se.get() + 2 * (size_t)n; }
};

// Helpers that cross a unit: defined once, in the unit named, and hidden from the dynamic symbol table.
namespace pg {
// pg_api.hip
extern PG_INTERNAL thread_local std::string g_err;  // the one error slot (pg_last_error)
PG_INTERNAL int fail(int code, const char *fmt, ...);
PG_INTERNAL int use_device(const pg_ctx *c);
PG_INTERNAL int check_step(const pg_result *r, int step);
PG_INTERNAL void ctx_release(pg_ctx *c);
PG_INTERNAL void table_release(pg_table *t);  // a dependant of the table (a result, a screen) lets go of it
PG_INTERNAL hipError_t row_alloc(pg_ctx *c, uint64_t bytes, uint8_t **out, uint64_t *cap);
PG_INTERNAL void row_free(pg_ctx *c, uint8_t *p, uint64_t cap);
PG_INTERNAL uint32_t window_cap(int ngenomes = 0);  // (PG_TABLE_WMAX)
PG_INTERNAL int read_counters(pg_table *t, unsigned long long out[2]);
PG_INTERNAL int ensure_room(pg_table *t, int si, uint64_t incoming);
PG_INTERNAL int grow_after_overflow(pg_table *t, int si, uint64_t incoming);
PG_INTERNAL int after_insert(pg_table *t, int si);
PG_INTERNAL int join_result(pg_result *r);
PG_INTERNAL int next_events(pg_result *r, bool probe);
// pg_api_seqset.hip
PG_INTERNAL void seqset_release(pg_seqset *s);
// pg_api_query.hip: what the window queries share (a call's own checks come between check_window_call and gather_windows)
PG_INTERNAL int check_window_call(const pg_result *r, int step, uint32_t stride, uint32_t n, const char *fn, const char *nouns);
PG_INTERNAL int gather_windows(const pg_result *r, int step, uint32_t stride, uint32_t n, const uint32_t *contig, const uint64_t *starts,
                               const uint64_t *ends, const char *noun, Windows &w);
PG_INTERNAL uint32_t valid_word(uint32_t N, uint32_t d);
PG_INTERNAL std::vector<uint32_t> mask_words(uint32_t N, const uint32_t *words, uint32_t if_null);
PG_INTERNAL uint32_t pieces_for(uint64_t longest, uint32_t nwin, uint32_t cap);
PG_INTERNAL int cut_chunks(const char *fn, uint32_t nwin, const uint64_t *starts, const uint64_t *ends, uint32_t chunk_rows,
                           std::vector<uint2> &chunks, std::vector<uint64_t> *first = nullptr);
// pg_api_bgzf.hip
PG_INTERNAL void df_free_buffers(pg_ctx::DfSet &d);
// pg_api_copies.hip: this thread's last pg_seqset_from_fastq (its kernels) and pg_copytable_sample_agree, in milliseconds (a
// function, not an extern thread_local: another unit would call the variable's absent initialiser)
PG_INTERNAL float *place_ms();
}  // namespace pg
