// blocks_stitch_check.cpp — the host half of the synteny blocks (panagram_amd/csrc/pg_blocks_host.h: blocks_stitch) held to a loop
// over the whole run list, as a stand-alone program for the host sanitizers: no GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o blocks_stitch_check tools/blocks_stitch_check.cpp
//   ./blocks_stitch_check      (prints "ok" and the cases it ran; any mismatch or sanitizer report ends it with a non-zero status)
// Random run lists over several contigs of A — stretches that link, substitutions, shifted links, strand flips, jumps, stray
// short runs — are cut into chunks of a few runs: chunks whose runs are all dropped, all kept, chunks of one run.  What
// k_run_blocks' count pass leaves per chunk (the first kept run undecided) is computed by a loop; blocks_stitch's offsets then
// drive a loop that writes what the emit pass writes, chunk by chunk in any order, and the blocks that come out — end record less
// start record — must equal those of one loop over the whole list.
#include "../panagram_amd/csrc/pg_blocks_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

using namespace pg;

struct Run {
    uint32_t s, e, m;
};
struct Block {
    uint32_t contig, start, end, mate_first, mate_last, kmers, runs, shifted;
    bool operator==(const Block &o) const {
        return contig == o.contig && start == o.start && end == o.end && mate_first == o.mate_first && mate_last == o.mate_last &&
               kmers == o.kmers && runs == o.runs && shifted == o.shifted;
    }
};
struct Params {
    uint32_t min_run, max_gap, max_shift;
    std::vector<uint64_t> boff;
};

static bool linked(const Params &p, uint32_t e, uint32_t ml, const Run &r, bool *sh) {
    return blocks_link(e, ml, r.s, r.m, p.max_gap, p.max_shift, p.boff.data(), (uint32_t)p.boff.size(), sh);
}

// the blocks of one contig by a loop over all its runs
static void whole(const Params &p, uint32_t contig, const std::vector<Run> &runs, std::vector<Block> &out) {
    uint32_t e = 0, ml = BLOCKS_NONE;
    for (const Run &r : runs) {
        const uint32_t n = r.e - r.s;
        if (n < p.min_run) continue;
        bool sh = false;
        if (linked(p, e, ml, r, &sh)) {
            Block &b = out.back();
            b.end = r.e, b.mate_last = blocks_last_mate(r.m, n), b.kmers += n, b.runs += 1, b.shifted += sh;
        } else {
            out.push_back(Block{contig, r.s, r.e, r.m, blocks_last_mate(r.m, n), n, 1, 0});
        }
        e = r.e, ml = blocks_last_mate(r.m, n);
    }
}

// one chunk as the kernel walks it.  offs == nullptr: the count pass; otherwise the emit pass into the 10 planes of `out`
static BlockChunkCount chunk_pass(const Params &p, const Run *runs, size_t n, bool last_of_contig, const BlockChunkOffs *offs, uint64_t total,
                                  std::vector<uint32_t> &out) {
    BlockChunkCount c{0, 0, 0, 0, 0, 0, 0, BLOCKS_NONE};
    uint32_t e = offs ? offs->carry_e : 0, ml = offs ? offs->carry_ml : BLOCKS_NONE;
    uint32_t kmers = offs ? offs->kmers : 0, kept = offs ? offs->runs : 0, shifted = offs ? offs->shifted : 0;
    uint64_t sat = offs ? offs->soff : 0, eat = offs ? offs->eoff : 0;
    bool have_first = false;
    auto end_record = [&]() {
        if (eat >= total) std::abort();  // (an offset past the blocks: the stitch counted wrong)
        out[5 * total + eat] = e, out[6 * total + eat] = ml, out[7 * total + eat] = kmers, out[8 * total + eat] = kept, out[9 * total + eat] = shifted;
        ++eat;
    };
    for (size_t i = 0; i < n; ++i) {
        const Run &r = runs[i];
        const uint32_t len = r.e - r.s;
        if (len < p.min_run) continue;
        if (!have_first) c.first_s = r.s, c.first_m = r.m, have_first = true;
        bool sh = false;
        const bool pred = ml != BLOCKS_NONE, lk = linked(p, e, ml, r, &sh);
        if (!lk && (offs || pred)) {
            c.starts += 1;
            if (offs) {
                if (pred) end_record();
                if (sat >= total) std::abort();
                out[sat] = r.s, out[total + sat] = r.m, out[2 * total + sat] = kmers, out[3 * total + sat] = kept, out[4 * total + sat] = shifted;
                ++sat;
            }
        }
        if (lk && sh) shifted += 1, c.shifted += 1;
        kmers += len, c.kmers += len;
        kept += 1, c.kept += 1;
        e = r.e, ml = blocks_last_mate(r.m, len);
    }
    if (offs && last_of_contig && ml != BLOCKS_NONE) end_record();
    c.last_e = e, c.last_ml = ml;
    return c;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    std::mt19937_64 rng(11);
    uint64_t cases = 0, across = 0, all_dropped = 0, all_kept = 0, one_run = 0;
    for (uint32_t round = 0; round < 400; ++round) {
        Params p;
        p.min_run = 1 + rng() % 4;
        p.max_gap = 1 + rng() % 60;
        p.max_shift = rng() % 12;
        p.boff = {0, 5000 + rng() % 5000, 20000, 20000, 1u << 20};  // (an empty contig of B among them)
        const uint32_t ncontigs = 1 + rng() % 5, chunk = 1 + rng() % 9;
        std::vector<std::vector<Run>> contigs(ncontigs);
        for (auto &runs : contigs) {
            const uint32_t nruns = rng() % 4 == 0 ? rng() % 3 : rng() % 120;
            uint32_t s = rng() % 10, b = 100 + rng() % 9000, strand = rng() & 1;
            uint32_t kind = 0;  // of the chunk being filled: 0 mixed, 1 all dropped, 2 all kept
            for (uint32_t i = 0; i < nruns; ++i) {
                if (i % chunk == 0) kind = rng() % 3;
                uint32_t n = kind == 1 ? 1 + rng() % (p.min_run - 1 ? p.min_run - 1 : 1) : kind == 2 ? p.min_run + rng() % 5 : 1 + rng() % 6;
                if (kind == 1 && p.min_run == 1) n = 1;  // (nothing can be dropped)
                const uint32_t what = rng() % 10;
                uint32_t dA = 1 + rng() % 8, dB = dA;
                if (what == 0) dB = dA + rng() % 14;             // an insertion in B
                if (what == 1) dA = dB + rng() % 14;             // a deletion from B
                if (what == 2) strand ^= 1;                      // a flip
                if (what == 3) b = 100 + rng() % 19000, dB = 0;  // a jump
                if (what == 4) dA = dB = p.max_gap + rng() % 2;  // at the bound and one past it
                s += dA - 1;
                if (strand == 0) b += dB;
                else b = b > dB + n + 50 ? b - dB : 15000 + rng() % 1000;
                runs.push_back(Run{s, s + n, (b << 1) | strand});
                s += n;
                b = strand ? b - (n - 1) : b + (n - 1);
            }
        }
        // the chunks, the count pass and the stitch
        std::vector<uint64_t> first(ncontigs + 1, 0), nblocks(ncontigs, ~0ull);
        std::vector<BlockChunkCount> counts;
        std::vector<uint32_t> none;
        struct Piece {
            uint32_t contig;
            size_t at, n;
            bool last;
        };
        std::vector<Piece> pieces;
        for (uint32_t c = 0; c < ncontigs; ++c) {
            first[c] = counts.size();
            for (size_t at = 0; at < contigs[c].size(); at += chunk) {
                const size_t n = std::min<size_t>(chunk, contigs[c].size() - at);
                pieces.push_back(Piece{c, at, n, at + n == contigs[c].size()});
                counts.push_back(chunk_pass(p, contigs[c].data() + at, n, pieces.back().last, nullptr, 0, none));
                all_dropped += counts.back().kept == 0;
                all_kept += counts.back().kept == n;
                one_run += n == 1;
            }
        }
        first[ncontigs] = counts.size();
        std::vector<BlockChunkOffs> offs(counts.size());
        const uint64_t total = blocks_stitch(ncontigs, first.data(), counts.data(), p.max_gap, p.max_shift, p.boff.data(),
                                             (uint32_t)p.boff.size(), offs.data(), nblocks.data());
        CHECK(total != ~0ull);
        // the emit pass, the chunks in any order
        std::vector<uint32_t> out(10 * total, 0xDEADBEEFu);
        std::vector<size_t> order(pieces.size());
        std::iota(order.begin(), order.end(), 0);
        std::shuffle(order.begin(), order.end(), rng);
        for (size_t i : order) chunk_pass(p, contigs[pieces[i].contig].data() + pieces[i].at, pieces[i].n, pieces[i].last, &offs[i], total, out);
        std::vector<Block> want;
        std::vector<uint64_t> want_n(ncontigs, 0);
        for (uint32_t c = 0; c < ncontigs; ++c) {
            const size_t before = want.size();
            whole(p, c, contigs[c], want);
            want_n[c] = want.size() - before;
        }
        CHECK(total == want.size());
        CHECK(nblocks == want_n);
        uint64_t at = 0;
        for (uint32_t c = 0; c < ncontigs; ++c)
            for (uint64_t i = 0; i < nblocks[c]; ++i, ++at) {
                const Block got{c, out[at], out[5 * total + at], out[total + at], out[6 * total + at], out[7 * total + at] - out[2 * total + at],
                                out[8 * total + at] - out[3 * total + at], out[9 * total + at] - out[4 * total + at]};
                CHECK(got == want[at]);
                across += got.runs > chunk;
            }
        ++cases;
    }
    std::printf("ok: %llu cases, %llu blocks longer than a chunk; chunks all dropped %llu, all kept %llu, of one run %llu\n",
                (unsigned long long)cases, (unsigned long long)across, (unsigned long long)all_dropped, (unsigned long long)all_kept,
                (unsigned long long)one_run);
    return across > 200 && all_dropped > 200 && all_kept > 200 && one_run > 200 ? 0 : 1;
}
