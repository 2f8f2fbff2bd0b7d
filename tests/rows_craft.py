"""Crafted bitmap rows for the kernels that read finished rows and reduce them (k_epilogue*, k_lowres, k_window_stats,
k_bin_colsums): rows planted straight into a rows container — no index build, no hash table — in the patterns the synthetic
genomes never produce (every column set at once, every row of a tile in one histogram slot, rows of all N bits, bits past
N), and plain numpy restatements of what the kernels' header comments say they compute.  No tests in here:
tests/test_rows_craft_cpu.py ties the restatements to the ones the suite already trusts (oracle.pyoracle.window_stats,
tests/intros_ref.bitmap_to_bins), tests/test_gpu_rows_craft.py holds the kernels to them.

Bit g of a row is bit g % 8 of its byte g // 8; a row of N genomes has (N + 7) // 8 bytes."""
import numpy as np


def row_bytes(n):
    return (n + 7) // 8


# ---------------------------------------------------------------------------
# pattern generators: (nk, nbytes) uint8, no bit at or past N (with_pad_bits apart)
# ---------------------------------------------------------------------------
def pack(bits):
    """(nk, N) 0/1 -> (nk, nbytes) uint8"""
    bits = np.asarray(bits, np.uint8)
    if bits.shape[0] == 0:
        return np.zeros((0, row_bytes(bits.shape[1])), np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


def unpack(rows, n):
    """(nk, nbytes) uint8 -> (nk, N) 0/1: the first N bits only"""
    return np.unpackbits(np.asarray(rows, np.uint8), axis=1, bitorder="little")[:, :n]


def ones(nk, n):
    return pack(np.ones((nk, n), np.uint8))


def zeros(nk, n):
    return np.zeros((nk, row_bytes(n)), np.uint8)


def column(nk, n, g):
    bits = np.zeros((nk, n), np.uint8)
    bits[:, g] = 1
    return pack(bits)


def ramp(nk, n):
    """row i: its lowest i mod (N + 1) bits — every histogram slot 0..N"""
    return pack(np.arange(n)[None, :] < (np.arange(nk) % (n + 1))[:, None])


def checker(nk, n):
    """0xAA on even rows, 0x55 on odd ones, cut to N bits"""
    rows = np.where((np.arange(nk) % 2 == 0)[:, None], 0xAA, 0x55).astype(np.uint8).repeat(row_bytes(n), axis=1)
    if n % 8:
        rows[:, -1] &= (1 << (n % 8)) - 1
    return rows


def bursts(nk, n, length):
    """`length` rows of ones, one row of zeros, and again"""
    on = (np.arange(nk) % (length + 1)) != length
    return pack(np.repeat(on[:, None], n, axis=1))


def dense(nk, n, seed):
    return pack(np.random.default_rng(seed).random((nk, n)) < 0.5)


def with_pad_bits(rows, n):
    """the same rows with the bits past N in their last byte set"""
    out = np.array(rows, np.uint8, copy=True)
    if n % 8:
        out[:, -1] |= (0xFF << (n % 8)) & 0xFF
    return out


def back_to_back(nk, parts):
    """`parts` = [(share, generator(nk_part))]: segments one after the other, the last one taking what is left of nk"""
    total = sum(s for s, _ in parts)
    out, used = [], 0
    for i, (share, gen) in enumerate(parts):
        m = nk - used if i == len(parts) - 1 else nk * share // total
        out.append(gen(m))
        used += m
    return np.concatenate(out)


# ---------------------------------------------------------------------------
# containers
# ---------------------------------------------------------------------------
def container(ctx, k, n, nkmers_list, **geometry):
    """a rows container of N-genome rows over contigs of the given numbers of k-mers (a SeqSet of its own, closed with it);
    geometry: colsums, lowres_step, max_bin_len, min_bin_count"""
    from panagram_amd import engine
    ss = engine.SeqSet(ctx, [int(nk) + k - 1 for nk in nkmers_list])
    try:
        res = engine.AnchorResult.rows_container(ctx, k, n, ss, **geometry)
    except Exception:
        ss.close()
        raise
    res._own_seqs = ss
    return res


def contig_offsets(nkmers_list, nbytes):
    """byte offset of each contig's rows in the row buffer, and the buffer's size: contig c starts where the earlier
    contigs' nkmers * nbytes, each rounded up to 16, end (pg_api.hip, result_create)"""
    offs, at = [], 0
    for nk in nkmers_list:
        offs.append(at)
        at += (int(nk) * nbytes + 15) & ~15
    return offs, at


SLACK = 16  # bytes every row buffer carries behind max(16, size) (pg_api.hip, result_create: k_epilogue_chunks' last load)


def plant(res, rows_per_contig, poison=None):
    """write each contig's (nk, nbytes) rows at its offset.  poison = b: every byte of the buffer that is not a row byte —
    the padding between contigs and the slack behind the last row — holds b."""
    import torch
    nb = res.nbytes
    (ptr, size), _ = res.device_ptrs()
    nks = [len(r) for r in rows_per_contig]
    assert len(nks) == len(res.seqs.lens)
    offs, total = contig_offsets(nks, nb)
    assert total == size, (total, size)
    assert not nks or offs[-1] + nks[-1] * nb <= size  # the last row fits
    cap = max(16, size) + SLACK

    class _Wrap:
        __cuda_array_interface__ = {"shape": (cap,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    buf = torch.as_tensor(_Wrap(), device=torch.device("cuda", res.ctx.device))
    if poison is not None:
        buf.fill_(int(poison))
    for off, r in zip(offs, rows_per_contig):
        r = np.ascontiguousarray(r, np.uint8)
        assert r.ndim == 2 and r.shape[1] == nb
        if r.size:
            buf[off:off + r.size].copy_(torch.from_numpy(r.reshape(-1)))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def bin_length(nk, max_bin_len=200000, min_bin_count=100):
    """rows per bin of a contig (include/panagram_hip.h: 200000, or nkmers / 100 for a contig with fewer than 100 such
    bins; a contig shorter than min_bin_count gets one bin per row)"""
    binlen = max_bin_len
    if nk // binlen < min_bin_count:
        binlen = nk // min_bin_count
    return max(1, binlen)


def ref_stats(rows, n, binlen, step):
    """(bins [ceil(nk / binlen), N + 1], column sums [N], low-resolution rows) of one contig's rows: bin b is the
    histogram of the popcounts of rows [b binlen, (b + 1) binlen)"""
    bits = unpack(rows, n)
    popc = bits.sum(axis=1, dtype=np.int64)
    nbins = (len(rows) + binlen - 1) // binlen
    bins = np.zeros((nbins, n + 1), np.int64)
    for b in range(nbins):
        bins[b] = np.bincount(popc[b * binlen:(b + 1) * binlen], minlength=n + 1)
    return bins, bits.sum(axis=0, dtype=np.int64), rows[::step]


def keep_bits(n, keep_words):
    """32-bit keep words (bit g of the mask = bit g % 32 of word g // 32) -> (N,) 0/1"""
    kb = np.zeros(n, np.uint8)
    if keep_words is not None:
        for d, w in enumerate(np.asarray(keep_words, np.uint32).ravel()):
            for b in range(32):
                if 32 * d + b < n and (int(w) >> b) & 1:
                    kb[32 * d + b] = 1
    return kb


def words_of(n, cols):
    """keep words with the given columns set"""
    w = np.zeros((n + 31) // 32, np.uint32)
    for g in cols:
        w[g // 32] |= np.uint32(1 << (g % 32))
    return w


def _transformed(rows, n, stride, keep_words):
    """sampled rows (row j * stride) as bits with the keep rule applied, and which of them had a keep bit"""
    bits = unpack(rows[::stride], n)                    # 1. the first N bits
    kb = keep_bits(n, keep_words)
    has_keep = (bits & kb).any(axis=1)
    bits = bits | (kb[None, :] & ~has_keep[:, None])    # 2. no keep bit: the keep bits are ORed in
    return bits, has_keep


def ref_bin_colsums(rows, n, starts, ends, stride, keep_words, omit_fixed):
    """(cs [nbins, N], kept [nbins]) of bins [starts[i], ends[i]) in sampled rows of ONE contig's rows, by the rule in
    pg_bins.hip's header"""
    bits, _ = _transformed(rows, n, stride, keep_words)
    take = ~bits.all(axis=1) if omit_fixed else np.ones(len(bits), bool)  # 3. rows of all N bits are dropped
    cs = np.zeros((len(starts), n), np.int64)
    kept = np.zeros(len(starts), np.int64)
    for i, (s, e) in enumerate(zip(starts, ends)):
        s, e = int(s), int(e)
        t = take[s:e]
        cs[i] = bits[s:e][t].sum(axis=0, dtype=np.int64)                  # 4. column sums and number of the rows left
        kept[i] = t.sum()
    return cs, kept


def classes(rows, n, keep_words, starts=None, ends=None, stride=1):
    """[[no keep bit & not full, no keep bit & full], [keep bit & not full, keep bit & full]] — rows in each class, "full"
    after the keep rule; with starts / ends one such 2 x 2 table per bin of sampled rows"""
    bits, has_keep = _transformed(rows, n, stride, keep_words)
    cls = 2 * has_keep.astype(np.int64) + bits.all(axis=1)
    if starts is None:
        return np.bincount(cls, minlength=4).reshape(2, 2)
    return np.stack([np.bincount(cls[int(s):int(e)], minlength=4).reshape(2, 2) for s, e in zip(starts, ends)]) \
        if len(starts) else np.zeros((0, 2, 2), np.int64)


# ---------------------------------------------------------------------------
# the planted cases, shared by the CPU test that checks their coverage and the GPU tests that run them
# ---------------------------------------------------------------------------
# row widths 1..16, 17, 32, 38, 50, 64 and 65 bytes.  (65 bytes: five lanes per row in k_epilogue_chunks, 21 rows per lane and tile — the
# width at which a workgroup's 16 to 20 tiles of ones bring a lane far past the 255 rows its planes hold; at 38 bytes they
# bring it 260, at 17 bytes 160.)
# 256, 400 and 512: the instantiations k_epilogue_chunks<2, true>, <4, false> and <4, true> (EXACT: aligned loads, no tail mask,
# the `full` shortcut).
# The flush of the column sums' counter planes in the MIDDLE of a contig — after 240 rows of a thread, 248 or 252 in k_epilogue_w
# — is NOT reached by these cases for rows of 2..16 bytes (k_epilogue_n, k_epilogue_w), nor for 17..32 bytes: the launcher gives a
# workgroup 16 to 20 tiles (64 rows per thread) until a launch holds more than 16 384 tiles, and the flush takes 60 tiles of one
# contig in one workgroup (30 at 17..32 bytes).  It is covered by the flush cases below (FLUSH_*): the same kernels under
# PG_EPI_WORKGROUPS = 1 and 2, launch_rows_epilogue's bound on the grid, over a contig of 131 tiles — tests/
# test_gpu_planes_flush.py; tests/epi_walk.py restates which thread meets which flush, and tests/test_rows_craft_cpu.py holds
# the cases to that model, the absence of any such flush without the bound included.  (tools/planes_check.cpp checks the planes'
# integer arithmetic alone, on the host.)
STATS_N = [1, 8, 13, 24, 29, 40, 45, 56, 61, 72, 77, 88, 93, 104, 109, 120, 128, 130, 256, 300, 400, 512, 520]
STATS_NK = [1, 99, 100, 101, 255, 256, 257, 1023, 1024, 1025, 8 * 1024 + 1, 20000, 70001]
STATS_GEOMETRY = {
    "default": {},
    "long_bins": dict(max_bin_len=5000, min_bin_count=1),  # bins longer than a tile of 1024 rows
    "nocs_low7": dict(colsums=False, lowres_step=7),
}


def stats_rows(n):
    """one contig per STATS_NK: every pattern on a short contig, whole tiles of ones / zeros (every row in ONE histogram
    slot, every column counted at every row), and on the two long contigs ones, ramp, bursts of 255 / 256 / 257 and dense
    rows back to back"""
    def long(nk, seed, nones):
        # (the ones first and many tiles long: a workgroup of the statistics pass takes 16 to 20 consecutive tiles of so small
        # an input, and its carry-save planes reach their ceiling only where all of them are rows of ones)
        rest = back_to_back(nk - nones, [(1, lambda m: ramp(m, n)), (1, lambda m: bursts(m, n, 255)),
                                         (1, lambda m: bursts(m, n, 256)), (1, lambda m: bursts(m, n, 257)),
                                         (1, lambda m: dense(m, n, seed))])
        return np.concatenate([ones(nones, n), rest])
    rows = [ones(1, n), zeros(99, n), column(100, n, n - 1), ramp(101, n), checker(255, n), bursts(256, n, 3),
            dense(257, n, 1), ones(1023, n), ones(1024, n), zeros(1025, n),
            back_to_back(8 * 1024 + 1, [(1, lambda m: ones(m, n)), (1, lambda m: column(m, n, 0))]),
            long(20000, 2, 6000), long(70001, 3, 36000)]
    assert [len(r) for r in rows] == STATS_NK
    return rows


# The flush of the counter planes in the MIDDLE of a contig (tests/test_gpu_planes_flush.py; which thread meets which flush:
# tests/epi_walk.py).  Every row width of 2..16 bytes, 17 and 32 bytes (k_epilogue_chunks<2, false> and <2, true>, 8 rows per
# lane and tile) and one byte (accumulators of its own: it must equal the reference all the same).
FLUSH_N = [8, 13, 24, 29, 40, 45, 56, 61, 72, 77, 88, 93, 104, 109, 120, 128, 130, 256]
FLUSH_BOUNDS = [1, 2]  # PG_EPI_WORKGROUPS: one workgroup walks every contig; a second one starts inside the long contig
# a contig of exactly the 60 tiles of one flush and a partial tile; the long one, 131 tiles and a partial one (two flushes and rows
# behind them); a short one behind it (its end-of-contig flush follows a mid-contig one and starts from clean planes).  In this
# order a second workgroup starts at tile 35 of the long contig and has 97 of its tiles.
FLUSH_NK = [60 * 1024 + 77, 131 * 1024 + 300, 2500]
FLUSH_ONES_TILES = 64  # of the long contig: all N bits, so that every column of every thread stands at the count at which the first flush comes


def flush_rows(n):
    long_nk = FLUSH_NK[1] - FLUSH_ONES_TILES * 1024
    long_rest = back_to_back(long_nk, [(1, lambda m: ramp(m, n)), (1, lambda m: bursts(m, n, 255)), (1, lambda m: bursts(m, n, 256)),
                                       (1, lambda m: bursts(m, n, 257)), (1, lambda m: column(m, n, n - 1)),
                                       (1, lambda m: dense(m, n, 11))])
    rows = [np.concatenate([ones(60 * 1024, n), dense(77, n, 10)]),
            np.concatenate([ones(FLUSH_ONES_TILES * 1024, n), long_rest]),
            back_to_back(FLUSH_NK[2], [(1, lambda m: ramp(m, n)), (1, lambda m: ones(m, n)), (1, lambda m: dense(m, n, 12))])]
    assert [len(r) for r in rows] == FLUSH_NK
    return rows


def flush_geometries(n):
    """{name: geometry} of the flush cases of N: the default bins (nkmers / 100 rows), bins longer than a tile, and what the walk
    needs to reach the sites those two do not — k_epilogue_n's one-tile site (bins the window holds, groups of 4 tiles refused)
    and k_epilogue_w's flush at 252 rows (groups and single tiles in turn), both found by the model of the walk"""
    from tests import epi_walk as ew
    geoms = {"default": {}, "long_bins": dict(max_bin_len=5000, min_bin_count=1)}
    if ew.kernel_of(n) == "n":
        geoms["one_tile"] = ew.one_tile_bins(n, FLUSH_NK)
    elif ew.kernel_of(n) == "w":
        # (uniform bins mix groups and single tiles at ONE bin length per N, about 2048 / MAXB rows; at N = 77 — 53 rows — the
        # single tiles come in pairs under both bounds and every flush stays at 248: no such case for rows of 10 bytes)
        geom = ew.carry_bins(n, FLUSH_NK)
        if geom is not None:
            geoms["carry252"] = geom
    return geoms


def flush_cases():
    """(N, geometry name) of every flush case (a geometry the model of the walk does not find — None — is no case: tests/
    test_rows_craft_cpu.py fails then)"""
    return [(n, name) for n in FLUSH_N for name, geom in flush_geometries(n).items() if geom is not None]


WINDOW_N =[1, 8, 33, 64, 128, 130, 300]
WINDOW_NK = [200000, 300]


def window_rows(n):
    big = back_to_back(WINDOW_NK[0], [(1, lambda m: ones(m, n)), (1, lambda m: ramp(m, n)), (1, lambda m: dense(m, n, 4)),
                                      (1, lambda m: column(m, n, n - 1))])
    return [big, back_to_back(WINDOW_NK[1], [(1, lambda m: dense(m, n, 5)), (1, lambda m: ones(m, n))])]


def windows(nk):
    """(starts, ends): empty, one row, around multiples of 256, past the contig's end, the whole contig"""
    w = [(0, 0), (5, 5), (7, 8), (nk - 1, nk), (0, 1), (255, 257), (256, 512), (257, 511), (1, 256), (255, 1025),
         (511, 769), (nk - 10, nk + 500), (nk, nk + 7), (nk + 1000, nk + 2000), (0, nk), (1, nk - 1), (0, nk + 12345)]
    w = [(max(0, s), e) for s, e in w]
    return np.array([s for s, _ in w], np.uint64), np.array([e for _, e in w], np.uint64)


BINS_N = [3, 8, 9, 32, 33, 64, 65, 128, 129, 130, 256, 300]
BINS_NK = [201000, 1000, 1]
BINS_STRIDES = [1, 7, 100]
BINS_MIN_ROWS = 64  # bins of at least this many sampled rows hold every class of row (test_rows_craft_cpu.py)


def keep_cases(n):
    """{name: columns or None}: no mask, one column that is not always set, one column in every 32-bit word, the last
    column alone"""
    every = sorted({min(32 * d + 5, n - 1) for d in range((n + 31) // 32)})
    return {"none": None, "one": [n // 2], "every_word": every, "last": [n - 1]}


def bins_rows(n):
    """rows whose kind goes by i mod 9 (9 shares no factor with the strides 1, 7, 100, so every run of nine sampled rows
    holds every kind at every stride): 0 all N bits; 1..3 all but the columns of one keep mask; 4 all but the columns of
    every keep mask; 5..8 dense.  For every keep mask this gives rows with and without a keep bit that do and do not end
    up with all N bits."""
    masks = [c for c in keep_cases(n).values() if c is not None]
    out = []
    for c, nk in enumerate(BINS_NK):
        bits = unpack(dense(nk, n, 20 + c), n).copy()
        kind = np.arange(nk) % 9
        bits[kind <= 4] = 1
        for j, cols in enumerate(masks):
            bits[np.ix_(kind == j + 1, cols)] = 0
        bits[np.ix_(kind == 4, sorted({g for cols in masks for g in cols}))] = 0
        out.append(pack(bits))
    return out


def bins_cases(stride):
    """(contigs, starts, ends) in sampled rows: a bin the launch cuts into many pieces (200 000 sampled rows at stride 1),
    starts that are no multiples of 256, one-row bins (a row of all N bits among them), empty bins, bins of three contigs"""
    ns = [(nk - 1) // stride + 1 for nk in BINS_NK]
    big_end = min(200003, ns[0])
    first_full = next(j for j in range(ns[0]) if (j * stride) % 9 == 0 and j > 0)  # (kind 0: all N bits)
    bins = [(0, 3, big_end), (0, 5, 5), (0, ns[0] - 1, ns[0]), (0, first_full, first_full + 1), (0, 1, min(300, ns[0])),
            (0, min(257, ns[0] - 1), min(777, ns[0])), (0, 100, 101), (0, 0, ns[0]), (1, 0, ns[1]), (1, ns[1], ns[1]),
            (1, ns[1] // 3, 2 * (ns[1] // 3) + 1), (2, 0, 1), (2, 0, 0), (0, min(1000, ns[0] - 1), min(1256, ns[0]))]
    c, s, e = (np.array(x) for x in zip(*bins))
    return c.astype(np.uint32), s.astype(np.uint64), e.astype(np.uint64)
