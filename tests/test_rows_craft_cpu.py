"""CPU: the crafted-rows helper (tests/rows_craft.py) — its references against the restatements the suite already trusts
(oracle.pyoracle.window_stats, tests/intros_ref.bitmap_to_bins), its pattern generators, and the coverage the GPU tests
(tests/test_gpu_rows_craft.py) claim for the rows they plant; and the model of the statistics kernels' walk (tests/epi_walk.py):
which mid-contig flush of the column sums' counter planes the cases of tests/test_gpu_planes_flush.py reach under the bound on the
grid, and that the default launch shape reaches none."""
import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd.index import Genome
from tests import epi_walk as ew
from tests import intros_ref as ref
from tests import rows_craft as rc

SMALL_N = [1, 3, 8, 9, 13, 40, 65, 130]


def _patterns(nk, n):
    return {"ones": rc.ones(nk, n), "zeros": rc.zeros(nk, n), "column0": rc.column(nk, n, 0),
            "column_last": rc.column(nk, n, n - 1), "ramp": rc.ramp(nk, n), "checker": rc.checker(nk, n),
            "bursts": rc.bursts(nk, n, 3), "dense": rc.dense(nk, n, 7)}


@pytest.mark.parametrize("n", SMALL_N + [300])
def test_patterns_set_no_bit_at_or_past_n(n):
    nk, nb = 2 * n + 9, (n + 7) // 8
    for name, rows in _patterns(nk, n).items():
        assert rows.shape == (nk, nb) and rows.dtype == np.uint8, name
        allbits = np.unpackbits(rows, axis=1, bitorder="little")
        assert not allbits[:, n:].any(), name
        padded = rc.with_pad_bits(rows, n)
        pb = np.unpackbits(padded, axis=1, bitorder="little")
        assert pb[:, n:].all() and np.array_equal(pb[:, :n], allbits[:, :n]), name
        assert np.array_equal(rc.pack(rc.unpack(rows, n)), rows), name
    p = _patterns(nk, n)
    bits = rc.unpack(p["ramp"], n).sum(axis=1)
    assert np.array_equal(bits, np.arange(nk) % (n + 1)) and set(bits) == set(range(n + 1))  # every histogram slot
    assert rc.unpack(p["ones"], n).all() and not p["zeros"].any()
    assert np.array_equal(rc.unpack(p["column_last"], n).sum(axis=0), [0] * (n - 1) + [nk])
    assert np.array_equal(rc.unpack(p["bursts"], n).all(axis=1), np.arange(nk) % 4 != 3)
    assert np.array_equal(p["checker"][0::2, 0], np.full((nk + 1) // 2, 0xAA if n >= 8 else 0xAA & ((1 << n) - 1), np.uint8))
    assert np.array_equal(p["checker"][1::2, 0], np.full(nk // 2, 0x55 if n >= 8 else 0x55 & ((1 << n) - 1), np.uint8))


def test_offsets_follow_the_row_buffer_rule():
    offs, total = rc.contig_offsets([1, 99, 16, 0, 5], 3)
    assert offs == [0, 16, 320, 368, 368] and total == 384
    assert rc.bin_length(70001) == 700 and rc.bin_length(99) == 1 and rc.bin_length(3 * 10 ** 7) == 200000
    assert rc.bin_length(70001, 5000, 1) == 5000 and rc.bin_length(300, 5000, 1) == 300
    for nk in (1, 99, 100, 20000, 70001, 2 * 10 ** 7 + 1):
        assert rc.bin_length(nk) == max(1, po.bin_length(nk))


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("binlen, step", [(1, 1), (7, 7), (100, 100), (5000, 3)])
def test_ref_stats_equals_window_stats_over_the_bins(n, binlen, step):
    nk = 1234
    rows = np.concatenate([rc.dense(400, n, n), rc.ramp(300, n), rc.ones(200, n), rc.checker(234, n), rc.zeros(100, n)])
    bins, cs, low = rc.ref_stats(rows, n, binlen, step)
    starts = np.arange(0, nk, binlen)
    hist, wcs = po.window_stats(rows, n, starts, starts + binlen)
    assert bins.dtype == np.int64 and cs.dtype == np.int64
    assert np.array_equal(bins, hist) and np.array_equal(cs, wcs.sum(axis=0))
    assert bins.sum() == nk and np.array_equal(low, rows[np.arange(0, nk, step)])


def _frames(rows, n, size_step, binlen, omit, keep_cols):
    """(frame from ref_bin_colsums, frame from bitmap_to_bins) of one contig's rows sampled every `size_step`-th row"""
    names = pd.Index([f"g{i}" for i in range(n)], name="name")
    pos = np.arange(0, len(rows), size_step)
    frame = pd.DataFrame(rc.unpack(rows, n)[::size_step], index=pd.RangeIndex(0, len(rows), size_step), columns=names)
    want = ref.bitmap_to_bins(frame, binlen, omit, [names[i] for i in keep_cols] if keep_cols else None)
    b, s, e = Genome.similarity_bin_geometry(len(rows), size_step, binlen)
    assert np.array_equal(np.unique(pos // binlen), b)
    cs, kept = rc.ref_bin_colsums(rows, n, s, e, size_step, rc.words_of(n, keep_cols) if keep_cols else None, omit)
    return Genome._similarity_frame(cs.astype(np.uint64), kept.astype(np.uint64), b * binlen, names), want


@pytest.mark.parametrize("n, keep_cols", [(3, [0, 2]), (3, [1]), (9, [8]), (9, [0, 4]), (40, [1, 33]), (40, [39])])
@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("use_keep", [False, True])
def test_ref_bin_colsums_equals_bitmap_to_bins(n, keep_cols, omit, use_keep):
    rows = np.concatenate([rc.dense(900, n, 3 * n), rc.ones(260, n), rc.zeros(240, n), rc.bins_rows(n)[1],
                           rc.with_pad_bits(rc.dense(333, n, 5), n)])
    for step, binlen in ((1, 100), (7, 250), (3, 1000)):
        got, want = _frames(rows, n, step, binlen, omit, keep_cols if use_keep else None)
        pd.testing.assert_frame_equal(got, want, obj=f"step {step} bin {binlen}")
    # the edges occur: a bin of rows of ones (all dropped with omit: 1.0 by the fill value), an all-zero bin (NaN) without a keep mask
    got, _ = _frames(rows, n, 1, 100, omit, keep_cols if use_keep else None)
    assert (got[1000] == 1.0).all()
    assert got[1200].isna().all() == (not use_keep)
    s, e = np.array([1000, 900]), np.array([1100, 1200])
    kept = rc.ref_bin_colsums(rows, n, s, e, 1, None, omit)[1]
    assert list(kept) == ([0, 40] if omit else [100, 300])


def test_classes_counts_the_four_kinds():
    n = 9
    rows = rc.pack(np.array([[1] * 9, [1] * 8 + [0], [0] * 9, [0, 1, 0, 0, 0, 0, 0, 0, 0], [1, 0] + [1] * 7, [1] * 9], np.uint8))
    assert np.array_equal(rc.classes(rows, n, rc.words_of(n, [1])), [[1, 1], [2, 2]])
    assert np.array_equal(rc.classes(rows, n, None), [[4, 2], [0, 0]])
    per_bin = rc.classes(rows, n, rc.words_of(n, [8]), [0, 2, 6], [2, 6, 6])
    assert np.array_equal(per_bin, [[[0, 1], [0, 1]], [[2, 0], [1, 1]], [[0, 0], [0, 0]]])
    assert np.array_equal(rc.keep_bits(40, rc.words_of(40, [1, 33])), np.isin(np.arange(40), [1, 33]))


@pytest.mark.parametrize("n", rc.BINS_N)
def test_planted_bins_hold_every_class_of_row(n):
    """The condition of test_gpu_rows_craft.py's k_bin_colsums cases: for every keep mask and stride, every bin of at least
    BINS_MIN_ROWS sampled rows holds rows with and without a keep bit that do and do not end up with all N bits (without a
    keep mask: rows of all N bits and others), so both sides of the keep rule and of omit_fixed run in every such bin."""
    rows = rc.bins_rows(n)
    assert [len(r) for r in rows] == rc.BINS_NK
    for r in rows:
        assert not np.unpackbits(r, axis=1, bitorder="little")[:, n:].any()
    for name, cols in rc.keep_cases(n).items():
        kw = None if cols is None else rc.words_of(n, cols)
        assert cols is None or all(0 <= g < n for g in cols)
        for stride in rc.BINS_STRIDES:
            contigs, starts, ends = rc.bins_cases(stride)
            lens = (ends - starts).astype(np.int64)
            assert (lens == 0).any() and (lens == 1).any() and (starts[lens >= rc.BINS_MIN_ROWS] % 256 != 0).any()
            assert stride != 1 or 200000 in lens
            big = 0
            for c in range(len(rows)):
                m = contigs == c
                assert (ends[m].astype(np.int64) <= (len(rows[c]) - 1) // stride + 1).all()
                cl = rc.classes(rows[c], n, kw, starts[m], ends[m], stride)
                assert np.array_equal(cl.sum(axis=(1, 2)), lens[m])
                for t, ln in zip(cl, lens[m]):
                    if ln >= rc.BINS_MIN_ROWS:
                        big += 1
                        assert (t[0] > 0).all() and (cols is None or (t[1] > 0).all()), (name, stride, t)
                    if cols is None:
                        assert (t[1] == 0).all()
            assert big >= 4


def test_planted_statistics_rows_cover_the_ceilings():
    """what test_gpu_rows_craft.py's statistics cases rest on: whole tiles of 1024 rows in ONE histogram slot (slot N and
    slot 0), every column set over more consecutive rows than any carry-save plane holds (255), runs of ones of 255, 256
    and 257 rows, every slot 0..N hit"""
    for n in (1, 13, 130):
        rows = rc.stats_rows(n)
        assert [len(r) for r in rows] == rc.STATS_NK
        popc = [rc.unpack(r, n).sum(axis=1) for r in rows]
        assert (popc[8] == n).all() and len(popc[8]) == 1024 and (popc[9] == 0).all()
        big = popc[-1]
        assert (big[:36000] == n).all()
        assert set(np.concatenate(popc)) == set(range(n + 1))
        full = np.concatenate([[0], (big == n).astype(np.int8), [0]])
        edges = np.flatnonzero(np.diff(full))
        runs = set(edges[1::2] - edges[0::2])
        assert {255, 256, 257} <= runs


# ---------------------------------------------------------------------------
# the flush of the counter planes in the middle of a contig: the model of the walk (tests/epi_walk.py) and what
# tests/test_gpu_planes_flush.py claims to reach
# ---------------------------------------------------------------------------
def _mid(w):
    return [f for f in w.flushes if f.site != "end"]


def test_walk_model_restates_the_launch_shape():
    assert [ew.kernel_of(n) for n in (1, 8, 9, 64, 65, 128, 129, 256)] == ["b1", "b1", "n", "n", "w", "w", "chunks", "chunks"]
    assert [ew.maxb_for(n) for n in (8, 13, 61, 72, 128, 130, 520)] == [128, 128, 49, 42, 23, 23, 16]
    assert [ew.minbin(m) for m in (128, 49, 42, 23, 16)] == [9, 22, 26, 49, 74]
    # about 16 tiles per workgroup until a launch holds more than 16 384 tiles, then 128 at the most
    assert [ew.grid_for(t) for t in (1, 15, 16, 196, 16384, 16400, 131072, 10 ** 6)] == [1, 1, 1, 12, 1024, 1024, 1024, 2048]
    assert [ew.grid_for(196, b) for b in (0, 1, 2, 12, 13, 10 ** 9)] == [1, 1, 2, 12, 12, 12]
    for gt in (4, 8):
        for ntiles, grid in ((196, 1), (196, 2), (196, 12), (5, 3), (1, 1)):
            rg = [ew.epi_range(gt, ntiles, j, grid) for j in range(grid)]
            assert rg[0][0] == 0 and rg[-1][1] == ntiles and all(a[1] == b[0] for a, b in zip(rg, rg[1:]))
            assert all(b % gt == 0 for b, _ in rg)
    assert ew.epi_range(4, 196, 1, 2) == (96, 196)
    # rows per lane and tile of the chunk kernel: 4 * IPT (a partial tile: its iterations of 4 steps that hold a row)
    assert [ew.chunk_rows_per_tile(n) for n in (130, 256, 300, 400, 512, 520)] == [8, 8, 16, 16, 16, 24]
    assert ew.chunk_rows_per_tile(130, 300) == 4 and ew.chunk_rows_per_tile(130, 513) == 8
    for nk in rc.FLUSH_NK + rc.STATS_NK:
        for g in ({}, dict(max_bin_len=5000, min_bin_count=1), dict(max_bin_len=22, min_bin_count=1)):
            assert ew.bin_length(nk, **g) == rc.bin_length(nk, **g)
    assert ew.tiles_of([1, 1024, 1025])[0] == [0, 1, 2, 2] and ew.tiles_of(rc.FLUSH_NK)[1] == [0, 61, 193]
    assert (ew.PLANES_FLUSH, ew.PLANES_CEIL) == (240, 255)


def test_planted_flush_rows_stand_at_the_ceiling():
    """every column of every row set over the 60 full tiles of the first contig and the first 64 tiles of the long one (a thread's
    planes hold the highest count at the first flush), runs of ones of 255, 256 and 257 rows behind, every slot hit"""
    assert rc.FLUSH_NK[0] == 60 * 1024 + 77 and rc.FLUSH_NK[1] > 130 * 1024 and rc.FLUSH_NK[1] % 1024
    for n in (8, 13, 128, 130):
        rows = rc.flush_rows(n)
        assert [len(r) for r in rows] == rc.FLUSH_NK
        popc = [rc.unpack(r, n).sum(axis=1) for r in rows]
        assert (popc[0][:60 * 1024] == n).all() and (popc[1][:64 * 1024] == n).all()
        rest = popc[1][64 * 1024:]
        full = np.concatenate([[0], (rest == n).astype(np.int8), [0]])
        edges = np.flatnonzero(np.diff(full))
        assert {255, 256, 257} <= set(edges[1::2] - edges[0::2])
        assert set(rest) == set(range(n + 1))
        assert rc.unpack(rows[1], n).sum(axis=0).min() > 64 * 1024 + 10000 > rc.unpack(rows[1], n)[64 * 1024:].sum(axis=0).min()


@pytest.mark.parametrize("n", rc.FLUSH_N)
def test_flush_cases_reach_their_sites_under_the_bound(n):
    """the reach tests/test_gpu_planes_flush.py rests on, by the model of the walk: under PG_EPI_WORKGROUPS = 1 every site of the
    width's kernel is met at least twice inside one contig with rows of that contig behind the last flush; under 2 the second
    workgroup starts inside the long contig, has more than 60 of its tiles and meets the site again"""
    kern = ew.kernel_of(n)
    geoms = rc.flush_geometries(n)
    assert all(g is not None for g in geoms.values()), geoms
    # (rows of 10 bytes: the one bin length that mixes groups and single tiles, 53 rows, pairs the single tiles up under both
    # bounds — no flush at 252 rows there; every other width of k_epilogue_w, both group sizes' instantiations, has one)
    assert set(geoms) == {"b1": {"default", "long_bins"}, "n": {"default", "long_bins", "one_tile"},
                          "w": {"default", "long_bins"} | ({"carry252"} if n != 77 else set()),
                          "chunks": {"default", "long_bins"}}[kern]
    assert [(m, g) for m, g in rc.flush_cases() if m == n] == [(n, g) for g in geoms]
    _, tile0 = ew.tiles_of(rc.FLUSH_NK)
    walks = {(g, b): ew.walk(n, rc.FLUSH_NK, b, **geom) for g, geom in geoms.items() for b in rc.FLUSH_BOUNDS}
    for (g, b), w in walks.items():
        assert len(w.ranges) == b and all(f.vrows % 4 == 0 and 0 < f.vrows <= ew.PLANES_CEIL for f in w.flushes), (g, b)
        if b == 2:
            begin, end = w.ranges[1]
            assert tile0[1] < begin < tile0[2] and min(end, tile0[2]) - begin > 60, w.ranges
    if kern == "b1":
        assert not any(w.flushes for w in walks.values())  # (accumulators of its own)
        return
    plain = {"n": "n.group", "w": "w", "chunks": "chunks"}[kern]
    site_of = {"default": plain, "long_bins": plain, "one_tile": "n.tile", "carry252": "w"}
    for g in geoms:
        w1, w2 = walks[g, 1], walks[g, 2]
        site = site_of[g]
        assert {f.site for f in _mid(w1)} == {site}, (g, _mid(w1))
        if g != "carry252":  # (with groups and single tiles in turn the two flushes of the long contig may come under either bound)
            assert ew.reaches(w1, site, times=2), (g, w1.flushes)
            assert len(ew.mid_contig(w1, site)[0, 1]) >= 2  # (workgroup 0, the long contig)
        assert any(f.wg == 1 and f.contig == 1 for f in _mid(w2)), (g, w2.flushes)  # the workgroup that starts inside the long contig
    if kern == "n":
        # the contig of exactly 60 tiles: the flush comes with its last full tile, the partial tile's 4 rows leave at the contig's end
        for g in ("default", "one_tile"):
            fl = [f for f in walks[g, 1].flushes if f.contig == 0]
            assert [(f.site, f.vrows) for f in fl] == [(site_of[g], 240), ("end", 4)], fl
        assert set(walks["one_tile", 1].paths.values()) == {"tile"} and "unwindowed" not in walks["default", 1].paths.values()
    if kern == "w":
        # the plain group walk (two tiles = 8 rows a group) flushes at 248: the carry of weight 8 held back
        for g in ("default", "long_bins"):
            assert {f.vrows for f in _mid(walks[g, 1])} == {248}, g
        if "carry252" not in geoms:
            return
        # groups and single tiles in turn: 252 rows, the carries of weight 4 and 8 held back — under one of the bounds
        both = _mid(walks["carry252", 1]) + _mid(walks["carry252", 2])
        assert 252 in {f.vrows for f in both}, both
        long_paths = [walks["carry252", 1].paths[t] for t in range(tile0[1], tile0[2])]
        assert {"group", "tile"} <= set(long_paths)
    if kern == "chunks":
        assert ew.chunk_rows_per_tile(n) == 8 and len(_mid(walks["default", 1])) >= 6


def test_carry_geometry_of_128_genomes():
    """bins of 90 rows at N = 128: a group of two tiles spans MAXB = 23 or 24 bins in turn, so groups and single tiles
    alternate inside the long contig and a flush comes at 252 rows (the shortest such bins the model finds)"""
    assert ew.carry_bins(128, rc.FLUSH_NK) == dict(max_bin_len=90, min_bin_count=1)
    w = ew.walk(128, rc.FLUSH_NK, 1, max_bin_len=90, min_bin_count=1)
    assert sorted(f.vrows for f in _mid(w) if f.contig == 1) == [248, 252]
    assert ew.reaches(w, "w", times=1, vrows=252)


@pytest.mark.parametrize("n", [m for m in rc.STATS_N if ew.kernel_of(m) in ("n", "w")] + [130, 256])
def test_default_launch_shape_reaches_no_mid_contig_flush(n):
    """THE GAP the bound closes, written down: with PG_EPI_WORKGROUPS unset neither the flush cases nor the statistics cases of
    tests/test_gpu_rows_craft.py meet a single mid-contig flush at rows of 2..16 bytes (nor at 17 and 32 bytes) — a workgroup
    gets 16 to 20 tiles.  Nobody should believe the default-shaped tests cover these lines."""
    for geom in (rc.flush_geometries(n) if n in rc.FLUSH_N else {}).values():
        w = ew.walk(n, rc.FLUSH_NK, None, **geom)
        assert len(w.ranges) == 12 and not _mid(w), (geom, _mid(w))
        assert max(f.vrows for f in w.flushes) <= 4 * 20 * (2 if ew.kernel_of(n) == "chunks" else 1)
    for geom in rc.STATS_GEOMETRY.values():
        assert not _mid(ew.walk(n, rc.STATS_NK, None, **geom)), geom
