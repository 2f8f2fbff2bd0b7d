"""CPU: the crafted-rows helper (tests/rows_craft.py) — its references against the restatements the suite already trusts
(oracle.pyoracle.window_stats, tests/intros_ref.bitmap_to_bins), its pattern generators, and the coverage the GPU tests
(tests/test_gpu_rows_craft.py) claim for the rows they plant."""
import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd.index import Genome
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
