"""GPU: the kernels that read finished bitmap rows and reduce them, on rows PLANTED into a rows container
(tests/rows_craft.py) instead of rows anchored from synthetic genomes: every column set at once for tiles on end, every row
of a tile in one histogram slot, rows of all N bits with and without a keep bit, bits past N, bytes around the rows that are
not zero — at every row width.  The references are the plain numpy restatements of tests/rows_craft.py, tied on the CPU to
oracle.pyoracle.window_stats and tests/intros_ref.bitmap_to_bins (tests/test_rows_craft_cpu.py); every comparison is exact.

Which kernel runs for which N (bytes per row = ceil(N / 8)):
  rows_epilogue   1 byte k_epilogue_b1; 2..8 bytes k_epilogue_n<2..8>; 9..16 bytes k_epilogue_w<9..16>; 17 bytes (N = 130)
                  k_epilogue_chunks<2,false>; 32 bytes (N = 256) k_epilogue_chunks<2,true>; 38 bytes (N = 300)
                  k_epilogue_chunks<3,false>; 50 bytes (N = 400) k_epilogue_chunks<4,false>; 64 bytes (N = 512)
                  k_epilogue_chunks<4,true>; 65 bytes (N = 520) k_epilogue_chunks<0,false>; k_lowres with lowres_step=7
                  (the flushes of the counter planes in the middle of a contig: tests/test_gpu_planes_flush.py)
  window_stats    k_window_stats
  bin_colsums     N <= 128 k_bin_colsums<4>, beyond k_bin_colsums<0>
with_pad_bits (bits past N) is planted for k_bin_colsums only, whose header states the rule for them; the statistics
kernels have no written rule for such bits and no writer of the rows sets them."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import rows_craft as rc

pytestmark = pytest.mark.gpu

K = 21
_rows_cache = {}


def _cached(kind, n):
    """the planted rows of one case, made once (a test module's cases come N by N: one entry per kind is enough)"""
    if _rows_cache.get(kind, (None,))[0] != n:
        _rows_cache[kind] = (n, {"stats": rc.stats_rows, "window": rc.window_rows, "bins": rc.bins_rows}[kind](n))
    return _rows_cache[kind][1]


# ---------------------------------------------------------------------------
# a. the statistics pass
# ---------------------------------------------------------------------------
def _stats_outputs(res, want_cs):
    from panagram_amd._lib import PanagramHipError
    out = []
    for ci in range(len(res.seqs.lens)):
        rows, low, bins, info = res.download(ci)
        out.append((rows, low, bins, info))
    if want_cs:
        return out, res.contig_colsums()
    with pytest.raises(PanagramHipError, match="PG_ANCHOR_COLSUMS"):  # column sums that were not asked for are refused
        res.contig_colsums()
    return out, None


def _check_stats(ctx, n, geom_name, poison=None):
    """plant the statistics rows, run the pass twice, hold every output to the reference; returns the outputs"""
    geom = rc.STATS_GEOMETRY[geom_name]
    step, want_cs = geom.get("lowres_step", 100), geom.get("colsums", True)
    rows = _cached("stats", n)
    res = rc.container(ctx, K, n, rc.STATS_NK, **geom)
    try:
        rc.plant(res, rows, poison=poison)
        res.rows_epilogue()
        first, first_cs = _stats_outputs(res, want_cs)
        res.rows_epilogue()  # the statistics start from zero: a second pass gives the same
        again, again_cs = _stats_outputs(res, want_cs)
    finally:
        res.close()
    assert (first_cs is None and again_cs is None) or np.array_equal(first_cs, again_cs)
    for ci, (r, nk) in enumerate(zip(rows, rc.STATS_NK)):
        tag = f"N {n} {geom_name} poison {poison} contig {ci} ({nk} rows)"
        got_rows, got_low, got_bins, info = first[ci]
        binlen = rc.bin_length(nk, geom.get("max_bin_len", 200000), geom.get("min_bin_count", 100))
        assert info["nkmers"] == nk and info["binlen"] == binlen, tag
        bins, cs, low = rc.ref_stats(r, n, binlen, step)
        assert np.array_equal(got_rows, r), tag
        assert got_low.shape == low.shape and np.array_equal(got_low, low), tag
        assert got_bins.shape == bins.shape and np.array_equal(got_bins.astype(np.int64), bins), tag
        assert not want_cs or np.array_equal(first_cs[ci].astype(np.int64), cs), tag
        for a, b in zip(first[ci][:3], again[ci][:3]):
            assert np.array_equal(a, b), tag
    return first, first_cs


@pytest.mark.parametrize("n, geom", [(n, g) for n in rc.STATS_N for g in rc.STATS_GEOMETRY],
                         ids=[f"N{n}_{g}" for n in rc.STATS_N for g in rc.STATS_GEOMETRY])
def test_statistics_pass_on_crafted_rows(ctx, n, geom):
    """rows_epilogue (k_epilogue* by row width, k_lowres) on 13 contigs of 1 to 70 001 rows around the tile of 1024: the rows
    come back as planted, the low-resolution rows are rows[::step], bins and column sums equal the reference — with whole
    tiles in ONE histogram slot and every column set over more consecutive rows than the carry-save planes and packed
    counters hold between flushes; bins of 1 row to 5000 rows (longer than a tile); a second pass gives the same."""
    _check_stats(ctx, n, geom)


# ---------------------------------------------------------------------------
# b. bytes outside the rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 13, 77, 300])
def test_statistics_ignore_bytes_outside_the_rows(ctx, n):
    """every byte of the row buffer that is no row byte — the padding that rounds each contig's rows up to 16 bytes and the 16
    bytes of slack behind the last row — filled with 0x00 and with 0xFF: all outputs equal the reference, hence each other.
    (Nothing defines these bytes in production: a recycled row buffer is not cleared, k_probe stores row bytes only.)"""
    for geom in rc.STATS_GEOMETRY:
        a, a_cs = _check_stats(ctx, n, geom, poison=0x00)
        b, b_cs = _check_stats(ctx, n, geom, poison=0xFF)
        assert (a_cs is None and b_cs is None) or np.array_equal(a_cs, b_cs)
        for x, y in zip(a, b):
            assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]


# ---------------------------------------------------------------------------
# c. k_window_stats
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.WINDOW_N)
def test_window_stats_on_crafted_rows(ctx, n):
    """windows that are empty, one row long, start and end at multiples of 256 +- 1, run past the contig's end, lie behind it,
    and the whole contig of 200 000 rows (several pieces per window) — with and without column sums, on the rows and on the
    low-resolution rows — equal oracle.pyoracle.window_stats"""
    rows = _cached("window", n)
    res = rc.container(ctx, K, n, rc.WINDOW_NK)
    try:
        rc.plant(res, rows)
        res.rows_epilogue()
        for ci, r in enumerate(rows):
            for step in (1, 100):
                rr = r[::step]
                starts, ends = rc.windows(len(rr))
                want_h, want_cs = po.window_stats(rr, n, starts, ends)
                assert want_h.sum(axis=1).max() == len(rr) and want_h[0].sum() == 0
                if n > 1 and ci == 0 and step == 1:
                    assert (want_h[-1] > 0).all()  # every slot 0..N is hit (the ramp)
                h, cs = res.window_stats(ci, starts, ends, step=step)
                assert np.array_equal(h.astype(np.int64), want_h), (n, ci, step)
                assert np.array_equal(cs.astype(np.int64), want_cs), (n, ci, step)
                h, cs = res.window_stats(ci, starts, ends, step=step, colsums=False)
                assert cs is None and np.array_equal(h.astype(np.int64), want_h), (n, ci, step)
    finally:
        res.close()


# ---------------------------------------------------------------------------
# d. k_bin_colsums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.BINS_N)
def test_bin_colsums_on_crafted_rows(ctx, n):
    """k_bin_colsums<4> (N <= 128) / <0> against the rule of pg_bins.hip's header: no keep mask, a column that is not always
    set, a column in every 32-bit word, the last column; omit_fixed off and on; strides 1, 7, 100; bins that start off the
    multiples of 256, a bin of 200 000 sampled rows (cut into many pieces), one-row and empty bins, bins of three contigs in one launch.
    Every bin of 64 rows and more holds every class of row (tests/test_rows_craft_cpu.py).  The same again with the bits past
    N set in every row: nothing changes."""
    rows = _cached("bins", n)
    padded = [rc.with_pad_bits(r, n) for r in rows] if n % 8 else None
    res = rc.container(ctx, K, n, rc.BINS_NK, colsums=False)
    res_pad = rc.container(ctx, K, n, rc.BINS_NK, colsums=False) if padded else None
    try:
        rc.plant(res, rows)
        res.rows_epilogue()  # (a rows container is read once its statistics have been enqueued)
        if res_pad is not None:
            rc.plant(res_pad, padded, poison=0xFF)
            res_pad.rows_epilogue()
        dropped = 0
        for name, cols in rc.keep_cases(n).items():
            kw = None if cols is None else rc.words_of(n, cols)
            for stride in rc.BINS_STRIDES:
                contigs, starts, ends = rc.bins_cases(stride)
                lens = (ends - starts).astype(np.int64)
                for omit in (False, True):
                    tag = f"N {n} keep {name} stride {stride} omit {omit}"
                    want_cs = np.zeros((len(contigs), n), np.int64)
                    want_kept = np.zeros(len(contigs), np.int64)
                    for c in range(len(rows)):
                        m = contigs == c
                        want_cs[m], want_kept[m] = rc.ref_bin_colsums(rows[c], n, starts[m], ends[m], stride, kw, omit)
                    cs, kept = res.bin_colsums(contigs, starts, ends, step=1, stride=stride, keep_words=kw, omit_fixed=omit)
                    assert np.array_equal(kept.astype(np.int64), want_kept), tag
                    assert np.array_equal(cs.astype(np.int64), want_cs), tag
                    if res_pad is not None:
                        cs2, kept2 = res_pad.bin_colsums(contigs, starts, ends, step=1, stride=stride, keep_words=kw, omit_fixed=omit)
                        assert np.array_equal(kept2, kept) and np.array_equal(cs2, cs), tag + " (bits past N set)"
                    if omit:  # rows are dropped where the reference says so, in the long bins and in a one-row bin
                        short = want_kept < lens
                        assert short[lens >= rc.BINS_MIN_ROWS].all() and (short & (lens == 1)).any(), tag
                        assert (kept.astype(np.int64)[short] < lens[short]).all(), tag
                        dropped += int((lens - want_kept).sum())
                    else:
                        assert np.array_equal(want_kept, lens), tag
        assert dropped > 0
    finally:
        res.close()
        if res_pad is not None:
            res_pad.close()
