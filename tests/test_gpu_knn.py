"""GPU: k_knn_rows / k_knn_rows_wide (panagram_amd/csrc/pg_knn.hip) through engine.knn_rows.  idx and d2 must be BIT-EQUAL to
the numpy restatement (tests/knn_ref.py): float32 sums over the columns in order, entries sorted by (d2, row number).

Which kernel runs where: D <= 8, 32, 64, 128 k_knn_rows with the query row in that many registers, beyond k_knn_rows_wide
(32-column chunks); K <= 4, 8, 16, 32 list slots; blocks of 64 query rows while 256-row tiles would number fewer than 512,
of 256 beyond."""
import numpy as np
import pytest

from tests import knn_ref

pytestmark = pytest.mark.gpu

N = 600
DS = [1, 3, 8, 9, 33, 64, 65, 128, 129, 300]
KS = [1, 2, 4, 5, 32]
_cache = {}


def crafted(D, n=N, seed=0):
    """random float32; c / m with small integers (what the binning produces); copies of the first rows (ties at distance 0
    where the row itself is NOT the lowest row number); all-zero rows; rows differing only in the last column; 0/1 rows of
    a few patterns (many equal distances)"""
    rng = np.random.default_rng(seed + D)
    X = np.zeros((n, D), np.float32)
    X[0:100] = rng.standard_normal((100, D)).astype(np.float32)
    m = rng.integers(1, 12, (100, 1))
    X[100:200] = (rng.integers(0, 12, (100, D)) % (m + 1) / m).astype(np.float32)
    X[200:260] = X[0:60]
    X[300:400] = X[150]
    X[300:400, D - 1] = (np.arange(100) % 17 * 0.25).astype(np.float32)
    pats = (rng.random((5, D)) < 0.5).astype(np.float32)
    X[400:600] = pats[rng.integers(0, 5, 200)]
    return X


def reference(D):
    if D not in _cache:
        X = crafted(D)
        _cache[D] = (X, knn_ref.knn_rows(X, max(KS)))
    return _cache[D]


def bit_equal(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DS)
def test_knn_on_crafted_rows(ctx, D, K):
    from panagram_amd import engine
    X, (widx, wd2) = reference(D)
    idx, d2 = engine.knn_rows(ctx, X, K)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == (N, K)
    # (a sorted list's first K entries are the K nearest: the reference is computed once, at the largest K)
    assert np.array_equal(idx, widx[:, :K]), (D, K, np.argwhere(idx != widx[:, :K])[:5])
    assert bit_equal(d2, np.ascontiguousarray(wd2[:, :K])), (D, K)
    assert (d2[:, 0] == 0).all()
    if K >= 2:  # a copy of row i sorts row i before itself
        assert np.array_equal(idx[200:260, 0], np.arange(60)) and np.array_equal(idx[200:260, 1], np.arange(200, 260))


def _segments(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


@pytest.mark.parametrize("D,K", [(9, 4), (64, 5), (129, 4), (8, 32)])
def test_segment_shapes(ctx, D, K):
    """empty, shorter than K (padded with -1 / inf), K, K + 1, around a wave, around a 256-row tile, three tiles; the
    segments' starts are no multiples of 64; blocks of 64 query rows"""
    from panagram_amd import engine
    lengths = [0, 1, 2, K, K + 1, 63, 64, 65, 255, 256, 257, 700]
    seg = _segments(lengths)
    assert all(int(s) % 64 for s in seg[2:-1])
    X = np.random.default_rng(D).integers(0, 4, (int(seg[-1]), D)).astype(np.float32) / 3  # (few values: many ties)
    widx, wd2 = knn_ref.knn_rows(X, K, seg)
    idx, d2 = engine.knn_rows(ctx, X, K, seg)
    assert np.array_equal(idx, widx) and bit_equal(d2, wd2)
    assert (idx[0] == [0] + [-1] * (K - 1)).all() and np.isinf(d2[0, 1:]).all()
    for lo, hi in zip(seg[:-1], seg[1:]):  # nobody leaves its segment
        part = idx[int(lo):int(hi)]
        assert ((part == -1) | ((part >= int(lo)) & (part < int(hi)))).all()


def test_many_segments_take_256_row_tiles(ctx):
    """more than 512 tiles: blocks of 256 query rows (partly filled tiles, a segment of three tiles, empty segments)"""
    from panagram_amd import engine
    lengths = [700, 257, 256, 5, 0] + [1, 2, 3] * 170
    seg = _segments(lengths)
    assert sum((n + 255) // 256 for n in lengths) >= 512
    X = np.random.default_rng(3).integers(0, 3, (int(seg[-1]), 33)).astype(np.float32) / 2
    widx, wd2 = knn_ref.knn_rows(X, 4, seg)
    idx, d2 = engine.knn_rows(ctx, X, 4, seg)
    assert np.array_equal(idx, widx) and bit_equal(d2, wd2)


def test_single_segment_equals_no_segments(ctx):
    from panagram_amd import engine
    X, (widx, wd2) = reference(9)
    idx, d2 = engine.knn_rows(ctx, X, 4, [0, N])
    assert np.array_equal(idx, widx[:, :4]) and bit_equal(d2, np.ascontiguousarray(wd2[:, :4]))
    e_idx, e_d2 = engine.knn_rows(ctx, np.zeros((0, 9), np.float32), 4)
    assert e_idx.shape == (0, 4) and e_d2.shape == (0, 4)


@pytest.mark.parametrize("shape,K,seg", [((10, 4), 0, None), ((10, 4), 33, None), ((10, 0), 4, None), ((2, 4097), 4, None),
                                         ((10, 4), 4, [0, 7, 5, 10]), ((10, 4), 4, [1, 10]), ((10, 4), 4, [0, 9])])
def test_argument_errors(ctx, shape, K, seg):
    """K = 0, K = 33, D = 0, D = 4097, descending offsets, offsets that do not run from 0 to n: PG_E_INVALID, with a message"""
    from panagram_amd import engine
    from panagram_amd._lib import PanagramHipError
    with pytest.raises(PanagramHipError) as e:
        engine.knn_rows(ctx, np.zeros(shape, np.float32), K, seg)
    assert e.value.code == -1 and "pg_knn_rows" in str(e.value)
