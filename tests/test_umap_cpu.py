"""CPU: the host side of the UMAP files (panagram_amd/umap.py) and the numpy restatement of the neighbour kernel
(tests/knn_ref.py).  Nothing here needs a GPU: the neighbour tables come from the restatement, the binned frames from the host
functions the GPU path shares (Genome.similarity_bin_geometry, Genome._similarity_frame) fed with numpy column sums."""
import dataclasses
import logging

import numpy as np
import pandas as pd
import pytest

from panagram_amd import index as pidx, umap
from tests import knn_ref


# ---------------------------------------------------------------------------
# 1. the restatement itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(1, 3), (7, 4), (40, 9)])
def test_restatement_agrees_with_float64_brute_force(D, K):
    """integer-valued rows: every float32 operation is exact, so float64 brute force gives the same numbers"""
    rng = np.random.default_rng(D)
    X = rng.integers(-6, 7, (150, D)).astype(np.float32)
    seg = [0, 0, 2, 50, 150]
    idx, d2 = knn_ref.knn_rows(X, K, seg)
    for lo, hi in zip(seg[:-1], seg[1:]):
        S = X[lo:hi].astype(np.float64)
        full = ((S[:, None, :] - S[None, :, :]) ** 2).sum(axis=2)
        for i in range(hi - lo):
            order = sorted(range(hi - lo), key=lambda j: (full[i, j], j))[:K]
            m = len(order)
            assert list(idx[lo + i, :m]) == [lo + j for j in order] and list(d2[lo + i, :m]) == [full[i, j] for j in order]
            assert (idx[lo + i, m:] == -1).all() and np.isinf(d2[lo + i, m:]).all()
    assert idx.dtype == np.int32 and d2.dtype == np.float32


# ---------------------------------------------------------------------------
# 2. paircount_matrix
# ---------------------------------------------------------------------------
class _Idx:
    lowres_step = 100
    bitmap_to_paircount_bins = pidx.Index.bitmap_to_paircount_bins
    _bin_ids = staticmethod(pidx.Index._bin_ids)
    _paircount_bins = staticmethod(pidx.Index._paircount_bins)

    def __init__(self, n):
        self.genome_names = pd.Index([f"g{i}" for i in range(n)], name="name")


class _Genome:
    """a genome whose low-resolution bitmaps live in memory: kmer_similarity_bins as Genome's, the kernel's sums by numpy"""

    def __init__(self, n, bitmaps):
        self.index, self.ngenomes, self.bitmaps, self.calls = _Idx(n), n, bitmaps, []

    def query(self, chrom, step):
        return self.bitmaps[chrom]

    def kmer_similarity_bins(self, chroms=None, step=100, bin_size=1_000_000):
        self.calls.append((step, bin_size))
        out = {}
        for c, bm in self.bitmaps.items():
            size = int(bm.index[-1]) + 1
            b, s, e = pidx.Genome.similarity_bin_geometry(size, step, bin_size)
            v = bm.to_numpy().astype(np.uint64)
            cs = np.stack([v[i:j].sum(axis=0) for i, j in zip(s, e)])
            out[c] = pidx.Genome._similarity_frame(cs, (e - s).astype(np.uint64), b * bin_size, self.index.genome_names)
        return out


def _bitmaps(n, sizes, seed=1):
    rng = np.random.default_rng(seed)
    out = {}
    for c, size in sizes.items():
        pos = np.arange(0, size, 100)
        v = (rng.random((len(pos), n)) < 0.6).astype(np.uint8)
        v[(pos // 2000) == 1] = 0  # an all-zero bin: 0 / 0 = NaN -> 0
        out[c] = pd.DataFrame(v, index=pos, columns=[f"g{i}" for i in range(n)])
    return out


def test_paircount_matrix_is_the_pandas_expression():
    """index.py:1111-1121: bitmap_to_paircount_bins(query(chrom, step=lowres_step), bin_size).T.fillna(0), chromosome after
    chromosome; an all-zero bin, last bins of part of a bin's length"""
    g = _Genome(5, _bitmaps(5, {"c1": 10_000, "c2": 7_301, "c3": 2_001}))
    frame, X = umap.paircount_matrix(g, 2000)
    assert g.calls == [(100, 2000)]
    want = pd.concat({c: g.index.bitmap_to_paircount_bins(g.query(c, step=100), 2000).T.fillna(0) for c in g.bitmaps},
                     names=["chrom", "start"])
    assert X.dtype == np.float32 and X.shape == (5 + 4 + 2, 5) and X.flags.c_contiguous
    assert np.array_equal(X, want.to_numpy().astype(np.float32))
    assert list(frame.columns) == ["chrom", "start"]
    assert list(zip(frame["chrom"], frame["start"])) == list(want.index)
    assert not X[1].any() and not X[6].any()  # the all-zero bins
    assert list(frame["start"][-2:]) == [0, 2000] and frame["start"].dtype == np.int64


# ---------------------------------------------------------------------------
# 3. fuzzy_graph
# ---------------------------------------------------------------------------
def test_fuzzy_graph_properties():
    rng = np.random.default_rng(2)
    K = 6
    X = rng.random((300, 8)).astype(np.float32)
    idx, d2 = knn_ref.knn_rows(X, K)
    G = umap.fuzzy_graph(idx, d2, K)
    assert G.shape == (300, 300) and G.dtype == np.float64
    assert abs(G - G.T).max() == 0
    assert (G.data > 0).all() and (G.data <= 1).all() and G.diagonal().sum() == 0
    # umap-learn's own criterion (SMOOTH_K_TOLERANCE) for every row's bandwidth
    dist = np.sqrt(d2.astype(np.float64))
    sigma, rho = umap.smooth_knn_dist(dist, K)
    assert np.array_equal(rho, dist[:, 1])  # (no duplicate rows here: the nearest other row)
    psum = np.exp(-np.maximum(dist[:, 1:] - rho[:, None], 0) / sigma[:, None]).sum(axis=1)
    assert (np.abs(psum - np.log2(K)) < 1e-5).all()
    # a directed strength is exp(-(d - rho) / sigma), 1 for the nearest; the union of the two directions
    i, j = 17, int(idx[17, 1])
    back = np.flatnonzero(idx[j] == i)
    w_ij = 1.0
    w_ji = float(np.exp(-max(dist[j, back[0]] - rho[j], 0) / sigma[j])) if len(back) else 0.0
    assert G[i, j] == pytest.approx(w_ij + w_ji - w_ij * w_ji, abs=1e-15)


def test_fuzzy_graph_keeps_disjoint_supports_apart():
    rng = np.random.default_rng(3)
    X = np.zeros((80, 8), np.float32)
    X[:40, :4] = rng.random((40, 4))
    X[40:, 4:] = rng.random((40, 4))
    idx, d2 = knn_ref.knn_rows(X, 5)
    G = umap.fuzzy_graph(idx, d2, 5).tocoo()
    assert G.nnz and not ((G.row < 40) != (G.col < 40)).any()
    # padded entries (a segment shorter than the table) add no edge
    idx, d2 = knn_ref.knn_rows(X[:3], 5)
    G = umap.fuzzy_graph(idx, d2, 5)
    assert G.shape == (3, 3) and G.nnz == 6


# ---------------------------------------------------------------------------
# 4. find_ab
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("min_dist", [0.0, 0.1])
def test_find_ab_fits_the_target_curve(min_dist):
    """The fitted curve against umap-learn's 300 target points: the mean squared residual — what curve_fit minimises — is
    below 1e-3 (measured 5.8e-4 at min_dist 0, 2.6e-4 at 0.1; no curve of this family is within 1e-3 POINTWISE of a target
    with a kink: umap-learn's own published a = 1.5769, b = 0.8951 for min_dist 0.1 miss it by 0.027).  The fit is a
    minimum — no nearby (a, b) does better — and at min_dist 0.1 it is umap-learn's published pair."""
    a, b = umap.find_ab(spread=1.0, min_dist=min_dist)
    xv, yv = umap.ab_target(1.0, min_dist)
    assert len(xv) == 300 and xv[0] == 0 and xv[-1] == 3 and yv[0] == 1

    def mse(a_, b_):
        return float(((1.0 / (1.0 + a_ * xv ** (2 * b_)) - yv) ** 2).mean())
    best = mse(a, b)
    assert best < 1e-3
    for da, db in [(1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3), (1e-3, 1e-3), (1e-3, -1e-3)]:
        assert mse(a + da, b + db) > best
    if min_dist == 0.1:
        assert a == pytest.approx(1.576943460405378, abs=1e-6) and b == pytest.approx(0.8950608781227859, abs=1e-6)


# ---------------------------------------------------------------------------
# 5, 6. layout
# ---------------------------------------------------------------------------
def _two_point_graph(w=1.0):
    import scipy.sparse as sp
    return sp.csr_matrix(np.array([[0.0, w], [w, 0.0]]))


@pytest.mark.parametrize("a,b,y1,clipped", [(1.5, 0.9, (0.3, -0.4), False), (100.0, 1.0, (0.1, -0.001), True)])
def test_layout_one_attractive_step_by_hand(a, b, y1, clipped):
    """two points, one edge (both directions of it), no negative samples, one epoch at alpha = 1: each direction moves its
    head by clip(c * (y_head - y_tail)) and its tail by the opposite, c = -2ab d^(2(b-1)) / (1 + a d^(2b))"""
    init = np.array([[0.0, 0.0], y1])
    out = umap.layout(_two_point_graph(), None, 1, a, b, negative_sample_rate=0, init=init)
    delta = init[0] - init[1]
    d = float(np.sqrt((delta ** 2).sum()))
    c = -2 * a * b * d ** (2 * (b - 1)) / (1 + a * d ** (2 * b))
    g = np.clip(c * delta, -4, 4)
    assert (np.abs(c * delta) > 4).any() == clipped
    assert np.abs(out[0] - (init[0] + 2 * g)).max() < 1e-12 and np.abs(out[1] - (init[1] - 2 * g)).max() < 1e-12
    assert np.array_equal(init, np.array([[0.0, 0.0], y1]))  # the caller's array is not written


def _planted(seed=5):
    rng = np.random.default_rng(seed)
    X = np.zeros((80, 8), np.float32)
    X[:40, :4] = rng.random((40, 4))
    X[40:, 4:] = rng.random((40, 4))
    return X


def test_layout_is_deterministic():
    Xc = np.random.default_rng(6).random((120, 6)).astype(np.float32)  # one component: the spectral start
    for X, K in ((Xc, 12), (_planted(), 4)):                        # two components: the PCA start
        idx, d2 = knn_ref.knn_rows(X, K)
        G = umap.fuzzy_graph(idx, d2, K)
        a, b = umap.find_ab(1.0, 0.0)
        one, two = umap.layout(G, X, 60, a, b), umap.layout(G.copy(), X.copy(), 60, a, b)
        assert one.dtype == np.float64 and one.shape == (len(X), 2) and np.isfinite(one).all()
        assert one.tobytes() == two.tobytes()
        assert umap.layout(G, X, 60, a, b, seed=7).tobytes() != one.tobytes()
    assert umap.default_epochs(10000) == 500 and umap.default_epochs(10001) == 200


def test_initial_positions_scale():
    X = _planted()
    idx, d2 = knn_ref.knn_rows(X, 4)
    y = umap.initial_positions(umap.fuzzy_graph(idx, d2, 4), X)
    assert abs(np.abs(y).max() - 10) < 1e-3
    assert (y[:40, 0] > 0).all() != (y[40:, 0] > 0).all()  # the first principal component separates the two groups


# ---------------------------------------------------------------------------
# 7. dbscan
# ---------------------------------------------------------------------------
def test_dbscan_min_samples_1_is_sklearns():
    sk = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(8)
    pts = rng.random((200, 2)) * 6
    pts[150:170] = pts[10:30]  # coincident points
    pts[170:175] = pts[0]
    for eps in (0.1, 0.3, 1.0):
        want = sk.DBSCAN(eps=eps, min_samples=1).fit_predict(pts)
        got = umap.dbscan(pts, eps, 1)
        assert got.dtype == np.int64 and np.array_equal(got, want), eps
    assert got[0] == 0 and set(got) == set(range(got.max() + 1))
    assert np.array_equal(umap.dbscan(pts, 0.3, 3), sk.DBSCAN(eps=0.3, min_samples=3).fit_predict(pts))
    assert umap.dbscan(np.zeros((0, 2)), 1.0, 1).shape == (0,)


# ---------------------------------------------------------------------------
# 8. run_umap
# ---------------------------------------------------------------------------
def _args(**kw):
    return dataclasses.replace(pidx.UMAP(), **kw)


@pytest.mark.parametrize("rows", [1, 2])
def test_small_segments_get_the_zero_fallback(rows, caplog):
    frame = pd.DataFrame({"chrom": ["c9"] * rows, "start": np.arange(rows) * 500})
    with caplog.at_level(logging.WARNING, logger="panagram_amd.umap"):
        out = umap.run_umap(np.ones((rows, 4), np.float32), frame, _args(bin_size=500), name="g0")
    assert "UMAP failed" in caplog.text
    assert list(out.columns) == ["chrom", "start", "end", "umap1", "umap2", "cluster"]
    assert (out[["umap1", "umap2", "cluster"]].to_numpy() == 0).all() and list(out["end"] - out["start"]) == [500] * rows


def test_run_umap_from_a_given_neighbour_table():
    """n_neighbors = min(neighbors, rows - 1); the table's first n_neighbors columns are used; end = start + bin_size"""
    X = _planted()
    frame = pd.DataFrame({"chrom": ["c1"] * 80, "start": np.arange(80) * 2000})
    knn = knn_ref.knn_rows(X, 6)
    out = umap.run_umap(X, frame, _args(neighbors=4, bin_size=2000), knn=knn)
    again = umap.run_umap(X, frame, _args(neighbors=4, bin_size=2000), knn=knn_ref.knn_rows(X, 4))
    assert out.equals(again) and list(out.columns) == umap.COLUMNS
    assert np.isfinite(out[["umap1", "umap2"]].to_numpy()).all() and (out["end"] - out["start"] == 2000).all()
    lab = out["cluster"].to_numpy()
    assert lab[0] == 0 and set(lab) == set(range(lab.max() + 1))
    assert not set(lab[:40]) & set(lab[40:])  # no cluster holds bins of both groups
    three = umap.run_umap(X[:3], frame.iloc[:3], _args(neighbors=4), knn=knn_ref.knn_rows(X[:3], 2))
    assert np.isfinite(three[["umap1", "umap2"]].to_numpy()).all() and len(three) == 3


# ---------------------------------------------------------------------------
# 9. the public interface
# ---------------------------------------------------------------------------
def test_cli_umaps(monkeypatch, capsys):
    from panagram_amd.__main__ import main
    wrote, opened = [], []

    class G:
        def __init__(self, name, anchored):
            self.name, self.anchored = name, anchored

        def write_umaps(self):
            wrote.append(self.name)
            return f"{self.name}/chrom_umaps.csv", f"{self.name}/genome_umap.csv"

    class I:
        genomes = {n: G(n, n != "g2") for n in ("g0", "g1", "g2")}
        genome_names = pd.Index(["g0", "g1", "g2"])

        def __getitem__(self, n):
            return self.genomes[n]

        def close(self):
            opened.append("closed")

    def open_index(path, mode=None, device=0):
        opened.append((path, mode, device))
        return I()
    monkeypatch.setattr(pidx, "Index", open_index)
    assert main(["umaps", "some/index", "--device", "0"]) == 0
    assert wrote == ["g0", "g1"] and opened == [("some/index", "r", 0), "closed"]
    assert "g1/genome_umap.csv" in capsys.readouterr().out
    assert main(["umaps", "some/index", "g1"]) == 0 and wrote == ["g0", "g1", "g1"]
    with pytest.raises(SystemExit):
        main(["umaps", "some/index", "g2"])  # not an anchor genome
    assert "not an anchor genome" in capsys.readouterr().err


def test_index_switch_and_file_names(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c1\nACGT\n")
    (tmp_path / "s.tsv").write_text(f"name\tfasta\na\t{fa}\n")
    plain = pidx.Index(str(tmp_path / "s.tsv"), prefix=str(tmp_path / "i0"), prepare=True)
    with_umaps = pidx.Index(str(tmp_path / "s.tsv"), prefix=str(tmp_path / "i1"), prepare=True, umaps=True)
    assert plain.umaps is False and with_umaps.umaps is True
    # config.yaml does not change: the switch describes an invocation
    assert (tmp_path / "i0" / "config.yaml").read_text() == (tmp_path / "i1" / "config.yaml").read_text()
    g = with_umaps["a"]
    assert g.chrom_umaps_filename.endswith("anchor/a/chrom_umaps.csv") and g.genome_umap_filename.endswith("anchor/a/genome_umap.csv")
    g.load_umaps()
    assert g.chrom_umaps is None and g.genome_umap is None
    # the reference's layout, read back as its load_umaps does (index.py:1158-1167; view.py:922, 2197)
    import os
    os.makedirs(g.prefix, exist_ok=True)
    frame = pd.DataFrame({"chrom": ["c1", "c1", "c2"], "start": [0, 10, 0], "end": [10, 20, 10], "umap1": [0.5, 1.5, 2.5],
                          "umap2": [1.0, 2.0, 3.0], "cluster": [0, 0, 1]})
    frame.set_index("chrom").to_csv(g.chrom_umaps_filename)
    frame.to_csv(g.genome_umap_filename, index=False)
    g.load_umaps()
    assert list(g.chrom_umaps.loc["c1"]["start"]) == [0, 10] and len(g.genome_umap.query("chrom == 'c2'")) == 1
