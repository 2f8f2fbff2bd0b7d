"""The viewer's UMAP files, restated without umap-learn (``panagram/index.py:1107-1156``: ``Genome.write_umaps`` and ``run_umap``).

The reference bins a chromosome's low-resolution bitmap into pair counts, hands the bins x genomes matrix to
``umap.UMAP(n_neighbors, min_dist, n_components=2, random_state=42)`` and clusters the embedding with ``DBSCAN(eps, min_samples)``.
Here the matrix comes from ``Genome.kmer_similarity_bins`` (k_bin_colsums), the exact k-nearest-neighbour graph from
``engine.knn_rows`` (k_knn_rows) — the one step whose cost grows with the square of the bins — and the rest, O(bins x epochs),
stays on the host: umap-learn's documented graph construction (``fuzzy_graph``), its curve fit (``find_ab``), a layout with its
schedule (``layout``) and DBSCAN's labels (``dbscan``).

NOT claimed: umap-learn's numbers.  Its neighbour search is approximate and its layout a lock-free parallel stochastic gradient
descent, so no two installations agree on an embedding anyway.  Claimed, and tested: the file layout the viewer reads, the
exact input matrix, an exact neighbour graph, the graph construction, a deterministic layout — the same input gives the same
bytes — and the cluster labels.  Deviations of the layout from ``optimize_layout_euclidean``, on purpose: one synchronous update
per epoch (every gradient of an epoch is taken at the epoch's starting positions and summed per vertex), epochs counted from
1 (an edge of the largest weight is sampled in every epoch, the first included), negative samples drawn from one seeded
generator, and a PCA start where the graph is not connected."""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import numpy as np
import pandas as pd

logger = logging.getLogger(__name__)

SMOOTH_K_TOLERANCE = 1e-5  # umap-learn's
MIN_K_DIST_SCALE = 1e-3
COLUMNS = ["chrom", "start", "end", "umap1", "umap2", "cluster"]


# ---------------------------------------------------------------------------
# the input matrix (index.py:1111-1121)
# ---------------------------------------------------------------------------
def paircount_matrix(genome, bin_size: int) -> Tuple[pd.DataFrame, np.ndarray]:
    """(frame of ``chrom``, ``start``; n x N float32 matrix): one row per bin of ``bin_size`` positions of every chromosome,
    in ``chrs.tsv`` order — ``bitmap_to_paircount_bins(query(chrom, step=lowres_step), bin_size).T.fillna(0)``, binned on the
    GPU (``Genome.kmer_similarity_bins``)."""
    bins = genome.kmer_similarity_bins(step=int(genome.index.lowres_step), bin_size=int(bin_size))
    chrom, start, rows = [], [], []
    for c, frame in bins.items():
        chrom.append(np.full(frame.shape[1], c, dtype=object))
        start.append(np.asarray(frame.columns, np.int64))
        rows.append(np.nan_to_num(frame.to_numpy(np.float64).T, nan=0.0).astype(np.float32))
    N = genome.ngenomes
    index = pd.DataFrame({"chrom": np.concatenate(chrom) if chrom else np.zeros(0, object),
                          "start": np.concatenate(start) if start else np.zeros(0, np.int64)})
    X = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, N), np.float32))
    return index, X


# ---------------------------------------------------------------------------
# the fuzzy graph (umap-learn: smooth_knn_dist, compute_membership_strengths, fuzzy_simplicial_set)
# ---------------------------------------------------------------------------
def smooth_knn_dist(dist: np.ndarray, k: float, n_iter: int = 64) -> Tuple[np.ndarray, np.ndarray]:
    """(sigma, rho) per row of the n x K neighbour DISTANCES (first entry: the row itself): rho the smallest non-zero
    distance (``local_connectivity = 1``), sigma by bisection so that sum_{j >= 1} exp(-max(d_j - rho, 0) / sigma) is
    log2(k) to within SMOOTH_K_TOLERANCE, then floored at MIN_K_DIST_SCALE times the mean distance."""
    dist = np.asarray(dist, np.float64)
    n = dist.shape[0]
    finite = np.isfinite(dist)
    pos = finite & (dist > 0)
    rho = np.where(pos.any(axis=1), np.where(pos, dist, np.inf).min(axis=1), 0.0)
    target = np.log2(k)
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    active = np.ones(n, bool)
    d = dist[:, 1:] - rho[:, None]
    for _ in range(n_iter):
        if not active.any():
            break
        with np.errstate(over="ignore", invalid="ignore"):
            psum = np.where(d > 0, np.exp(-d / mid[:, None]), 1.0).sum(axis=1)
        active &= np.abs(psum - target) >= SMOOTH_K_TOLERANCE
        up = active & (psum > target)
        down = active & ~up
        hi = np.where(up, mid, hi)
        lo = np.where(down, mid, lo)
        mid = np.where(up, (lo + hi) / 2.0, mid)
        mid = np.where(down, np.where(np.isinf(hi), mid * 2.0, (lo + hi) / 2.0), mid)
    sigma = mid
    row_mean = np.where(finite, dist, 0.0).sum(axis=1) / np.maximum(finite.sum(axis=1), 1)
    all_mean = dist[finite].mean() if finite.any() else 0.0
    floor = MIN_K_DIST_SCALE * np.where(rho > 0, row_mean, all_mean)
    return np.maximum(sigma, floor), rho


def fuzzy_graph(idx: np.ndarray, d2: np.ndarray, n_neighbors: int):
    """The symmetric fuzzy graph (scipy CSR, float64, weights in (0, 1]) of an exact neighbour table: ``idx`` / ``d2`` are
    n x n_neighbors row numbers and SQUARED distances sorted by (d2, row), the row itself among them, as ``engine.knn_rows``
    gives them (-1 / inf: no neighbour).  Membership strengths as umap-learn computes them, then A + A^T - A o A^T."""
    import scipy.sparse as sp
    idx = np.asarray(idx)[:, :n_neighbors]
    dist = np.sqrt(np.asarray(d2, np.float64)[:, :n_neighbors])
    n, K = idx.shape
    sigma, rho = smooth_knn_dist(dist, float(n_neighbors))
    rows = np.repeat(np.arange(n), K)
    cols = idx.ravel().astype(np.int64)
    d = dist.ravel() - rho[rows]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        val = np.where((d <= 0) | (sigma[rows] == 0), 1.0, np.exp(-d / sigma[rows]))
    val[cols == rows] = 0.0
    keep = cols >= 0
    A = sp.coo_matrix((val[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    A.eliminate_zeros()
    T = A.T.tocsr()
    G = (A + T - A.multiply(T)).tocsr()
    G.eliminate_zeros()
    G.sort_indices()
    return G


# ---------------------------------------------------------------------------
# the curve (umap-learn: find_ab_params)
# ---------------------------------------------------------------------------
def _curve(x, a, b):
    return 1.0 / (1.0 + a * x ** (2 * b))


def ab_target(spread: float = 1.0, min_dist: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """the 300 points umap-learn fits its curve to: 1 up to ``min_dist``, then exp(-(x - min_dist) / spread)"""
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    return xv, yv


def find_ab(spread: float = 1.0, min_dist: float = 0.0) -> Tuple[float, float]:
    """(a, b) of 1 / (1 + a x^(2b)), least squares against ``ab_target``"""
    from scipy.optimize import curve_fit
    xv, yv = ab_target(spread, min_dist)
    params, _ = curve_fit(_curve, xv, yv)
    return float(params[0]), float(params[1])


# ---------------------------------------------------------------------------
# the layout (umap-learn: simplicial_set_embedding, optimize_layout_euclidean)
# ---------------------------------------------------------------------------
def _fix_signs(v: np.ndarray) -> np.ndarray:
    """each column's entry of largest magnitude made positive: an eigenvector's sign is arbitrary"""
    v = np.array(v, np.float64)
    for c in range(v.shape[1]):
        if v[np.argmax(np.abs(v[:, c])), c] < 0:
            v[:, c] = -v[:, c]
    return v


def _pca(X: np.ndarray, dim: int = 2) -> np.ndarray:
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(axis=0, keepdims=True)
    u, s, _ = np.linalg.svd(Xc, full_matrices=False)
    out = np.zeros((X.shape[0], dim))
    m = min(dim, u.shape[1])
    out[:, :m] = u[:, :m] * s[:m]
    return _fix_signs(out)


def _spectral(graph, dim: int = 2) -> Optional[np.ndarray]:
    """eigenvectors 2 .. dim + 1 of the normalised Laplacian I - D^-1/2 A D^-1/2, taken as the LARGEST of D^-1/2 A D^-1/2
    (the same vectors; Lanczos finds the large end faster), from a fixed start vector.  None where ARPACK gives up."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n = graph.shape[0]
    deg = np.asarray(graph.sum(axis=0)).ravel()
    inv = sp.diags(1.0 / np.sqrt(deg))
    M = (inv @ graph @ inv).tocsr()
    k = dim + 1
    if n <= max(64, k + 1):
        w, v = np.linalg.eigh(M.toarray())
    else:
        try:
            w, v = spl.eigsh(M, k=k, which="LA", v0=np.ones(n), tol=1e-6, maxiter=n * 5, ncv=max(2 * k + 1, int(np.sqrt(n))))
        except spl.ArpackError:
            return None
    order = np.argsort(-w, kind="stable")[1:k]
    return _fix_signs(v[:, order])


def initial_positions(graph, X, seed: int = 42) -> np.ndarray:
    """spectral where the graph is connected, the first two principal components of ``X`` otherwise; scaled so that the
    largest |coordinate| is 10, plus N(0, 1e-4) noise from ``default_rng(seed)``"""
    from scipy.sparse.csgraph import connected_components
    n = graph.shape[0]
    init = None
    if n > 3 and connected_components(graph, directed=False)[0] == 1:
        init = _spectral(graph)
    if init is None:
        init = _pca(X)
    top = np.abs(init).max()
    if top > 0:
        init = init * (10.0 / top)
    return init + np.random.default_rng(seed).normal(scale=1e-4, size=init.shape)


def default_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


def layout(graph, X, n_epochs: Optional[int], a: float, b: float, seed: int = 42, negative_sample_rate: int = 5,
           gamma: float = 1.0, init: Optional[np.ndarray] = None) -> np.ndarray:
    """n x 2 float64 positions of the graph's vertices: umap-learn's schedule — an edge of weight w is sampled every
    max(w) / w epochs, ``negative_sample_rate`` repulsive samples per attractive one, the step alpha falling linearly from 1,
    every gradient component clipped to +-4 — applied as ONE synchronous update per epoch.  Deterministic."""
    n = graph.shape[0]
    n_epochs = default_epochs(n) if not n_epochs else int(n_epochs)
    y = np.array(initial_positions(graph, X, seed) if init is None else init, np.float64)
    g = graph.tocoo()
    g.sum_duplicates()
    w = np.asarray(g.data, np.float64)
    if w.size == 0:
        return y
    keep = w >= w.max() / n_epochs
    head, tail, w = np.asarray(g.row)[keep], np.asarray(g.col)[keep], w[keep]
    order = np.lexsort((tail, head))
    head, tail, w = head[order], tail[order], w[order]
    eps = w.max() / w  # epochs per sample (n_epochs / (n_epochs * w / max w))
    next_pos = eps.copy()
    neg = negative_sample_rate > 0
    eps_neg = eps / negative_sample_rate if neg else None
    next_neg = eps_neg.copy() if neg else None
    rng = np.random.default_rng(seed)

    def clip(v):
        return np.clip(v, -4.0, 4.0)

    for epoch in range(1, n_epochs + 1):
        alpha = 1.0 - (epoch - 1) / n_epochs
        fire = np.nonzero(next_pos <= epoch)[0]
        if fire.size == 0:
            continue
        h, t = head[fire], tail[fire]
        move = np.zeros_like(y)
        delta = y[h] - y[t]
        d2 = (delta * delta).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            coeff = np.where(d2 > 0, -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0), 0.0)
        grad = clip(coeff[:, None] * delta) * alpha
        np.add.at(move, h, grad)
        np.add.at(move, t, -grad)
        next_pos[fire] += eps[fire]
        if neg:
            cnt = np.floor((epoch - next_neg[fire]) / eps_neg[fire]).astype(np.int64)
            cnt = np.maximum(cnt, 0)
            hh = np.repeat(h, cnt)
            other = rng.integers(0, n, size=hh.size)
            delta = y[hh] - y[other]
            d2 = (delta * delta).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                coeff = np.where(d2 > 0, 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0)), 0.0)
            np.add.at(move, hh, clip(coeff[:, None] * delta) * alpha)
            next_neg[fire] += cnt * eps_neg[fire]
        y += move
    return y


# ---------------------------------------------------------------------------
# clusters (sklearn.cluster.DBSCAN's labels)
# ---------------------------------------------------------------------------
def dbscan(points: np.ndarray, eps: float, min_samples: int = 1) -> np.ndarray:
    """DBSCAN's labels.  With ``min_samples == 1`` every point is a core point, and the clusters are the connected
    components of the graph joining points at most ``eps`` apart, numbered by their first row — which is how sklearn numbers
    them.  Beyond, sklearn does it."""
    points = np.asarray(points, np.float64)
    n = len(points)
    if int(min_samples) != 1:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError as e:
            raise RuntimeError("dbscan: min_samples > 1 needs scikit-learn (only min_samples = 1 is restated here)") from e
        return np.asarray(DBSCAN(eps=eps, min_samples=int(min_samples)).fit_predict(points), np.int64)
    if n == 0:
        return np.zeros(0, np.int64)
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    pairs = cKDTree(points).query_pairs(float(eps), output_type="ndarray")
    adj = sp.coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, lab = connected_components(adj, directed=False)
    _, first = np.unique(lab, return_index=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[lab]


# ---------------------------------------------------------------------------
# run_umap (index.py:1131-1156)
# ---------------------------------------------------------------------------
def run_umap(X: np.ndarray, index_frame: pd.DataFrame, args, ctx=None, knn=None, name: str = "") -> pd.DataFrame:
    """The frame ``chrom start end umap1 umap2 cluster`` of ONE embedding: the rows of ``X`` (n x N float32) are the bins that
    ``index_frame`` (``chrom``, ``start``) names, ``args`` the ``UMAP`` section (neighbors, dist, eps, samples, bin_size).
    ``knn``: (idx, d2) of these rows from ``engine.knn_rows``, row numbers counted from this matrix's first row, at least
    ``n_neighbors`` columns — else they are computed on ``ctx``'s GPU.  ``n_neighbors = min(args.neighbors, n - 1)``; fewer
    than 3 rows, or fewer than 2 neighbours, get what the reference writes when umap fails: zeros, with a warning."""
    X = np.ascontiguousarray(X, np.float32)
    n = len(X)
    out = pd.DataFrame({"chrom": np.asarray(index_frame["chrom"]), "start": np.asarray(index_frame["start"], np.int64)})
    k = min(int(args.neighbors), n - 1)
    if n < 3 or k < 2:
        if n:
            logger.warning("%s UMAP failed for at least one chromosome", name)
        out["umap1"], out["umap2"], out["cluster"] = 0, 0, 0
    else:
        if knn is None:
            from . import engine
            knn = engine.knn_rows(ctx, X, k)
        graph = fuzzy_graph(knn[0], knn[1], k)
        a, b = find_ab(1.0, float(args.dist))
        emb = layout(graph, X, None, a, b)
        out["umap1"], out["umap2"] = emb[:, 0], emb[:, 1]
        out["cluster"] = dbscan(emb, float(args.eps), int(args.samples))
    out["end"] = out["start"] + int(args.bin_size)
    return out[COLUMNS]
