"""numpy restatement of k_knn_rows (pg_knn.hip): exact k nearest neighbours among the rows of a float32 matrix, per segment.

d2(i, j) is accumulated in float32 over the columns IN ORDER, each subtract, multiply and add rounded to float32 (numpy's
float32 arithmetic does exactly that: no fused multiply-add); a row's entries are sorted by (d2, row number); a segment of
fewer than k rows is padded with (-1, +inf)."""
import numpy as np


def d2_matrix(X: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """[hi - lo, hi - lo] float32 squared distances among rows lo .. hi - 1"""
    S = np.ascontiguousarray(X[lo:hi], np.float32)
    acc = np.zeros((hi - lo, hi - lo), np.float32)
    for g in range(S.shape[1]):
        d = S[:, None, g] - S[None, :, g]
        acc = acc + d * d
    assert acc.dtype == np.float32
    return acc


def knn_rows(X: np.ndarray, k: int, seg=None):
    X = np.ascontiguousarray(X, np.float32)
    n = len(X)
    seg = [0, n] if seg is None else [int(s) for s in seg]
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf, np.float32)
    for lo, hi in zip(seg[:-1], seg[1:]):
        if hi <= lo:
            continue
        D = d2_matrix(X, lo, hi)
        rows = np.arange(lo, hi)
        m = min(k, hi - lo)
        for i in range(hi - lo):
            order = np.lexsort((rows, D[i]))[:m]
            idx[lo + i, :m] = rows[order]
            d2[lo + i, :m] = D[i, order]
    return idx, d2
