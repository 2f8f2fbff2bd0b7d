"""The absence runs k_absence_runs computes (panagram_amd/csrc/pg_gaps.hip), restated in numpy the obvious way: unpack the
window's sampled rows and take np.diff of every column's padded absence vector.  No tests in here: tests/test_gaps_cpu.py ties
the restatement to a hand-written loop, tests/test_gpu_absence_runs.py holds the kernel to it."""
import numpy as np

from tests import rows_craft as rc


def ref_window(bits, maxlen, cols=None):
    """(runs [m, 3] = (genome, first row, rows) of the CLOSED runs sorted by (genome, first row), hist [N, maxlen + 1],
    absent [N], edges [N, 2]) of ONE window whose sampled rows are ``bits`` [rows, N] 0 / 1; ``cols``: the selected columns
    (None: all), everything of the others zero"""
    m, n = bits.shape
    a = 1 - np.asarray(bits, np.int8)                                   # 1. absence
    if cols is not None:
        keep = np.zeros(n, bool)
        keep[list(cols)] = True
        a = a * keep[None, :]
    at = np.ascontiguousarray(a.T)                                      #    (a column's rows side by side)
    pad = np.zeros((n, 1), np.int8)
    d = np.diff(np.concatenate([pad, at, pad], axis=1), axis=1)         # 2. padded: edges cut runs
    g, s = np.nonzero(d == 1)                                           # 3. per column, in row order: a run's first row ...
    g2, e = np.nonzero(d == -1)                                         #    ... and the row behind its last
    assert np.array_equal(g, g2)
    closed = (s > 0) & (e < m)                                          # 4. a present row on both sides
    hist = np.zeros((n, maxlen + 1), np.int64)
    np.add.at(hist, (g[closed], np.minimum(e - s, maxlen)[closed]), 1)  # 5. the spectrum, its last bin open-ended
    edges = np.zeros((n, 2), np.int64)                                  # 6. the runs at the edges stay open
    edges[g[s == 0], 0] = (e - s)[s == 0]
    edges[g[e == m], 1] = (e - s)[e == m]
    runs = np.stack([g, s, e - s], axis=1)[closed].astype(np.int64)
    return runs, hist, a.sum(axis=0, dtype=np.int64), edges


def ref_absence_runs(rows, n, contigs, starts, ends, stride, maxlen, min_len=1, max_len=0, cols=None):
    """what AnchorResult.absence_runs returns for the windows over the contigs' ``rows``: (runs [total, 4] = (window, genome,
    first sampled row of the contig, rows) sorted by (window, genome, first row), hist [nwin, N, maxlen + 1], absent
    [nwin, N], edges [nwin, N, 2])"""
    bits = {}
    out, hist, absent, edges = [], [], [], []
    for i, (c, s, e) in enumerate(zip(contigs, starts, ends)):
        c, s, e = int(c), int(s), int(e)
        if c not in bits:
            bits[c] = rc.unpack(np.asarray(rows[c], np.uint8)[::stride], n)
        r, h, a, ed = ref_window(bits[c][s:e], maxlen, cols)
        r = r[(r[:, 2] >= min_len) & ((r[:, 2] <= max_len) if max_len else True)]
        out.append(np.concatenate([np.full((len(r), 1), i, np.int64), r + np.array([0, s, 0], np.int64)], axis=1))
        hist.append(h)
        absent.append(a)
        edges.append(ed)
    if not out:
        return np.zeros((0, 4), np.int64), np.zeros((0, n, maxlen + 1), np.int64), np.zeros((0, n), np.int64), np.zeros((0, n, 2), np.int64)
    return np.concatenate(out), np.stack(hist), np.stack(absent), np.stack(edges)


# ---------------------------------------------------------------------------
# the planted variants, shared by tests/test_gaps_cpu.py (rows by the oracle) and tests/test_gpu_gaps_e2e.py (an index)
# ---------------------------------------------------------------------------
PLANTED_K, PLANTED_LEN, PLANTED_SEED = 21, 3000, 3
# (first row, rows, class, site, span) of the four runs genome 1 must show against genome 0, by the arithmetic of gaps.classify
PLANTED_RUNS = [(480, 21, "sub", 500, 1), (880, 28, "del_or_multi", 900, 8), (1380, 23, "del_or_multi", 1400, 3),
                (1980, 20, "ins", 2000, 0)]


def planted_genomes(seed=PLANTED_SEED):
    """(anchor, variant) as code arrays 0..3: a random anchor of 3 kb, and the same with one substitution at base 500, two
    substitutions at bases 900 and 907, bases 1400..1402 deleted and two bases inserted before base 2000 — each more than 2 k
    from its neighbours.  A substituted base is the old one + 1; the inserted bases differ from the anchor base on their
    outer side, so the insertion cannot be shifted.  (Whether the deletion can be shifted depends on the anchor: the caller
    asserts that it cannot.)"""
    a = np.random.default_rng(seed).integers(0, 4, PLANTED_LEN, dtype=np.uint8)
    b = a.copy()
    for p in (500, 900, 907):
        b[p] = (a[p] + 1) & 3
    ins = np.array([(a[2000] + 1) & 3, (a[1999] + 1) & 3], np.uint8)
    b = np.concatenate([b[:1400], b[1403:2000], ins, b[2000:]])
    return a, b
