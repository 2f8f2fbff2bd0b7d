"""The presence profile k_presence_profile computes (panagram_amd/csrc/pg_profile.hip; include/panagram_hip.h:
pg_result_presence_profile), restated in numpy straight from the definitions: per genome its column of a window of rows, the
runs of set rows from np.diff of the padded column, and ``covered`` by MARKING the bases [i, i + k) of every set row — not by
the identity covered = hits + sum of min(k - 1, L) + (k - 1 if hits), which tests/test_search_cpu.py checks against this.  No
tests in here: tests/test_search_cpu.py ties the model to a hand-written loop and to tests/gaps_ref.py,
tests/test_gpu_presence_profile.py and tests/test_gpu_search_e2e.py hold the kernel and Index.search to it."""
import numpy as np

from tests import rows_craft as rc

FIELDS = ("hits", "runs", "longest", "first", "end", "covered")


def ref_window(bits, k, cols=None):
    """(profile [N, 6] = hits, runs, longest, first, end, covered; (all, none)) of ONE window whose rows are ``bits`` [rows, N]
    0 / 1; ``cols``: the selected columns (None: all), everything of the others zero; all / none over the selected columns,
    zero when none is selected"""
    bits = np.asarray(bits, np.uint8)
    n, N = bits.shape
    sel = list(range(N)) if cols is None else sorted(set(int(c) for c in cols))
    out = np.zeros((N, len(FIELDS)), np.int64)
    if n == 0 or not sel:
        return out, (0, 0)
    chosen = bits[:, sel]
    pt = np.ascontiguousarray(chosen.T).astype(np.int32)                # (a column's rows side by side)
    pad = np.zeros((len(sel), 1), np.int32)
    d = np.diff(np.concatenate([pad, pt, pad], axis=1), axis=1)
    g, s = np.nonzero(d == 1)                                           # per column, in row order: a run's first row ...
    g2, e = np.nonzero(d == -1)                                         #    ... and the row behind its last
    assert np.array_equal(g, g2)
    longest, first, end = np.zeros(len(sel), np.int64), np.full(len(sel), n, np.int64), np.zeros(len(sel), np.int64)
    np.maximum.at(longest, g, e - s)
    np.minimum.at(first, g, s)
    np.maximum.at(end, g, e)
    # the window's n + k - 1 bases, one counter each: every set row i marks bases [i, i + k) (+1 at i, -1 behind i + k - 1)
    marks = np.zeros((len(sel), n + k), np.int32)
    marks[:, :n] += pt
    marks[:, k:] -= pt
    covered = (np.cumsum(marks, axis=1)[:, :n + k - 1] > 0).sum(axis=1)
    hits = pt.sum(axis=1)
    out[sel, 0], out[sel, 1], out[sel, 2] = hits, np.bincount(g, minlength=len(sel)), longest
    out[sel, 3], out[sel, 4], out[sel, 5] = np.where(hits > 0, first, 0), end, covered
    return out, (int(chosen.all(axis=1).sum()), int((~chosen.any(axis=1)).sum()))


def ref_presence_profile(rows, n, k, contigs, starts, ends, cols=None):
    """what AnchorResult.presence_profile returns for the windows over the contigs' packed ``rows``: (profile [nwin, N, 6],
    rows [nwin, 2]) as int64"""
    bits = {}
    prof, allnone = np.zeros((len(starts), n, len(FIELDS)), np.int64), np.zeros((len(starts), 2), np.int64)
    for i, (c, s, e) in enumerate(zip(contigs, starts, ends)):
        c, s, e = int(c), int(s), int(e)
        if c not in bits:
            bits[c] = rc.unpack(np.asarray(rows[c], np.uint8), n)
        prof[i], allnone[i] = ref_window(bits[c][s:e], k, cols)
    return prof, allnone


def gap_lengths(p):
    """the lengths L of the runs of absent rows that lie between two set rows of column ``p``"""
    d = np.diff(np.concatenate([[1], np.asarray(p, np.int8), [1]]))
    s, e = np.flatnonzero(d == -1), np.flatnonzero(d == 1)
    inner = (s > 0) & (e < len(p))
    return (e - s)[inner]
