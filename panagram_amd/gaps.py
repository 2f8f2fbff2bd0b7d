"""Absence runs over the genomes of a pan-k-mer bitmap: the host side of ``Genome.absence_runs`` — no import of the GPU library
in here.

The rule (include/panagram_hip.h: pg_result_absence_runs): per genome, the maximal runs of consecutive sampled rows that lack
its bit.  A run is CLOSED when a present row bounds it on both sides; the two runs that touch the edges of what was searched are
OPEN, their true length unknown.  Row r of bitmap.1 is the k-mer at anchor bases [r, r + k), so the LENGTH of a closed run says
what kind of difference made it (``classify``).  The kernel returns, per window, the closed runs, their length spectrum, the
absent rows and the two open runs; what is done with them on the host — joining the pieces of a region, the classes, the
tables — is here."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

import numpy as np
import pandas as pd

CLASSES = ("sub", "ins", "del_or_multi", "short", "open")


def select_words(names: Sequence[str], genomes=None) -> Tuple[np.ndarray, List[str]]:
    """(words, selected names in column order) of a selection over the genomes ``names`` (the bitmap's columns, in order), built
    as ``patterns.select_words`` builds it but of any number of genomes: ``genomes`` are names or column numbers, None all of
    them; the words are ceil(N / 32) uint32, bit g of the set = bit g % 32 of word g // 32.  ValueError on an unknown genome,
    a column out of range, a genome given twice and an empty selection."""
    names = list(names)
    cols = []
    for g in range(len(names)) if genomes is None else genomes:
        if isinstance(g, (int, np.integer)) and not isinstance(g, bool):
            i = int(g)
            if not 0 <= i < len(names):
                raise ValueError(f"column {i} out of range (0..{len(names) - 1})")
        else:
            if g not in names:
                raise ValueError(f"unknown genome {g!r}")
            i = names.index(g)
        if i in cols:
            raise ValueError(f"genome {names[i]!r} is selected twice")
        cols.append(i)
    if not cols:
        raise ValueError("no genome selected")
    words = np.zeros((len(names) + 31) // 32, np.uint32)
    for g in cols:
        words[g // 32] |= np.uint32(1 << (g % 32))
    return words, [names[g] for g in sorted(cols)]


def check_lengths(maxlen: int, min_len: int, max_len: int) -> None:
    """the argument checks of the entry point, made before anything is read"""
    if not 1 <= int(maxlen) <= 4096:
        raise ValueError(f"maxlen must be 1 to 4096, got {maxlen}")
    if int(min_len) < 1 or int(max_len) < 0:
        raise ValueError(f"min_len must be positive and max_len not negative, got {min_len}, {max_len}")


def _selected(rows, min_len: int, max_len: int):
    rows = np.asarray(rows)
    return (rows >= int(min_len)) & ((rows <= int(max_len)) if int(max_len) else np.ones(rows.shape, bool))


def join_pieces(pieces: Iterable[tuple], ngenomes: int, maxlen: int, min_len: int = 1, max_len: int = 0):
    """Results found piece by piece -> the result of the whole: (runs [M, 3] int64, hist [N, maxlen + 1], absent [N],
    edges [N, 2]; the last three int64).  A piece is (first, n, runs, hist, absent, edges): its ``n`` sampled rows are the
    whole's sampled rows [first, first + n), searched as ONE window — ``runs`` [m, 3] = (genome, first sampled row counted from
    the piece's own first row, rows) of its selected closed runs, ``hist`` [N, maxlen + 1], ``absent`` [N], ``edges`` [N, 2] as
    the kernel leaves them.  Pieces come in order.  Piece p's edge_tail, the pieces behind it that are absent throughout and
    the edge_head of the first piece with a present row are ONE run, closed by the present rows on both its sides: its start
    is known, it is added to the spectrum at min(rows, maxlen), and it is emitted when min_len <= rows (and rows <= max_len
    unless that is 0).  The whole's own first head and last tail stay OPEN — a run is never cut at a piece border.  ``runs`` of
    the whole: (genome, first sampled row of the whole, rows), sorted by (genome, first row)."""
    N, nb = int(ngenomes), int(maxlen) + 1
    hist, absent = np.zeros((N, nb), np.int64), np.zeros(N, np.int64)
    open_, edge_head, seen = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, bool)
    out = []
    for first, n, runs, h, a, edges in pieces:
        first, n = int(first), int(n)
        if n <= 0:
            continue
        h, a, edges = np.asarray(h).astype(np.int64), np.asarray(a).astype(np.int64), np.asarray(edges).astype(np.int64)
        if h.shape != (N, nb) or a.shape != (N,) or edges.shape != (N, 2):
            raise ValueError(f"a piece's tables need the shapes {(N, nb)}, {(N,)} and {(N, 2)}")
        hist += h
        absent += a
        runs = np.asarray(runs, np.int64).reshape(-1, 3)
        out.append(runs + np.array([0, first, 0], np.int64))
        throughout = edges[:, 0] >= n  # no present row in this piece
        rows = open_ + edges[:, 0]
        opens_whole = ~throughout & ~seen
        edge_head[opens_whole] = rows[opens_whole]
        closed = np.flatnonzero(~throughout & seen & (rows > 0))
        np.add.at(hist, (closed, np.minimum(rows[closed], nb - 1)), 1)
        keep = closed[_selected(rows[closed], min_len, max_len)]
        out.append(np.stack([keep, first - open_[keep], rows[keep]], axis=1))
        seen |= ~throughout
        open_ = np.where(throughout, open_ + n, edges[:, 1])
    runs = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    runs = runs[np.lexsort((runs[:, 1], runs[:, 0]))]
    return runs, hist, absent, np.stack([np.where(seen, edge_head, open_), open_], axis=1)


def classify(rows, k: int, start=0, open=False):
    """(class, site, span) of runs of ``rows`` absent rows at step 1, ``start`` the anchor base of a run's first row (arrays or
    scalars; ``open``: the run touches an edge of what was searched, its length is a lower bound):

        rows == k       "sub"           one isolated substitution at base site = start + k - 1             span 1
        rows == k - 1   "ins"           an insertion in the genome before anchor base site = start + k - 1  span 0
        rows >  k       "del_or_multi"  a deletion of span = rows - k + 1 anchor bases from site = start + k - 1 on, or
                                        several substitutions less than k apart, the first at site, the last span - 1 behind it
        rows <  k - 1   "short"         a k-mer over the site occurs elsewhere in the genome; site -1, span 0
        open            "open"          site -1, span 0

    These are CANDIDATES by run-length arithmetic, not calls.  What breaks the arithmetic: repeats — a k-mer the genome holds
    somewhere else keeps its row present, which shortens or splits a run (hence "short"), and a k-mer the genome lacks for
    another reason lengthens one — and N bases in the anchor, whose rows hold no k-mer at all and so read as absent in every
    genome.  An event within k of a contig's end gives an open run.  Presence is presence of the canonical k-mer anywhere in
    the genome, so an inversion or a translocation shows only at its breakpoints."""
    rows, start = np.asarray(rows, np.int64), np.asarray(start, np.int64)
    k = int(k)
    if k < 2:
        raise ValueError(f"k must be at least 2, got {k}")
    rows, start, is_open = np.broadcast_arrays(rows, start, np.asarray(open, bool))
    cls = np.full(rows.shape, "short", object)
    cls[rows == k] = "sub"
    cls[rows == k - 1] = "ins"
    cls[rows > k] = "del_or_multi"
    cls[is_open] = "open"
    sited = (rows >= k - 1) & ~is_open
    site = np.where(sited, start + k - 1, -1)
    span = np.where(sited, rows - k + 1, 0)
    return cls, site.astype(np.int64), span.astype(np.int64)


def spectrum_frame(hist, names: Sequence[str]) -> pd.DataFrame:
    """genome, rows, runs: one row per genome and run length with a closed run, by genome in column order, then rows;
    ``hist`` [N, maxlen + 1], whose last bin ``rows`` = maxlen stands for runs of maxlen rows AND MORE"""
    hist = np.asarray(hist).astype(np.int64)
    if hist.ndim != 2 or hist.shape[0] != len(names):
        raise ValueError("hist needs one row per genome")
    g, L = np.nonzero(hist)
    return pd.DataFrame({"genome": np.array([names[i] for i in g], object), "rows": L.astype(np.int64), "runs": hist[g, L]})


def open_rows(edges, nrows: int) -> np.ndarray:
    """[N] rows in open runs: head + tail, or ``nrows`` where the genome holds no row at all (head = tail = nrows)"""
    edges = np.asarray(edges).astype(np.int64)
    return np.where((edges[:, 0] >= int(nrows)) & (int(nrows) > 0), int(nrows), edges.sum(axis=1))


def summary_frame(hist, absent, open_rows_, nrows: int, names: Sequence[str], k: int) -> pd.DataFrame:
    """genome, rows, absent, runs, sub, ins, del_or_multi, long_rows, sub_per_kb — per genome: the sampled rows searched, the
    absent ones, the closed runs, the runs of each class of ``classify`` (step 1; the spectrum must reach past k: maxlen > k),
    the absent rows in closed runs of maxlen rows and more (absent rows less those in shorter closed runs and the
    ``open_rows_`` [N] of the open runs: ``open_rows``, added up over the regions the tables were added up over), and the "sub"
    runs per 1000 sampled rows"""
    hist, absent = np.asarray(hist).astype(np.int64), np.asarray(absent).astype(np.int64)
    k, maxlen = int(k), hist.shape[1] - 1
    if maxlen <= k:
        raise ValueError(f"the summary needs a spectrum that reaches past k: maxlen {maxlen} <= k {k}")
    short = (hist[:, :maxlen] * np.arange(maxlen)[None, :]).sum(axis=1)
    sub = hist[:, k]
    return pd.DataFrame({"genome": np.array(list(names), object), "rows": np.full(len(names), int(nrows), np.int64), "absent": absent,
                         "runs": hist.sum(axis=1), "sub": sub, "ins": hist[:, k - 1], "del_or_multi": hist[:, k + 1:].sum(axis=1),
                         "long_rows": absent - short - np.asarray(open_rows_).astype(np.int64),
                         "sub_per_kb": sub * 1000.0 / nrows if nrows else np.zeros(len(names))})
