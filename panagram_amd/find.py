"""Presence/absence patterns over the genomes of a pan-k-mer bitmap: the host side of ``Genome.find_pattern`` — no import of
the GPU library in here.

The rule (include/panagram_hip.h: pg_result_find_runs): two sets of genomes, ``have`` and ``lack``, and two thresholds; a
row matches iff at least ``min_have`` of the ``have`` genomes hold its k-mer and at most ``max_lack`` of the ``lack``
genomes do.  ``min_have = len(have)`` and ``max_lack = 0``, the defaults, are the expression scripts/query_index.py's
"custom" branch spells out column by column; other thresholds are quorum rules ("at least 3 of these 4, at most 1 of
those").  The kernel returns the maximal runs of matching sampled rows; what is done with runs on the host is here."""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Tuple

import numpy as np


def _columns(names: Sequence[str], genomes, what: str) -> list:
    names = list(names)
    cols = []
    for g in genomes:
        if isinstance(g, (int, np.integer)) and not isinstance(g, bool):
            i = int(g)
            if not 0 <= i < len(names):
                raise ValueError(f"{what}: column {i} out of range (0..{len(names) - 1})")
        else:
            if g not in names:
                raise ValueError(f"{what}: unknown genome {g!r}")
            i = names.index(g)
        cols.append(i)
    return sorted(set(cols))


def rule_words(names: Sequence[str], have, lack=(), min_have: Optional[int] = None, max_lack: int = 0):
    """(have_words, lack_words, min_have, max_lack) of a rule over the genomes ``names`` (the bitmap's columns, in order):
    ``have`` / ``lack`` are genome names or column numbers; the words are ceil(N / 32) uint32 each, bit g of a set = bit
    g % 32 of word g // 32.  ``min_have=None``: every ``have`` genome.  ValueError on an unknown genome, a genome in both
    sets and a negative threshold; a threshold that cannot be met (min_have > len(have)) is legal and matches nothing."""
    n = len(names)
    h, l = _columns(names, have, "have"), _columns(names, lack, "lack")
    both = sorted(set(h) & set(l))
    if both:
        raise ValueError(f"genome {names[both[0]]!r} is in both sets")
    min_have = len(h) if min_have is None else int(min_have)
    max_lack = int(max_lack)
    if min_have < 0 or max_lack < 0:
        raise ValueError(f"min_have and max_lack must not be negative, got {min_have}, {max_lack}")
    words = np.zeros((2, (n + 31) // 32), np.uint32)
    for k, cols in enumerate((h, l)):
        for g in cols:
            words[k, g // 32] |= np.uint32(1 << (g % 32))
    return words[0], words[1], min_have, max_lack


def join_pieces(pieces: Iterable[Tuple[int, int, np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    """Runs found piece by piece -> the runs of the whole.  A piece is (first, n, starts, ends): its ``n`` sampled rows are
    the whole's sampled rows [first, first + n), its runs [starts[i], ends[i]) count from the piece's first sampled row,
    sorted.  Pieces come in order.  A run that ends on a piece's last sampled row and one that starts on the first sampled
    row of the piece right behind it are ONE run: each piece was searched as a window of its own, whose edges cut runs."""
    S, E = [], []
    for first, n, starts, ends in pieces:
        S.append(np.asarray(starts, np.int64) + int(first))
        E.append(np.asarray(ends, np.int64) + int(first))
    if not S:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    S, E = np.concatenate(S), np.concatenate(E)
    if len(S) == 0:
        return S, E
    glue = S[1:] == E[:-1]  # (inside a piece runs are maximal: one ends where the next begins only across an edge)
    return S[np.concatenate([[True], ~glue])], E[np.concatenate([~glue, [True]])]


def merge_runs(starts, ends, min_len: int = 1, max_gap: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(starts, ends, rows) of the spans left when neighbouring runs separated by at most ``max_gap`` non-matching sampled
    rows are merged and then the spans shorter than ``min_len`` sampled rows are dropped; ``rows`` = the matching sampled
    rows inside each span.  Runs are [start, end) in sampled rows, sorted and disjoint."""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    if int(min_len) < 1 or int(max_gap) < 0:
        raise ValueError(f"min_len must be positive and max_gap not negative, got {min_len}, {max_gap}")
    if len(starts) != len(ends):
        raise ValueError("starts and ends need one entry per run")
    if len(starts) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    head = np.concatenate([[True], starts[1:] - ends[:-1] > int(max_gap)])  # a run that opens a span
    at = np.flatnonzero(head)
    s, e = starts[at], ends[np.concatenate([at[1:] - 1, [len(ends) - 1]])]
    rows = np.add.reduceat(ends - starts, at)
    keep = e - s >= int(min_len)
    return s[keep], e[keep], rows[keep]
