"""The presence/absence pattern spectrum of a pan-k-mer bitmap: the host side of ``Genome.pattern_spectrum`` — no import of the
GPU library in here.

The rule (include/panagram_hip.h: pg_result_pattern_counts): a set of 1 to 64 selected genomes; a row's key is a 64-bit word
whose bit i is the row's bit for the i-th selected genome, in column order; the spectrum gives, for every key that occurs,
the number of rows that have it.  The kernel returns (keys, counts) sorted by key; what is done with them on the host —
adding up pieces, the table with its pattern strings, the rows per number of genomes — is here.  ``find.py`` then tells
where the rows of one pattern are."""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

MAX_SELECTED = 64  # genomes per pattern: a key is one 64-bit word


def select_words(names: Sequence[str], genomes=None) -> Tuple[np.ndarray, List[str]]:
    """(words, selected names in column order) of a selection over the genomes ``names`` (the bitmap's columns, in order):
    ``genomes`` are names or column numbers, None all of them; the words are ceil(N / 32) uint32, bit g of the set = bit
    g % 32 of word g // 32.  ValueError on an unknown genome, a column out of range, a genome given twice, an empty
    selection and more than 64 genomes."""
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
    if len(cols) > MAX_SELECTED:
        raise ValueError(f"{len(cols)} genomes selected: a pattern takes at most {MAX_SELECTED}, select fewer")
    words = np.zeros((len(names) + 31) // 32, np.uint32)
    for g in cols:
        words[g // 32] |= np.uint32(1 << (g % 32))
    return words, [names[g] for g in sorted(cols)]


def merge(parts: Iterable[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    """(keys, counts) pairs of several pieces or chromosomes -> those of the whole: keys ascending and distinct, the counts
    of equal keys added up"""
    parts = [(np.asarray(k, np.uint64), np.asarray(c, np.uint64)) for k, c in parts]
    for k, c in parts:
        if k.shape != c.shape or k.ndim != 1:
            raise ValueError("keys and counts need one entry per pattern")
    if not parts:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    keys, inv = np.unique(np.concatenate([k for k, _ in parts]), return_inverse=True)
    # (bincount adds in float64: exact while a pattern holds fewer than 2^53 rows)
    counts = np.bincount(inv, weights=np.concatenate([c for _, c in parts]).astype(np.float64), minlength=len(keys))
    return keys, counts.astype(np.uint64)


def _bits(keys: np.ndarray, m: int) -> np.ndarray:
    """(len(keys), m) 0/1: bit i of every key"""
    keys = np.asarray(keys, np.uint64)
    return ((keys[:, None] >> np.arange(m, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)


def _checked(keys, counts, m: int):
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint64)
    if not 1 <= int(m) <= MAX_SELECTED:
        raise ValueError(f"a pattern takes 1 to {MAX_SELECTED} genomes, got {m}")
    if keys.shape != counts.shape or keys.ndim != 1:
        raise ValueError("keys and counts need one entry per pattern")
    if m < 64 and len(keys) and int(keys.max()) >> int(m):
        raise ValueError(f"a key has bits at or past the {m} selected genomes")
    return keys, counts


def spectrum_frame(keys, counts, selected_names: Sequence[str], top: Optional[int] = None, min_rows: int = 1) -> pd.DataFrame:
    """pattern, n, rows, frac: one row per pattern — ``pattern`` a string of 0 / 1 with one character per selected genome in
    column order, ``n`` the genomes present, ``rows`` its rows, ``frac`` = rows over the total of ALL patterns given, before
    ``min_rows`` (patterns with fewer rows are dropped) and ``top`` (only the first so many are kept) cut anything.  Sorted by
    rows descending, then pattern ascending."""
    m = len(selected_names)
    keys, counts = _checked(keys, counts, m)
    if int(min_rows) < 0 or (top is not None and int(top) < 0):
        raise ValueError(f"top and min_rows must not be negative, got {top}, {min_rows}")
    bits = _bits(keys, m)
    total = int(counts.sum())
    frame = pd.DataFrame({"pattern": np.array(["".join("1" if b else "0" for b in row) for row in bits], object),
                          "n": bits.sum(axis=1, dtype=np.int64), "rows": counts.astype(np.int64)})
    frame["frac"] = frame["rows"] / total if total else np.zeros(len(frame))
    frame = frame[frame["rows"] >= int(min_rows)].sort_values(["rows", "pattern"], ascending=[False, True], kind="stable")
    if top is not None:
        frame = frame.iloc[:int(top)]
    return frame.reset_index(drop=True)


def occupancy(keys, counts, m: int) -> np.ndarray:
    """[m + 1] int64: the rows whose pattern holds n of the m selected genomes, n = 0..m"""
    keys, counts = _checked(keys, counts, m)
    n = _bits(keys, int(m)).sum(axis=1, dtype=np.int64)
    out = np.zeros(int(m) + 1, np.int64)
    np.add.at(out, n, counts.astype(np.int64))
    return out
