"""Host side of `synteny`: the runs of unique k-mer matches the GPU returns (engine.synteny_segments: per run the contig of A,
its first k-mer position and exclusive end, and the mate word ``posB << 1 | strand`` of the first position) as a table of
segments with base coordinates on both genomes, and its summary; the blocks the GPU chains from those runs
(engine.synteny_blocks) as the same table with their runs and shifted links, and as PAF lines.  No device code here.

A run of n k-mers covers n + k - 1 bases on either genome.  On strand ``+`` the run's first k-mer lies at ``posB`` and B's range
is ``[posB, posB + n + k - 1)``; on ``-`` the positions of B descend from ``posB``, the range is ``[posB - n + 1, posB + k)``.
Global positions of B become (contig, offset) by a search in the contigs' cumulative lengths: a run never crosses a contig edge
of B, since the last k-mer of one contig and the first of the next lie k bases apart."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import pandas as pd

NO_MATE = 0xFFFFFFFF
COLUMNS = ["chrA", "startA", "endA", "chrB", "startB", "endB", "strand", "kmers"]
BLOCK_COLUMNS = COLUMNS + ["runs", "shifted"]
SUMMARY_COLUMNS = ["chrA", "chrB", "strand", "segments", "kmers"]
TOTALS_COLUMNS = ["side", "genome", "unique", "mated"]
ALL = "*"  # a summary line's chromosome: every chromosome of that side


def contig_offsets(lens: Sequence[int]) -> np.ndarray:
    """[n + 1] int64: the global base offset of every contig of a side, and the side's bases"""
    out = np.zeros(len(lens) + 1, np.int64)
    out[1:] = np.cumsum(np.asarray(lens, np.int64))
    return out


def locate(pos, offsets: np.ndarray):
    """(contig, offset inside it) of global base positions (an empty contig shares its offset with the next one: the search
    from the right lands on the one that holds the base)"""
    pos = np.asarray(pos, np.int64)
    c = np.searchsorted(offsets[:-1], pos, side="right") - 1
    return c, pos - offsets[c]


def segment_frame(run_contig, run_start, run_end, run_mate, k: int, names_a: Sequence[str], lens_b: Sequence[int],
                  names_b: Sequence[str], min_len: int = 1) -> pd.DataFrame:
    """one line per run of at least ``min_len`` k-mers, in the order of the runs: sorted by (contig of A, startA).  Base ranges
    are half-open and ``kmers + k - 1`` long on both genomes."""
    if min_len < 1:
        raise ValueError("min_len must be at least 1")
    c = np.asarray(run_contig, np.int64)
    s, e, m = (np.asarray(x, np.int64) for x in (run_start, run_end, run_mate))
    if not (len(c) == len(s) == len(e) == len(m)):
        raise ValueError("the run arrays differ in length")
    n = e - s
    if len(n) and (n.min() < 1 or (m == NO_MATE).any()):
        raise ValueError("a run without positions or without a mate")
    keep = n >= min_len
    c, s, e, m, n = c[keep], s[keep], e[keep], m[keep], n[keep]
    pos, strand = m >> 1, m & 1
    lo = np.where(strand == 0, pos, pos - (n - 1))
    offs = contig_offsets(lens_b)
    if len(lo) and (lo.min() < 0 or (lo + n + k - 1).max() > offs[-1]):
        raise ValueError("a run outside genome B")
    cb, ob = locate(lo, offs)
    if len(lo) and (ob + n + k - 1 > np.asarray(lens_b, np.int64)[cb]).any():
        raise ValueError("a run across a contig edge of genome B")
    na, nb = np.asarray(list(names_a), object), np.asarray(list(names_b), object)
    return pd.DataFrame({"chrA": na[c] if len(c) else np.zeros(0, object), "startA": s, "endA": e + k - 1,
                         "chrB": nb[cb] if len(c) else np.zeros(0, object), "startB": ob, "endB": ob + n + k - 1,
                         "strand": np.where(strand == 0, "+", "-").astype(object), "kmers": n}, columns=COLUMNS)


def block_frame(blk_contig, blk_start, blk_end, blk_mate_first, blk_mate_last, blk_kmers, blk_runs, blk_shifted, k: int,
                names_a: Sequence[str], lens_b: Sequence[int], names_b: Sequence[str], min_len: int = 1) -> pd.DataFrame:
    """one line per block (engine.synteny_blocks) of at least ``min_len`` k-mers, in the order of the blocks: sorted by (contig of
    A, startA).  Base ranges are half-open: ``endA = end + k - 1``; B's positions are monotone inside a block, so its range is
    ``[mate_first >> 1, (mate_last >> 1) + k)`` on ``+`` and ``[mate_last >> 1, (mate_first >> 1) + k)`` on ``-``.  The two
    ranges differ in length by the insertions and deletions the block bridges."""
    if min_len < 1:
        raise ValueError("min_len must be at least 1")
    cols = [np.asarray(x, np.int64) for x in (blk_contig, blk_start, blk_end, blk_mate_first, blk_mate_last, blk_kmers, blk_runs,
                                              blk_shifted)]
    if len({len(x) for x in cols}) != 1:
        raise ValueError("the block arrays differ in length")
    keep = cols[5] >= min_len
    c, s, e, mf, ml, km, nr, sh = (x[keep] for x in cols)
    if len(c) and ((e <= s).any() or (mf == NO_MATE).any() or (ml == NO_MATE).any() or ((mf ^ ml) & 1).any()):
        raise ValueError("a block without positions, without a mate or of two strands")
    strand = mf & 1
    lo = np.where(strand == 0, mf >> 1, ml >> 1)
    hi = np.where(strand == 0, ml >> 1, mf >> 1) + k
    offs = contig_offsets(lens_b)
    if len(lo) and ((lo > hi - k).any() or lo.min() < 0 or hi.max() > offs[-1]):  # (first k-mer of B behind the last: no block)
        raise ValueError("a block outside genome B")
    cb, ob = locate(lo, offs)
    if len(lo) and (ob + (hi - lo) > np.asarray(lens_b, np.int64)[cb]).any():
        raise ValueError("a block across a contig edge of genome B")
    na, nb = np.asarray(list(names_a), object), np.asarray(list(names_b), object)
    return pd.DataFrame({"chrA": na[c] if len(c) else np.zeros(0, object), "startA": s, "endA": e + k - 1,
                         "chrB": nb[cb] if len(c) else np.zeros(0, object), "startB": ob, "endB": ob + (hi - lo),
                         "strand": np.where(strand == 0, "+", "-").astype(object), "kmers": km, "runs": nr, "shifted": sh},
                        columns=BLOCK_COLUMNS)


def paf_lines(blocks: pd.DataFrame, lens_a, lens_b) -> list:
    """the blocks of ``block_frame`` as PAF lines, query = A, target = B: the 12 mandatory columns — name, length, start, end of
    the query, strand, name, length, start, end of the target, matches = ``kmers``, alignment length = the longer of the two
    ranges, mapping quality 255 (not available) — and the tags ``rn:i:<runs>`` and ``sh:i:<shifted>``.  ``lens_a`` / ``lens_b``:
    chromosome name -> length."""
    out = []
    for r in blocks.itertuples(index=False):
        aln = max(int(r.endA) - int(r.startA), int(r.endB) - int(r.startB))
        out.append("\t".join(str(v) for v in (r.chrA, int(lens_a[r.chrA]), int(r.startA), int(r.endA), r.strand, r.chrB, int(lens_b[r.chrB]),
                                              int(r.startB), int(r.endB), int(r.kmers), aln, 255, f"rn:i:{int(r.runs)}",
                                              f"sh:i:{int(r.shifted)}")))
    return out


def summary_frame(segments: pd.DataFrame) -> pd.DataFrame:
    """the segments and the shared unique k-mers of every (chrA, chrB, strand) that has a segment, in order of first appearance;
    then per side: one line per chromosome of A over all of B (chrB ``*``, strand ``*``), one per chromosome of B over all of A,
    and the total (``* * *``).  With ``min_len`` 1 the total's k-mers are the mated positions of A.  Works on any frame whose
    leading columns are ``segment_frame``'s — ``block_frame``'s too: the count column reads ``segments`` for either kind, and
    counts blocks there."""
    def lines(keys, a, b, strand):
        g = segments.groupby(keys, sort=False)["kmers"].agg(["size", "sum"]).reset_index()
        return pd.DataFrame({"chrA": g["chrA"] if a is None else a, "chrB": g["chrB"] if b is None else b,
                             "strand": g["strand"] if strand is None else strand, "segments": g["size"].astype(np.int64),
                             "kmers": g["sum"].astype(np.int64)}, columns=SUMMARY_COLUMNS)
    total = pd.DataFrame([[ALL, ALL, ALL, len(segments), int(segments["kmers"].sum())]], columns=SUMMARY_COLUMNS)
    if not len(segments):
        return total
    return pd.concat([lines(["chrA", "chrB", "strand"], None, None, None), lines(["chrA"], None, ALL, ALL),
                      lines(["chrB"], ALL, None, ALL), total], ignore_index=True)


def totals_frame(name_a: str, name_b: str, unique_a: int, unique_b: int, mated: int) -> pd.DataFrame:
    """per side: the positions whose k-mer is unique in that genome, and those of them that have a mate in the other — the
    same number on both sides, a mate being a pair"""
    return pd.DataFrame({"side": ["A", "B"], "genome": [name_a, name_b], "unique": [int(unique_a), int(unique_b)],
                         "mated": [int(mated), int(mated)]}, columns=TOTALS_COLUMNS)


def write_summary(path, summary: pd.DataFrame, totals: pd.DataFrame) -> None:
    """the summary table, tab-separated under its header, behind the totals as ``#`` lines (``side genome unique mated``)"""
    with open(path, "w") as f:
        f.write("# " + "\t".join(TOTALS_COLUMNS) + "\n")
        for row in totals.values.tolist():
            f.write("# " + "\t".join(str(v) for v in row) + "\n")
        summary.to_csv(f, sep="\t", index=False)


def chromosome_map(segments: pd.DataFrame) -> pd.DataFrame:
    """which chromosome of B corresponds to each chromosome of A: per chrA the chrB that holds most of its shared unique
    k-mers, with those k-mers, all of chrA's, and the share on strand ``-``.  Takes ``segment_frame``'s lines or
    ``block_frame``'s: it reads ``chrA``, ``chrB``, ``strand`` and ``kmers``."""
    rows = []
    for a, g in segments.groupby("chrA", sort=False):
        per = g.groupby("chrB", sort=False)["kmers"].sum()
        b = per.idxmax()
        best = g[g["chrB"] == b]
        rows.append([a, b, int(per.max()), int(per.sum()), float(best.loc[best["strand"] == "-", "kmers"].sum()) / float(per.max())])
    return pd.DataFrame(rows, columns=["chrA", "chrB", "kmers", "kmers_all", "minus_frac"])


def pick_contigs(names: Sequence[str], chosen) -> list:
    """the indices of the chromosomes ``chosen`` (None: all) in the order of ``names``' sequence set"""
    names = list(names)
    if chosen is None:
        return list(range(len(names)))
    chosen = list(chosen)
    unknown = [c for c in chosen if c not in names]
    if unknown:
        raise ValueError(f"unknown chromosome {unknown[0]!r} (there are {', '.join(map(str, names))})")
    if len(set(chosen)) != len(chosen):
        raise ValueError("a chromosome is named twice")
    want = set(chosen)
    return [i for i, n in enumerate(names) if n in want]
