"""place: which of the indexed genomes an unassembled sample resembles along an anchor genome, bin by bin.

The GPU side (``Index.place``) counts the sample's reads into a count table of the anchor's k-mers and joins that column with the
anchor's bitmap rows (pg_fastq.hip, pg_copies.hip, pg_place.hip); per bin it leaves four counts: ``valid`` rows, ``held`` rows (the
sample holds the k-mer), and per genome ``col`` (the genome holds it) and ``both``.  This module is the host side, plain numpy /
pandas: the FASTQ batches that feed the GPU, and the tables made of the counts.

Per bin and genome: ``jaccard = both / (col + held - both)``, ``cont_g = both / col``, ``cont_s = both / held``; 0 / 0 is NaN."""
from __future__ import annotations

import gzip
import os
from typing import Iterator, List, Optional, Sequence

import numpy as np
import pandas as pd

MAIN_COLUMNS = ["chrom", "start", "end", "valid", "held", "best", "best_jaccard", "second", "second_jaccard"]
SUMMARY_COLUMNS = ["genome", "col", "both", "jaccard", "cont_g", "cont_s", "bins_best"]
DEFAULT_BATCH_BYTES = 256 << 20
NONE = "."  # written for `best` / `second` where no genome has a Jaccard


class FastqBatches:
    """The text of a four-line FASTQ file (plain or ``.gz``) in batches of about ``batch_bytes``, each starting at the first byte
    of a record.  Iterate, and tell ``advance(consumed)`` after every batch how many of its bytes were whole records
    (``SeqSet.from_fastq``'s ``consumed``): the rest is carried in front of the next batch.  At the end of the file a line feed is
    appended if the last line lacks one; bytes that are no whole record even then raise ValueError."""

    def __init__(self, path, batch_bytes: int = DEFAULT_BATCH_BYTES):
        self.path, self.batch_bytes = os.fspath(path), int(batch_bytes)
        if self.batch_bytes < 1:
            raise ValueError(f"batch_bytes must be positive, got {batch_bytes}")
        self._used: Optional[int] = None

    def advance(self, consumed: int) -> None:
        self._used = int(consumed)

    def __iter__(self) -> Iterator[bytes]:
        opener = gzip.open if self.path.endswith((".gz", ".bgz")) else open
        tail = b""
        with opener(self.path, "rb") as f:
            while True:
                chunk = f.read(self.batch_bytes)
                eof = len(chunk) < self.batch_bytes
                buf = tail + chunk
                if eof and buf and not buf.endswith(b"\n"):
                    buf += b"\n"
                if buf:
                    self._used = None
                    yield buf
                    if self._used is None or not 0 <= self._used <= len(buf):
                        raise RuntimeError(f"{self.path}: advance() must follow every batch with a count within it")
                    tail = buf[self._used:]
                if eof:
                    break
        if tail:
            raise ValueError(f"{self.path}: the last {len(tail)} bytes are not a whole FASTQ record (four lines each)")


def ratios(col, both, held):
    """(jaccard, cont_g, cont_s) of counts that broadcast against each other; 0 / 0 is NaN"""
    col, both, held = (np.asarray(x, np.float64) for x in (col, both, held))
    with np.errstate(invalid="ignore", divide="ignore"):
        union = col + held - both
        return (np.where(union > 0, both / union, np.nan), np.where(col > 0, both / col, np.nan),
                np.where(held > 0, both / held, np.nan) + np.zeros_like(col))


def _ranked(jac: np.ndarray, names: Sequence[str]):
    """per row of ``jac``: (best, best value, second, second value) — the highest Jaccard first, ties to the earlier column, NaN
    never ranked; NONE / NaN where there is no such genome"""
    nb, ng = jac.shape
    key = np.where(np.isnan(jac), -np.inf, jac)
    order = np.argsort(-key, axis=1, kind="stable") if ng else np.zeros((nb, 0), np.int64)  # (stable: ties keep column order)
    out = []
    for rank in (0, 1):
        if ng > rank:
            at = order[:, rank]
            v = jac[np.arange(nb), at]
            out += [np.where(np.isnan(v), NONE, np.asarray(list(names), object)[at]), v]
        else:
            out += [np.full(nb, NONE, object), np.full(nb, np.nan)]
    return out


def pick_columns(names: Sequence[str], genomes) -> List[int]:
    """the columns of ``genomes`` (names; None: all) in index order"""
    names = list(names)
    if genomes is None:
        return list(range(len(names)))
    for g in genomes:
        if g not in names:
            raise KeyError(f"place: unknown genome {g!r} (the index has {', '.join(names)})")
    return sorted({names.index(g) for g in genomes})


def frames(bins: pd.DataFrame, valid, held, col, both, names: Sequence[str], genomes=None):
    """(main, matrix, summary) of the bins' counts.  ``bins``: chrom, start, end per bin; ``valid`` / ``held`` [bins], ``col`` /
    ``both`` [bins, all genomes of the index]; ``genomes``: the names that take part (None: all, the anchor's own column included).
    main: MAIN_COLUMNS, one line per bin; matrix: bins x genomes Jaccard, indexed by (chrom, start); summary: SUMMARY_COLUMNS, one
    line per genome, from the sums over all bins."""
    cols = pick_columns(names, genomes)
    chosen = [list(names)[c] for c in cols]
    valid, held = np.asarray(valid, np.int64), np.asarray(held, np.int64)
    col = np.asarray(col, np.int64).reshape(len(valid), len(list(names)))[:, cols]
    both = np.asarray(both, np.int64).reshape(len(valid), len(list(names)))[:, cols]
    jac, _, _ = ratios(col, both, held[:, None])
    best, bj, second, sj = _ranked(jac, chosen)
    main = pd.DataFrame({"chrom": bins["chrom"].to_numpy(), "start": bins["start"].to_numpy(np.int64), "end": bins["end"].to_numpy(np.int64),
                         "valid": valid, "held": held, "best": best, "best_jaccard": bj, "second": second, "second_jaccard": sj},
                        columns=MAIN_COLUMNS)
    matrix = pd.DataFrame(jac, columns=chosen,
                          index=pd.MultiIndex.from_arrays([main["chrom"].to_numpy(), main["start"].to_numpy()], names=["chrom", "start"]))
    tcol, tboth, theld = col.sum(axis=0), both.sum(axis=0), int(held.sum())
    j, cg, cs = ratios(tcol, tboth, theld)
    summary = pd.DataFrame({"genome": chosen, "col": tcol, "both": tboth, "jaccard": j, "cont_g": cg, "cont_s": cs,
                            "bins_best": [int((best == g).sum()) for g in chosen]}, columns=SUMMARY_COLUMNS)
    return main, matrix, summary


def depth_mode(hist) -> int:
    """the most frequent depth >= 1 of a depth histogram [bins] (the lowest such on a tie; 0 when no position has depth >= 1)"""
    h = np.asarray(hist, np.int64).ravel()
    return int(np.argmax(h[1:]) + 1) if len(h) > 1 and h[1:].any() else 0


def summary_comments(stats: dict) -> List[str]:
    """the comment lines in front of --summary: reads, read bases, hits, the depth histogram's mode over bins >= 1, min_count"""
    return [f"# reads\t{int(stats['reads'])}", f"# read_bases\t{int(stats['read_bases'])}", f"# hits\t{int(stats['hits'])}",
            f"# depth_mode\t{int(stats['depth_mode'])}", f"# min_count\t{int(stats['min_count'])}"]


def write_main(main: pd.DataFrame, out) -> None:
    main.to_csv(out, sep="\t", index=False, na_rep="NaN", float_format="%.6f")


def write_matrix(matrix: pd.DataFrame, path) -> None:
    matrix.to_csv(path, sep="\t", na_rep="NaN", float_format="%.6f")


def write_summary(summary: pd.DataFrame, stats: dict, path) -> None:
    with open(path, "w") as f:
        f.writelines(line + "\n" for line in summary_comments(stats))
        summary.to_csv(f, sep="\t", index=False, na_rep="NaN", float_format="%.6f")
