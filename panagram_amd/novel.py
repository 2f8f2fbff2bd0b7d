"""novel: what a sample holds that no indexed genome does.

The GPU side (``Index.novel``) streams the sample — reads, or an assembly — through the table of every indexed genome's k-mers once;
the windows that MISS it are counted in a key table of the sample's own, which grows while the sample streams (pg_novel.hip:
k_novel_count, k_novel_grow), and one pass over that table (k_novel_scan) gives the distinct novel k-mers, their depth spectrum and
the SOLID ones — those the sample holds at least ``min_count`` times.  For an assembly, k_novel_runs says where the novel k-mers
lie: the maximal runs of novel positions along its contigs.  This module is the host side, plain numpy / pandas: the tables made of
the counts.

``screen``'s ``novel_frac`` counts window instances, every sequencing error among them; ``solid_kmers`` here counts distinct k-mers
at a depth no lone error reaches.  ``min_count`` is the only error filter: an error that recurs ``min_count`` times is solid.

A run of ``kmers`` novel positions from ``start`` spans the bases [start, start + kmers + k - 1); ``bases`` counts those that lie
in novel windows ONLY — a held neighbour's window covers k - 1 of the run's bases on its side:
``bases = max(0, (right_held ? b : b + k - 1) - (left_held ? a + k - 1 : a))`` for the run [a, b): a substitution gives 1, an
insertion of L bases L, the junction of a deletion 0, a wholly novel contig its length."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import pandas as pd

from .place import depth_mode

STAT_NAMES = ["reads", "read_bases", "windows", "hits", "novel_windows", "novel_kmers", "solid_kmers", "solid_windows", "solid_frac",
              "error_windows", "depth_mode", "regions", "region_bases", "min_count"]
SPECTRUM_COLUMNS = ["depth", "kmers"]
KMER_COLUMNS = ["kmer", "depth"]
REGION_COLUMNS = ["file", "contig", "start", "end", "kmers", "bases", "left_held", "right_held"]
BINS = 64                  # the spectrum's depths: bin c = depth c, the last = that depth and beyond
MIN_COUNT_MAX = 0xFFFFFFFF  # a depth is 32 bits
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def default_min_count(any_fastq: bool) -> int:
    """reads: a k-mer seen once may be a sequencing error (2); an assembly: every k-mer counts (1)"""
    return 2 if any_fastq else 1


def check_min_count(min_count) -> int:
    m = int(min_count)
    if not 1 <= m <= MIN_COUNT_MAX:
        raise ValueError(f"novel: min_count={min_count} (1 to 2^32 - 1)")
    return m


def spell(keys, k: int) -> List[str]:
    """the k bases of every key: first base most significant, A < C < G < T"""
    keys = np.asarray(keys, np.uint64).ravel()
    shifts = (2 * np.arange(int(k) - 1, -1, -1)).astype(np.uint64)
    codes = ((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)
    return [row.tobytes().decode("ascii") for row in _ACGT[codes]]


def run_bases(start, end, left_held, right_held, k: int) -> np.ndarray:
    """the bases of the runs [start, end) that lie in novel windows only"""
    a, b = np.asarray(start, np.int64), np.asarray(end, np.int64)
    lh, rh = np.asarray(left_held).astype(bool), np.asarray(right_held).astype(bool)
    return np.maximum(0, np.where(rh, b, b + int(k) - 1) - np.where(lh, a + int(k) - 1, a)).astype(np.int64)


def spectrum_frame(depth_hist) -> pd.DataFrame:
    """SPECTRUM_COLUMNS, one line per depth 1 .. BINS - 1 (the last: that depth and beyond)"""
    h = np.asarray(depth_hist, np.int64).ravel()
    return pd.DataFrame({"depth": np.arange(1, len(h)), "kmers": h[1:]}, columns=SPECTRUM_COLUMNS)


def kmers_frame(keys, depths, k: int) -> pd.DataFrame:
    """KMER_COLUMNS: the k-mers spelled, sorted by key"""
    keys, depths = np.asarray(keys, np.uint64).ravel(), np.asarray(depths, np.int64).ravel()
    order = np.argsort(keys, kind="stable")
    return pd.DataFrame({"kmer": spell(keys[order], k), "depth": depths[order]}, columns=KMER_COLUMNS)


def regions_frame(file: str, names: Sequence[str], run_contig, run_start, run_end, left_held, right_held, k: int) -> pd.DataFrame:
    """REGION_COLUMNS of one file's runs, in (contig, start) order: end = start + kmers + k - 1, the run's last base"""
    c, a, b = np.asarray(run_contig, np.int64), np.asarray(run_start, np.int64), np.asarray(run_end, np.int64)
    names = np.asarray(list(names), object)
    return pd.DataFrame({"file": [str(file)] * len(c), "contig": names[c] if len(c) else np.zeros(0, object), "start": a,
                         "end": b + int(k) - 1, "kmers": b - a, "bases": run_bases(a, b, left_held, right_held, k),
                         "left_held": np.asarray(left_held, np.int64), "right_held": np.asarray(right_held, np.int64)}, columns=REGION_COLUMNS)


def filter_regions(regions: pd.DataFrame, min_bases: int = 0) -> pd.DataFrame:
    """the regions of at least ``min_bases`` bases"""
    if int(min_bases) < 0:
        raise ValueError(f"novel: min_bases={min_bases} must not be negative")
    return regions[regions["bases"] >= int(min_bases)].reset_index(drop=True)


def no_regions() -> pd.DataFrame:
    return regions_frame("", [], *[np.zeros(0, np.int64)] * 5, 1)


def stats(counts: dict, min_count: int, windows: int = 0, hits: int = 0, reads: int = 0, read_bases: int = 0, regions=None) -> dict:
    """STAT_NAMES of a novel table's counts (``engine.NovelTable.result``: nkeys, solid, solid_windows, depth_hist) and of the
    regions kept (None: none asked for).  ``solid_frac = solid_kmers / novel_kmers``, 0 / 0 reads 0; ``error_windows`` = the novel
    windows of k-mers that are not solid; ``depth_mode`` = the most frequent depth at or above ``min_count``."""
    windows, hits = int(windows), int(hits)
    hist = np.asarray(counts["depth_hist"], np.int64).ravel().copy()
    hist[:int(min_count)] = 0  # (the mode of the depths that count as solid)
    nkeys, solid, sw = int(counts["nkeys"]), int(counts["solid"]), int(counts["solid_windows"])
    return {"reads": int(reads), "read_bases": int(read_bases), "windows": windows, "hits": hits, "novel_windows": windows - hits,
            "novel_kmers": nkeys, "solid_kmers": solid, "solid_windows": sw, "solid_frac": solid / nkeys if nkeys else 0.0,
            "error_windows": windows - hits - sw, "depth_mode": depth_mode(hist), "regions": 0 if regions is None else int(len(regions)),
            "region_bases": 0 if regions is None else int(regions["bases"].sum()), "min_count": int(min_count)}


def stat_lines(st: dict) -> List[str]:
    """``name<TAB>value`` per statistic, in STAT_NAMES order: fractions to six places, counts as integers"""
    return [f"{n}\t{st[n]:.6f}" if isinstance(st[n], float) else f"{n}\t{int(st[n])}" for n in STAT_NAMES]


def write_stats(st: dict, out) -> None:
    out.writelines(line + "\n" for line in stat_lines(st))


def write_summary(st: dict, path) -> None:
    with open(path, "w") as f:
        write_stats(st, f)


def write_spectrum(spectrum: pd.DataFrame, path) -> None:
    spectrum.to_csv(path, sep="\t", index=False)


def write_kmers(kmers: pd.DataFrame, path) -> None:
    kmers.to_csv(path, sep="\t", index=False)


def write_regions(regions: pd.DataFrame, path) -> None:
    regions.to_csv(path, sep="\t", index=False)


# ---------------------------------------------------------------------------
# unitigs: the solid novel k-mers compacted into sequences (pg_unitigs.hip; ``engine.NovelTable.unitigs``)
# ---------------------------------------------------------------------------
UNITIG_COLUMNS = ["unitig", "bases", "kmers", "depth", "circular", "sequence"]
UNITIG_STAT_NAMES = ["unitigs", "unitig_bases", "unitig_n50", "longest_unitig", "circular_unitigs"]
FASTA_WIDTH = 80
_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def canonical_unitig(seq: str) -> str:
    """the smaller of a sequence and its reverse complement: what a linear unitig reads as, whichever end its walk began at"""
    rc = seq.translate(_COMPLEMENT)[::-1]
    return min(seq, rc)


def unitigs_frame(offsets, kmers, depth_sum, circular, bases, k: int, min_unitig_bases: int = 0) -> pd.DataFrame:
    """UNITIG_COLUMNS of ``engine.NovelTable.unitigs``' arrays: ``bases`` = kmers + k - 1, ``depth`` = the mean depth of the
    unitig's k-mers to two decimals, linear sequences canonicalised (a circular one starts at its smallest k-mer as it came),
    those of fewer than ``min_unitig_bases`` bases dropped, sorted by (-bases, sequence) and named u1, u2, ... in that order"""
    if int(min_unitig_bases) < 0:
        raise ValueError(f"novel: min_unitig_bases={min_unitig_bases} must not be negative")
    off, n = np.asarray(offsets, np.int64).ravel(), np.asarray(kmers, np.int64).ravel()
    ds, circ = np.asarray(depth_sum, np.uint64).ravel(), np.asarray(circular, np.int64).ravel()
    text = np.asarray(bases, np.uint8).tobytes().decode("ascii")
    length = n + int(k) - 1
    seqs = [text[o:o + l] if c else canonical_unitig(text[o:o + l]) for o, l, c in zip(off.tolist(), length.tolist(), circ.tolist())]
    keep = [i for i in range(len(seqs)) if length[i] >= int(min_unitig_bases)]
    keep.sort(key=lambda i: (-int(length[i]), seqs[i]))
    depth = [round(int(ds[i]) / int(n[i]), 2) for i in keep]
    return pd.DataFrame({"unitig": [f"u{j + 1}" for j in range(len(keep))], "bases": length[keep], "kmers": n[keep],
                         "depth": np.asarray(depth, np.float64), "circular": circ[keep], "sequence": [seqs[i] for i in keep]},
                        columns=UNITIG_COLUMNS)


def unitig_header(row) -> str:
    return f">{row.unitig} bases={int(row.bases)} kmers={int(row.kmers)} depth={float(row.depth):.2f} circular={int(row.circular)}"


def unitig_fasta(frame: pd.DataFrame) -> str:
    """FASTA text: ``>u7 bases=… kmers=… depth=… circular=0|1``, the sequence in lines of FASTA_WIDTH"""
    out = []
    for row in frame.itertuples(index=False):
        out.append(unitig_header(row))
        out.extend(row.sequence[i:i + FASTA_WIDTH] for i in range(0, len(row.sequence), FASTA_WIDTH))
    return "".join(line + "\n" for line in out)


def write_unitigs(frame: pd.DataFrame, path) -> None:
    with open(path, "w") as f:
        f.write(unitig_fasta(frame))


def unitig_stats(frame: pd.DataFrame) -> dict:
    """UNITIG_STAT_NAMES: ``unitig_n50`` = the length L at which the unitigs of at least L bases hold half of all bases or more
    (0: no unitig)"""
    lens = np.sort(np.asarray(frame["bases"], np.int64))[::-1]
    total = int(lens.sum())
    n50 = int(lens[np.searchsorted(np.cumsum(lens), (total + 1) // 2)]) if len(lens) else 0
    return {"unitigs": int(len(lens)), "unitig_bases": total, "unitig_n50": n50, "longest_unitig": int(lens[0]) if len(lens) else 0,
            "circular_unitigs": int(np.asarray(frame["circular"], np.int64).sum())}


def unitig_stat_lines(st: dict) -> List[str]:
    return [f"{n}\t{int(st[n])}" for n in UNITIG_STAT_NAMES]


# cleaning the graph before it is compacted (``engine.NovelTable.clean``): what `novel --unitigs --clean` prints behind the unitig statistics
CLEAN_STAT_NAMES = ["clipped_tips", "clipped_kmers", "popped_bubbles", "popped_kmers", "clean_rounds"]


def clean_options(k: int, tip_kmers=None, bubble_kmers=None, ratio=None, rounds=None) -> dict:
    """the arguments of ``engine.NovelTable.clean`` checked, the defaults filled in (2 k, 2 k, 0.25, 4): ValueError for a k-mer limit
    outside 1 to 1024, a ratio outside (0, 1) or rounds outside 0 to 64"""
    from . import engine
    ratio = 0.25 if ratio is None else float(ratio)
    engine.clean_ratio_milli(ratio)
    return {"tip_kmers": engine.clean_kmers(tip_kmers, k, "tip_kmers"), "bubble_kmers": engine.clean_kmers(bubble_kmers, k, "bubble_kmers"),
            "ratio": ratio, "rounds": engine.clean_rounds(4 if rounds is None else rounds)}


def clean_stat_lines(st: dict) -> List[str]:
    return [f"{n}\t{int(st[n])}" for n in CLEAN_STAT_NAMES]
