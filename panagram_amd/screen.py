"""screen: which of the indexed genomes a sample holds, and how much of each.

The GPU side (``Index.screen``) streams the sample — reads, or an assembly — through the table of every indexed genome's k-mers and
counts per k-mer how often the sample holds it (pg_screen.hip: k_table_mark), then joins the counts with the presence masks in one
pass over the table (k_table_screen).  A k-mer is SEEN when the sample holds it at least ``min_count`` times.  This module is the
host side, plain numpy / pandas: the tables made of the counts.

Per genome: ``containment = seen / distinct`` (how much of the genome's k-mers the sample recovers), ``identity = containment **
(1 / k)`` (mash screen's estimate), ``private_containment = private_seen / private`` over the k-mers no other genome holds; 0 / 0
reads 0.  Genomes are ranked by containment, ties by private_containment, then by index order.

``novel_frac = 1 - hits / windows`` is taken over window INSTANCES of the sample, not over distinct k-mers: every window that holds
a sequencing error is novel, so reads of a genome that is in the index still show a novel fraction of about 1 - (1 - e) ** k."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import pandas as pd

from .place import depth_mode

MAIN_COLUMNS = ["genome", "distinct", "seen", "containment", "identity", "private", "private_seen", "private_containment", "rank"]
OCCUPANCY_COLUMNS = ["n", "kmers", "seen"]
STAT_NAMES = ["reads", "read_bases", "windows", "hits", "hit_frac", "novel_frac", "nkeys", "keys_seen", "core", "core_seen",
              "core_containment", "depth_mode", "min_count"]
DEPTH_MAX = 255  # the depth of a k-mer saturates there: min_count goes up to it


def default_min_count(any_fastq: bool) -> int:
    """reads: a k-mer seen once may be a sequencing error (2); an assembly: every k-mer counts (1)"""
    return 2 if any_fastq else 1


def check_min_count(min_count) -> int:
    m = int(min_count)
    if not 1 <= m <= DEPTH_MAX:
        raise ValueError(f"screen: min_count={min_count} (1 to {DEPTH_MAX})")
    return m


def pick_genomes(names: Sequence[str], genomes) -> List[int]:
    """the positions of ``genomes`` (names; None: all) in index order"""
    names = list(names)
    if genomes is None:
        return list(range(len(names)))
    for g in genomes:
        if g not in names:
            raise KeyError(f"screen: unknown genome {g!r} (the index has {', '.join(names)})")
    return sorted({names.index(g) for g in genomes})


def ratio(num, den):
    """num / den elementwise; 0 / 0 reads 0"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den > 0)


def ranks(containment, private_containment) -> np.ndarray:
    """rank 1 = the highest containment; ties by private_containment, then by position"""
    c, p = np.asarray(containment, np.float64), np.asarray(private_containment, np.float64)
    order = np.lexsort((np.arange(len(c)), -p, -c))
    out = np.zeros(len(c), np.int64)
    out[order] = np.arange(1, len(c) + 1)
    return out


def frames(counts: dict, names: Sequence[str], k: int, min_count: int, windows: int = 0, hits: int = 0, reads: int = 0, read_bases: int = 0,
           genomes=None):
    """(main, occupancy, stats) of a screen's counts (``engine.TableScreen.result``: distinct, seen, private, private_seen [all
    genomes of the index], occ, seen_occ [genomes + 1], depth_hist, core_depth_hist, nkeys).  main: MAIN_COLUMNS, one line per
    genome in index order, ranked among ALL genomes of the index — ``genomes`` (names; None: all) only selects the lines;
    occupancy: OCCUPANCY_COLUMNS, one line per number of genomes n = 0 .. N; stats: STAT_NAMES."""
    names = list(names)
    N = len(names)
    cols = pick_genomes(names, genomes)
    distinct, seen, priv, pseen = (np.asarray(counts[f], np.int64).reshape(N) for f in ("distinct", "seen", "private", "private_seen"))
    occ, socc = np.asarray(counts["occ"], np.int64).reshape(N + 1), np.asarray(counts["seen_occ"], np.int64).reshape(N + 1)
    cont, pcont = ratio(seen, distinct), ratio(pseen, priv)
    main = pd.DataFrame({"genome": names, "distinct": distinct, "seen": seen, "containment": cont, "identity": cont ** (1.0 / int(k)),
                         "private": priv, "private_seen": pseen, "private_containment": pcont, "rank": ranks(cont, pcont)},
                        columns=MAIN_COLUMNS).iloc[cols].reset_index(drop=True)
    occupancy = pd.DataFrame({"n": np.arange(N + 1), "kmers": occ, "seen": socc}, columns=OCCUPANCY_COLUMNS)
    windows, hits = int(windows), int(hits)
    core_hist = np.asarray(counts["core_depth_hist"], np.int64).ravel().copy()
    core_hist[:int(min_count)] = 0  # (the mode of the depths that count as seen)
    stats = {"reads": int(reads), "read_bases": int(read_bases), "windows": windows, "hits": hits, "hit_frac": float(ratio(hits, windows)),
             "novel_frac": 1.0 - float(ratio(hits, windows)) if windows else 0.0, "nkeys": int(counts["nkeys"]), "keys_seen": int(socc.sum()),
             "core": int(occ[N]), "core_seen": int(socc[N]), "core_containment": float(ratio(socc[N], occ[N])),
             "depth_mode": depth_mode(core_hist), "min_count": int(min_count)}
    return main, occupancy, stats


def summary_comments(stats: dict) -> List[str]:
    """one comment line per statistic, in STAT_NAMES order: fractions to six places, counts as integers"""
    return [f"# {n}\t{stats[n]:.6f}" if isinstance(stats[n], float) else f"# {n}\t{int(stats[n])}" for n in STAT_NAMES]


def write_main(main: pd.DataFrame, out) -> None:
    main.to_csv(out, sep="\t", index=False, float_format="%.6f")


def write_summary(stats: dict, path) -> None:
    with open(path, "w") as f:
        f.writelines(line + "\n" for line in summary_comments(stats))


def write_occupancy(occupancy: pd.DataFrame, path) -> None:
    occupancy.to_csv(path, sep="\t", index=False)
