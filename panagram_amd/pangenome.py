"""The pan-genome's own numbers, from the shared distinct k-mer counts the GPU reads off the pan table
(engine.PanTable.kmer_stats: pg_table_pair_counts): how many distinct k-mers each genome holds, how many each pair
shares, how many are core, shell or private — and the exact Jaccard index and mash distance of every pair at the index's
own k, where genome_dist.tsv's default is a MinHash estimate at k = 21.  Plain functions over those arrays: no GPU here."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import pandas as pd

GENOME_COLUMNS = ("kmers", "private", "core", "shell")


def frames(stats: dict, names: Sequence[str]) -> Tuple[pd.DataFrame, pd.DataFrame]:
    """(shared, genomes) of a ``kmer_stats`` dict: ``shared`` the N x N matrix of shared distinct k-mers, rows and columns
    named; ``genomes`` one row per genome — ``kmers`` (its distinct k-mers: the diagonal), ``private`` (held by it alone),
    ``core`` (held by every genome: occupancy[N]) and ``shell`` (the rest: kmers - private - core; with one genome its
    k-mers are core and private at once, and the shell is what is left of ``kmers - core``)."""
    names = [str(n) for n in names]
    n = len(names)
    pairs = np.asarray(stats["pairs"], np.int64)
    occ = np.asarray(stats["occupancy"], np.int64)
    priv = np.asarray(stats["private"], np.int64)
    if pairs.shape != (n, n) or occ.shape != (n + 1,) or priv.shape != (n,):
        raise ValueError(f"kmer_stats of {pairs.shape[0]} genomes given for {n} names")
    shared = pd.DataFrame(pairs, index=pd.Index(names, name="name"), columns=names)
    kmers = np.diagonal(pairs).astype(np.int64)
    core = np.full(n, int(occ[n]), np.int64)
    shell = kmers - core - (priv if n > 1 else 0)
    genomes = pd.DataFrame({"kmers": kmers, "private": priv, "core": core, "shell": shell}, index=pd.Index(names, name="name"),
                           columns=list(GENOME_COLUMNS))
    return shared, genomes


def occupancy_frame(stats: dict) -> pd.DataFrame:
    """columns ``n``, ``kmers``: distinct k-mers held by exactly n genomes, n = 0..N"""
    occ = np.asarray(stats["occupancy"], np.int64)
    return pd.DataFrame({"n": np.arange(len(occ), dtype=np.int64), "kmers": occ})


def exact_distances(pairs, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """(jaccard, distance) of the upper triangle of a shared-k-mer matrix, pairs in sample order ((0,1), (0,2), ..., (1,2),
    ...): j = C[a][b] / (C[a][a] + C[b][b] - C[a][b]) and mash's d = -ln(2j / (1 + j)) / k held to 1, with d = 1 where
    j = 0 and d = 0 where j = 1; a genome without k-mers shares nothing: j = 0."""
    c = np.asarray(pairs, np.int64)
    n = c.shape[0]
    a, b = np.triu_indices(n, 1)
    inter = c[a, b].astype(np.float64)
    union = (c[a, a] + c[b, b] - c[a, b]).astype(np.float64)
    j = np.divide(inter, union, out=np.zeros(len(a), np.float64), where=union > 0)
    d = np.ones(len(a), np.float64)
    mid = (j > 0) & (j < 1)
    d[mid] = np.minimum(1.0, -np.log(2.0 * j[mid] / (1.0 + j[mid])) / k)
    d[j >= 1] = 0.0
    return j, d


def genome_dist_lines(names: Sequence[str], pairs, k: int) -> list:
    """the lines of genome_dist.tsv from exact counts, in the file's five-column layout and pair order: ``name_a, name_b,
    distance, p-value, shared/union`` — the distance the exact one at k, as %.6g; the p-value the literal 0 (nothing was
    sampled); the last column the two counts behind the Jaccard index"""
    names = [str(x) for x in names]
    c = np.asarray(pairs, np.int64)
    if c.shape != (len(names), len(names)):
        raise ValueError(f"a {c.shape} matrix given for {len(names)} names")
    _, d = exact_distances(c, k)
    lines, t = [], 0
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            lines.append(f"{names[i]}\t{names[j]}\t{d[t]:.6g}\t0\t{int(c[i, j])}/{int(c[i, i] + c[j, j] - c[i, j])}\n")
            t += 1
    return lines
