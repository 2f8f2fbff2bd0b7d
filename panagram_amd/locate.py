"""Locate: where each query sequence lies in every genome of an index — chromosome, range, strand, every copy — the host side of
``Index.locate``, ``Genome.gene_loci`` and the ``locate`` subcommand.  No import of the GPU library: numpy and pandas only, so the
frames are tested without a GPU (tests/test_locate_cpu.py).

The queries' k-mers go into a position table as its side 1; every genome's assembly is streamed through it, and the collinear runs
of its hits are chained on the GPU into blocks (k_hit_runs, k_run_blocks; include/panagram_hip.h: pg_postable_locate).  A block is
a locus: a stretch of one chromosome that matches one query on one strand, across substitutions and small insertions and
deletions.  ``synteny.block_frame`` lays the blocks out with A = the genome and B = the queries.

Three limits follow from the rule that a k-mer counts only when it occurs exactly once among the queries:
  - k-mers that repeat among the queries (overlapping genes, family members given as separate queries) count for nothing;
    ``unique`` says how much of a query is left, and ``frac`` is taken of that.
  - a query k-mer that is a repeat in the genome yields many short loci; ``min_kmers`` and ``min_frac`` are the remedy.
  - two queries whose hits interleave on a genome cut each other's chains: a block links a run to the nearest run before it."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import pandas as pd

from . import synteny

LOCI_COLUMNS = ["query", "genome", "chrom", "start", "end", "strand", "qstart", "qend", "kmers", "frac", "runs", "shifted"]
SUMMARY_COLUMNS = ["query", "length", "kmers", "unique", "loci", "genomes_hit", "best_genome", "best_frac"]
NO_BEST = "-"  # ``best_genome`` of a query without a locus


def genome_loci(blocks, k: int, nchroms: int, qlens: Sequence[int]) -> pd.DataFrame:
    """the eight block arrays of one genome (``PosTable.locate``) as ``synteny.block_frame`` lays them out, A the genome and B
    the queries, both numbered: chrA = the chromosome's index, chrB = the query's index among ``qlens`` — half-open base ranges,
    sorted by (chromosome, startA)"""
    return synteny.block_frame(*blocks, int(k), range(int(nchroms)), [int(n) for n in qlens], range(len(qlens)))


def frames(qnames: Sequence[str], qlens: Sequence[int], k: int, unique, genomes: Sequence[str], per_genome, min_kmers: int = 1,
           min_frac: float = 0.0):
    """(loci, matrix, summary) from ``unique`` [queries] — the k-mer positions of every query whose k-mer occurs once among the
    queries — and ``per_genome``: per chosen genome (its chromosomes' names, ``genome_loci``'s frame):
    loci     one line per locus, LOCI_COLUMNS: [start, end) on the chromosome and [qstart, qend) on the query in bases, kmers =
             the matched k-mers, frac = kmers / unique[query], runs and shifted as ``synteny.block_frame``; lines with kmers <
             ``min_kmers`` or frac < ``min_frac`` are dropped.  Sorted by query in file order, genome in the chosen order,
             chromosome in file order, start.
    matrix   queries x genomes: the loci kept, the index the query names
    summary  one line per query, SUMMARY_COLUMNS: kmers = max(0, length - k + 1), loci = all its lines, genomes_hit = the genomes
             with one, best_genome = the genome of its line of highest frac (the first in the table's order among equals;
             ``-`` without a line) and that frac
    A query shorter than k, or without a unique k-mer, stays in matrix and summary with zeros.  Duplicate names are kept; the
    length of every line's query rides in ``loci.attrs["qlen"]`` for ``paf_lines`` (a name does not say which)."""
    qnames, genomes = list(qnames), list(genomes)
    nq, ng = len(qnames), len(genomes)
    qlens = np.asarray(qlens, np.int64).reshape(nq)
    unique = np.asarray(unique).astype(np.int64).reshape(nq)
    if int(min_kmers) < 1:
        raise ValueError("locate: min_kmers must be at least 1")
    if not 0.0 <= float(min_frac) <= 1.0:
        raise ValueError("locate: min_frac is a fraction, 0 to 1")
    if len(per_genome) != ng:
        raise ValueError("locate: one set of blocks per genome")
    parts = []
    for g, (chroms, blk) in enumerate(per_genome):
        q, c = blk["chrB"].to_numpy(np.int64), blk["chrA"].to_numpy(np.int64)
        if len(blk) and (unique[q] < blk["kmers"].to_numpy(np.int64)).any():
            raise ValueError("locate: a locus of more k-mers than its query has unique ones")
        parts.append(pd.DataFrame({"q": q, "g": np.full(len(blk), g, np.int64), "c": c,
                                   "chrom": np.asarray(list(chroms), object)[c] if len(blk) else np.zeros(0, object),
                                   "start": blk["startA"].to_numpy(np.int64), "end": blk["endA"].to_numpy(np.int64),
                                   "strand": blk["strand"].to_numpy(object), "qstart": blk["startB"].to_numpy(np.int64),
                                   "qend": blk["endB"].to_numpy(np.int64), "kmers": blk["kmers"].to_numpy(np.int64),
                                   "runs": blk["runs"].to_numpy(np.int64), "shifted": blk["shifted"].to_numpy(np.int64)}))
    cols = ["q", "g", "c", "chrom", "start", "end", "strand", "qstart", "qend", "kmers", "runs", "shifted"]
    every = pd.concat(parts, ignore_index=True) if parts else pd.DataFrame({c: [] for c in cols})
    every = every.astype({c: np.int64 for c in cols if c not in ("chrom", "strand")})
    every["frac"] = every["kmers"] / np.maximum(unique[every["q"].to_numpy(np.int64)], 1) if len(every) else np.zeros(0)
    every = every[(every["kmers"] >= int(min_kmers)) & (every["frac"] >= float(min_frac))]
    every = every.sort_values(["q", "g", "c", "start"], kind="stable").reset_index(drop=True)
    qi, gi = every["q"].to_numpy(np.int64), every["g"].to_numpy(np.int64)
    empty = np.zeros(0, object)
    loci = pd.DataFrame({"query": np.asarray(qnames, object)[qi] if len(every) else empty,
                         "genome": np.asarray(genomes, object)[gi] if len(every) else empty,
                         **{c: every[c].to_numpy() for c in LOCI_COLUMNS[2:]}}, columns=LOCI_COLUMNS)
    loci.attrs["qlen"] = qlens[qi].tolist()
    counts = np.zeros((nq, ng), np.int64)
    np.add.at(counts, (qi, gi), 1)
    matrix = pd.DataFrame(counts, index=pd.Index(qnames, name="query", dtype=object), columns=genomes)
    best, best_frac = np.full(nq, NO_BEST, object), np.zeros(nq)
    frac = every["frac"].to_numpy(np.float64)
    for i in range(len(every)):  # (the table's order: the first among equals stays)
        if best[qi[i]] == NO_BEST or frac[i] > best_frac[qi[i]]:
            best[qi[i]], best_frac[qi[i]] = genomes[gi[i]], frac[i]
    summary = pd.DataFrame({"query": np.asarray(qnames, object) if nq else empty, "length": qlens, "kmers": np.maximum(qlens - int(k) + 1, 0),
                            "unique": unique, "loci": counts.sum(axis=1), "genomes_hit": (counts > 0).sum(axis=1),
                            "best_genome": best, "best_frac": best_frac}, columns=SUMMARY_COLUMNS)
    return loci, matrix, summary


def paf_lines(loci: pd.DataFrame, chrom_lens) -> list:
    """the loci as PAF lines, query = the query sequence, target = the genome's chromosome: the 12 mandatory columns as
    ``synteny.paf_lines`` builds them — matches = ``kmers``, alignment length = the longer of the two ranges, mapping quality 255
    — and the tags ``rn:i:<runs>``, ``sh:i:<shifted>`` and ``gn:Z:<genome>``.  Takes ``frames``' own table (the queries' lengths ride in its
    attrs); ``chrom_lens``: genome -> chromosome name -> length."""
    qlen = loci.attrs.get("qlen")
    if qlen is None or len(qlen) != len(loci):
        raise ValueError("paf_lines takes frames' own table: the queries' lengths ride in its attrs")
    out = []
    for r, n in zip(loci.itertuples(index=False), qlen):
        aln = max(int(r.end) - int(r.start), int(r.qend) - int(r.qstart))
        out.append("\t".join(str(v) for v in (r.query, int(n), int(r.qstart), int(r.qend), r.strand, r.chrom,
                                              int(chrom_lens[r.genome][r.chrom]), int(r.start), int(r.end), int(r.kmers), aln, 255,
                                              f"rn:i:{int(r.runs)}", f"sh:i:{int(r.shifted)}", f"gn:Z:{r.genome}")))
    return out
