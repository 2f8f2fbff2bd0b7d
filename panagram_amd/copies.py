"""Copies: how many copies of a target sequence each genome of an index holds — the host side of ``Index.copies``,
``Genome.gene_copies`` and the ``copies`` subcommand.  No import of the GPU library: numpy and pandas only, so the frames are
tested without a GPU (tests/test_copies_frames_cpu.py).

A target is a sequence that is asked of the genomes' ASSEMBLIES: a gene, a transposon, a marker.  Its canonical k-mers are put
into a count table, every genome is streamed through it (k_copy_count), and per target and genome the depths along the target
are reduced on the GPU to a histogram (k_copy_profile; include/panagram_hip.h: pg_copytable_profile):

    hist[t, g, c]   the valid k-mer positions of target t whose k-mer genome g holds c times (c = 63: 63 times or more)
    valid[t]        the valid positions of target t (a window with a non-ACGT base is none)

``copies`` is the lower median of the depth over a target's valid positions: a copy that diverged shares fewer k-mers, so it is
a lower bound on the size of a family.  Depth is counted per canonical k-mer, on both strands, and says nothing about where the
copies lie."""
from __future__ import annotations

from typing import Iterator, Sequence

import numpy as np
import pandas as pd

BINS = 64
TOP = BINS - 1  # the bin that holds its depth and every depth beyond
DEPTH_INVALID = 0xFFFF
DEPTH_MAX = 0xFFFE
LONG_COLUMNS = ["target", "length", "kmers", "valid", "genome", "present", "frac", "copies", "copies_nz", "mean", "mean_is_lower_bound",
                "max_bin"]
SUMMARY_COLUMNS = ["genome", "targets", "0", "1", "2", "3", "4+"]
TRACK_HEADER = "target\tgenome\tstart\tend\tdepth"


def lower_median(hist) -> np.ndarray:
    """per histogram along the last axis: the smallest bin c with 2 * (hist[0] + ... + hist[c]) >= the histogram's sum — the lower
    median of the binned values; 0 for an empty histogram"""
    h = np.asarray(hist).astype(np.int64)
    cum = np.cumsum(h, axis=-1)
    total = cum[..., -1:]
    return np.where(total[..., 0] > 0, (2 * cum >= total).argmax(axis=-1), 0).astype(np.int64)


def copies_text(c) -> str:
    """a median or bin as it is printed: the last bin is open"""
    return f"{TOP}+" if int(c) >= TOP else str(int(c))


def frames(names: Sequence[str], lens: Sequence[int], k: int, genomes: Sequence[str], hist, valid):
    """(long, matrix, summary) from ``hist`` [targets, genomes, BINS] and ``valid`` [targets] over the chosen ``genomes``:
    long     one line per target and genome, LONG_COLUMNS: kmers = max(0, length - k + 1); present = valid - hist[0] and frac =
             present / valid; copies = the lower median of the depth over the valid positions (``lower_median``), copies_nz the
             same over the positions of depth >= 1; mean = sum of c * hist[c] / valid, a lower bound when hist[63] > 0
             (mean_is_lower_bound); max_bin = the highest bin that is not empty.  ``copies_text`` prints a 63 as ``63+``.
    matrix   targets x genomes of copies, the index the target names
    summary  one line per genome, SUMMARY_COLUMNS: the targets with copies 0, 1, 2, 3, and 4 or more
    A target without a valid position gets zeros and stays in the tables (in the summary it counts under 0).  Targets stay in
    order; duplicate names are kept."""
    names, genomes = list(names), list(genomes)
    nt, ng = len(names), len(genomes)
    lens = np.asarray(lens, np.int64).reshape(nt)
    h = np.asarray(hist).astype(np.int64).reshape(nt, ng, BINS)
    valid = np.asarray(valid).astype(np.int64).reshape(nt)
    if (h.sum(axis=2) != valid[:, None]).any():
        raise ValueError("copies: a histogram does not sum to its target's valid positions")
    kmers = np.maximum(lens - int(k) + 1, 0)
    v = np.repeat(valid[:, None], ng, axis=1)
    present = v - h[:, :, 0]
    frac = np.where(v > 0, present / np.maximum(v, 1), 0.0)
    copies = lower_median(h)
    nz = h.copy()
    nz[:, :, 0] = 0
    copies_nz = lower_median(nz)
    mean = np.where(v > 0, (h * np.arange(BINS)).sum(axis=2) / np.maximum(v, 1), 0.0)
    filled = h > 0
    max_bin = np.where(filled.any(axis=2), BINS - 1 - filled[:, :, ::-1].argmax(axis=2), 0)
    ti = np.repeat(np.arange(nt), ng)
    long = pd.DataFrame({"target": np.array(names, object)[ti] if nt else np.zeros(0, object), "length": lens[ti], "kmers": kmers[ti],
                         "valid": valid[ti], "genome": np.tile(np.array(genomes, object), nt) if ng else np.zeros(0, object),
                         "present": present.ravel(), "frac": frac.ravel(), "copies": copies.ravel(), "copies_nz": copies_nz.ravel(),
                         "mean": mean.ravel(), "mean_is_lower_bound": (h[:, :, TOP] > 0).ravel(), "max_bin": max_bin.ravel()},
                        columns=LONG_COLUMNS)
    matrix = pd.DataFrame(copies, index=pd.Index(names, name="target", dtype=object), columns=genomes)
    cls = np.minimum(copies, 4)
    summary = pd.DataFrame({"genome": np.array(genomes, object) if ng else np.zeros(0, object), "targets": np.full(ng, nt, np.int64),
                            **{c: (cls == i).sum(axis=0).astype(np.int64) for i, c in enumerate(SUMMARY_COLUMNS[2:])}},
                           columns=SUMMARY_COLUMNS)
    return long, matrix, summary


def long_text(long: pd.DataFrame) -> pd.DataFrame:
    """the long table as it is written: copies, copies_nz and max_bin through ``copies_text``, a mean that is a lower bound with
    ``>=`` in front"""
    out = long.copy()
    for c in ("copies", "copies_nz", "max_bin"):
        out[c] = [copies_text(x) for x in long[c]]
    out["mean"] = [(">=" if lb else "") + f"{m:.3f}" for m, lb in zip(long["mean"], long["mean_is_lower_bound"])]
    return out.drop(columns=["mean_is_lower_bound"])


def matrix_text(matrix: pd.DataFrame) -> pd.DataFrame:
    return matrix.apply(lambda col: [copies_text(x) for x in col])


def track_lines(names: Sequence[str], lens: Sequence[int], k: int, genomes: Sequence[str], depths) -> Iterator[str]:
    """per target and genome the maximal runs of equal depth as TSV lines (TRACK_HEADER): [start, end) in k-mer positions of the
    target, the depth — ``65534+`` at the cap, ``.`` over positions whose window holds a non-ACGT base.  ``depths``: [genomes, the
    targets' k-mer positions back to back] as ``CopyTable.profile(track=True)`` returns them."""
    names, genomes = list(names), list(genomes)
    kmers = np.maximum(np.asarray(lens, np.int64) - int(k) + 1, 0)
    koff = np.concatenate([[0], np.cumsum(kmers)])
    d = np.asarray(depths).reshape(len(genomes), int(koff[-1]))
    for t, name in enumerate(names):
        for g, genome in enumerate(genomes):
            row = d[g, koff[t]:koff[t + 1]]
            if not len(row):
                continue
            starts = np.concatenate([[0], np.flatnonzero(row[1:] != row[:-1]) + 1])
            ends = np.concatenate([starts[1:], [len(row)]])
            for s, e in zip(starts, ends):
                x = int(row[s])
                yield f"{name}\t{genome}\t{s}\t{e}\t{'.' if x == DEPTH_INVALID else f'{DEPTH_MAX}+' if x == DEPTH_MAX else x}"


def table_slots(capacity: int) -> int:
    """the slots of a key table made for ``capacity`` keys, as the library sizes it: the power of two at or above twice the
    capacity, two at the least"""
    slots = 2
    while slots < 2 * int(capacity):
        slots *= 2
    return slots


def planes_for(free_bytes: int, slots: int, genomes: int, track_kmers: int = 0) -> int:
    """the planes of one batch of genomes beside a table of ``slots`` slots (``table_slots`` of its keys): what half the free
    memory holds beside the keys (8 bytes a slot; a plane 4, and with a
    track 2 bytes per target position), at least 1 and at most ``genomes``"""
    room = int(free_bytes) // 2 - 8 * int(slots)
    return int(max(1, min(int(genomes), room // max(1, 4 * int(slots) + 2 * int(track_kmers)))))


def gene_names(genes: pd.DataFrame) -> list:
    """``chr:start-end`` of every gene"""
    return [f"{c}:{s}-{e}" for c, s, e in zip(genes["chr"], genes["start"], genes["end"])]
