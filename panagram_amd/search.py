"""Search: which genomes of an index carry a query sequence, and how completely — the host side of ``Index.search`` and the
``search`` subcommand.  No import of the GPU library: numpy and pandas only, so the batching and the frames are tested without a
GPU (tests/test_search_cpu.py).

A query is a FASTA record that is NOT in the index: a gene, a transcript, a marker, a contig of a new assembly.  Its k-mers are
anchored against the table of every sample's k-mers (k_probe), which gives one row of genome bits per k-mer, and the rows are
reduced per query and genome on the GPU (k_presence_profile; include/panagram_hip.h: pg_result_presence_profile) to

    hits     the query's k-mers the genome holds
    runs     the maximal runs of consecutive held k-mers
    longest  the k-mers of the longest run
    first    the first held k-mer, ``end`` one past the last (0, 0 without one)
    covered  the query's bases that lie in at least one held k-mer

``frac = hits / kmers`` drops by k per substituted base; ``cov_frac = covered / length`` drops by one, and reads as an identity.
A k-mer with a non-ACGT base is held by no genome, as everywhere in the project."""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np
import pandas as pd

BATCH_BASES = 1 << 26  # query bases anchored at a time (a longer record is a batch of its own)
FIELDS = ("hits", "runs", "longest", "first", "end", "covered")  # the last axis of a profile array
LONG_COLUMNS = ["query", "length", "kmers", "genome", "hits", "frac", "covered", "cov_frac", "runs", "longest", "first", "end"]
SUMMARY_COLUMNS = ["query", "length", "kmers", "all", "none", "genomes_hit", "best", "best_frac"]
NO_BEST = "-"  # ``best`` of a query no genome holds a k-mer of

_WS = np.zeros(256, bool)
_WS[[32, 9, 10, 11, 12, 13]] = True


def scan_fasta(text) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """(names, lens [n] int64, offs [n + 1] int64) of the records of FASTA ``text`` (bytes or a uint8 array), by
    SeqSet.from_fasta's rules: a line starting with '>' opens a record whose name is the header up to the first white space,
    the other lines are joined with all white space removed, text before the first header is ignored.  Record i is
    ``text[offs[i]:offs[i + 1]]``."""
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
    gt = np.flatnonzero(t == ord(">")).astype(np.int64)
    hdr = gt[(gt == 0) | (t[gt - 1] == ord("\n"))]  # (gt - 1 == -1 only where gt == 0 decides)
    offs = np.append(hdr, len(t)).astype(np.int64)
    if len(hdr) == 0:
        return [], np.zeros(0, np.int64), offs
    nl = np.append(np.flatnonzero(t == ord("\n")), len(t)).astype(np.int64)
    hend = nl[np.searchsorted(nl, hdr)]  # the header line's end: its '\n', or the text's end
    seq = np.concatenate([[0], np.cumsum(~_WS[t], dtype=np.int64)])  # non-white bytes before each position
    lens = seq[offs[1:]] - seq[np.minimum(hend + 1, offs[1:])]
    names = []
    for s, e in zip(hdr, hend):
        words = t[s + 1:e].tobytes().split()
        names.append(words[0].decode("latin-1") if words else "")
    return names, lens.astype(np.int64), offs


def read_queries(queries) -> Tuple[np.ndarray, List[str], np.ndarray, np.ndarray]:
    """(text uint8, names, lens, offs) of ``queries``: a path (plain, or ``.gz`` / ``.bgz`` through gzip), FASTA bytes, or a
    list of (name, sequence) pairs, which are written out as FASTA text.  Records stay in order, duplicate names are kept."""
    if isinstance(queries, (str, os.PathLike)):
        path = os.fspath(queries)
        if path.endswith((".gz", ".bgz")):
            import gzip
            with gzip.open(path, "rb") as f:
                text = np.frombuffer(f.read(), np.uint8)
        else:
            text = np.fromfile(path, np.uint8)
    elif isinstance(queries, (bytes, bytearray, memoryview, np.ndarray)):
        text = np.frombuffer(queries, np.uint8) if not isinstance(queries, np.ndarray) else np.ascontiguousarray(queries, np.uint8)
    else:
        parts = []
        for name, seq in queries:
            name = str(name)
            if not name or name.split() != [name]:
                raise ValueError(f"search: a query name must be one word without white space, got {name!r}")
            seq = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
            if b">" in seq:
                raise ValueError(f"search: the sequence of query {name!r} holds a '>'")
            parts.append(b">" + name.encode("latin-1") + b"\n" + seq + b"\n")
        text = np.frombuffer(b"".join(parts), np.uint8)
    names, lens, offs = scan_fasta(text)
    return text, names, lens, offs


def batches(lens: Sequence[int], batch_bases: int = BATCH_BASES) -> List[Tuple[int, int]]:
    """record ranges [i, j) of at most ``batch_bases`` bases each, cut at record boundaries, in order; a record longer than
    that is a batch of its own.  No record: no batch."""
    if int(batch_bases) < 1:
        raise ValueError(f"search: batch_bases must be at least 1, got {batch_bases}")
    out, i, held = [], 0, 0
    for j, n in enumerate(lens):
        n = int(n)
        if j > i and held + n > batch_bases:
            out.append((i, j))
            i, held = j, 0
        held += n
    if len(lens) > i:
        out.append((i, len(lens)))
    return out


def pick_genomes(all_names: Sequence[str], genomes=None) -> List[int]:
    """the columns of the chosen genomes in the index's order (None: all); KeyError names an unknown one"""
    all_names = list(all_names)
    if genomes is None:
        return list(range(len(all_names)))
    for g in genomes:
        if g not in all_names:
            raise KeyError(f"unknown genome {g!r} (the index has {', '.join(all_names)})")
    chosen = set(genomes)
    return [i for i, g in enumerate(all_names) if g in chosen]


def frames(names: Sequence[str], lens: Sequence[int], k: int, genomes: Sequence[str], profile, rows, min_frac: float = 0.0,
           by: str = "kmers"):
    """(long, matrix, summary) from ``profile`` [queries, genomes, 6] (FIELDS) and ``rows`` [queries, 2] (all, none) over the
    chosen ``genomes``:
    long     one line per query and genome, LONG_COLUMNS: kmers = max(0, length - k + 1), frac = hits / kmers, cov_frac =
             covered / length, both 0 for a query shorter than k; lines whose frac (``by="bases"``: cov_frac) is below ``min_frac``
             are dropped
    matrix   queries x genomes of frac (``by="bases"``: of cov_frac), every query and genome, the index the query names
    summary  one line per query, SUMMARY_COLUMNS: all / none = the query's k-mers that every / no chosen genome holds,
             genomes_hit = the genomes with a hit, best = the genome of the highest matrix value (the first in genome order among
             equals; NO_BEST without a hit) and that value.
    Queries stay in order; duplicate names are kept."""
    if by not in ("kmers", "bases"):
        raise ValueError(f"search: by must be 'kmers' or 'bases', got {by!r}")
    names, genomes = list(names), list(genomes)
    nq, ng = len(names), len(genomes)
    lens = np.asarray(lens, np.int64).reshape(nq)
    profile = np.asarray(profile).astype(np.int64).reshape(nq, ng, len(FIELDS))
    rows = np.asarray(rows).astype(np.int64).reshape(nq, 2)
    kmers = np.maximum(lens - int(k) + 1, 0)
    has = kmers > 0
    f = {name: profile[:, :, i] for i, name in enumerate(FIELDS)}
    frac = np.where(has[:, None], f["hits"] / np.maximum(kmers, 1)[:, None], 0.0)
    cov_frac = np.where(has[:, None], f["covered"] / np.maximum(lens, 1)[:, None], 0.0)
    value = frac if by == "kmers" else cov_frac
    qi = np.repeat(np.arange(nq), ng)
    long = pd.DataFrame({"query": np.array(names, object)[qi] if nq else np.zeros(0, object), "length": lens[qi], "kmers": kmers[qi],
                         "genome": np.tile(np.array(genomes, object), nq) if ng else np.zeros(0, object),
                         "hits": f["hits"].ravel(), "frac": frac.ravel(), "covered": f["covered"].ravel(),
                         "cov_frac": cov_frac.ravel(), "runs": f["runs"].ravel(), "longest": f["longest"].ravel(),
                         "first": f["first"].ravel(), "end": f["end"].ravel()}, columns=LONG_COLUMNS)
    if min_frac > 0:
        long = long[value.ravel() >= min_frac].reset_index(drop=True)
    matrix = pd.DataFrame(value, index=pd.Index(names, name="query", dtype=object), columns=genomes)
    hit = f["hits"] > 0
    nhit = hit.sum(axis=1)
    best_i = value.argmax(axis=1) if ng else np.zeros(nq, np.int64)  # (argmax: the first among equals)
    best = np.where(nhit > 0, np.array(genomes, object)[best_i] if ng else NO_BEST, NO_BEST).astype(object)
    best_frac = np.where(nhit > 0, value[np.arange(nq), best_i] if ng else 0.0, 0.0)
    summary = pd.DataFrame({"query": np.array(names, object) if nq else np.zeros(0, object), "length": lens, "kmers": kmers,
                            "all": rows[:, 0], "none": rows[:, 1], "genomes_hit": nhit, "best": best if nq else np.zeros(0, object),
                            "best_frac": best_frac}, columns=SUMMARY_COLUMNS)
    return long, matrix, summary
