"""The depths, histograms and tracks pg_copies.hip computes, restated in numpy the obvious way: the canonical keys of every valid
window of a genome, np.unique with counts, and a lookup per position of the targets.  No tests in here:
tests/test_copies_cpu.py ties the restatement to genomes whose depths follow by construction, tests/test_gpu_copies.py holds the
kernels to it.

A sequence set is a list of contigs, each ASCII bytes.  ``depth_G(key)`` = the valid windows of genome G, over all its contigs,
whose canonical key is ``key`` (both strands count through the canonical form); ``d(p)`` of position p of a target contig =
depth_G of its key, the position being invalid when its window holds a non-ACGT byte.  Targets are not deduplicated."""
import numpy as np

from oracle import pyoracle as po

BINS = 64
DEPTH_MAX = 65534
DEPTH_INVALID = 65535


def keys_of(contigs, k):
    """per contig (canonical key of every window [uint64], valid [bool]); a contig shorter than k has no window"""
    out = []
    for seq in contigs:
        if len(seq) < k:
            out.append((np.zeros(0, np.uint64), np.zeros(0, bool)))
            continue
        key, valid = po.canonical_kmers(bytes(seq), k)
        out.append((np.asarray(key, np.uint64), np.asarray(valid, bool)))
    return out


def valid_keys(contigs, k):
    """the keys of the valid windows of all contigs, in position order"""
    ks = [key[valid] for key, valid in keys_of(contigs, k)]
    return np.concatenate(ks) if ks else np.zeros(0, np.uint64)


def distinct(contigs, k) -> int:
    return len(np.unique(valid_keys(contigs, k)))


def depths(targets, genome, k):
    """per target contig (d [int64] of every k-mer position — 0 where invalid —, valid [bool])"""
    u, counts = np.unique(valid_keys(genome, k), return_counts=True)
    out = []
    for key, valid in keys_of(targets, k):
        d = np.zeros(len(key), np.int64)
        if len(u) and len(key):
            at = np.minimum(np.searchsorted(u, key), len(u) - 1)
            d = np.where(valid & (u[at] == key), counts[at], 0).astype(np.int64)
        out.append((d, valid))
    return out


def hits(targets, genome, k) -> int:
    """the valid windows of the genome whose key is one of the targets' keys (what one count adds to a plane's sum)"""
    return int(np.isin(valid_keys(genome, k), np.unique(valid_keys(targets, k))).sum())


def profile(targets, genomes, k):
    """(hist [targets, genomes, BINS] uint64, valid [targets] uint64, track [genomes, all k-mer positions back to back] uint16)"""
    nt = len(targets)
    per = [depths(targets, g, k) for g in genomes]
    hist = np.zeros((nt, len(genomes), BINS), np.uint64)
    valid = np.zeros(nt, np.uint64)
    total = sum(max(0, len(t) - k + 1) for t in targets)
    track = np.zeros((len(genomes), total), np.uint16)
    for gi, dg in enumerate(per):
        at = 0
        for t, (d, v) in enumerate(dg):
            hist[t, gi] = np.bincount(np.minimum(d[v], BINS - 1), minlength=BINS).astype(np.uint64)
            valid[t] = int(v.sum())
            track[gi, at:at + len(d)] = np.where(v, np.minimum(d, DEPTH_MAX), DEPTH_INVALID).astype(np.uint16)
            at += len(d)
    return hist, valid, track
