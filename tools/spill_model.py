#!/usr/bin/env python3
"""CPU model of a pan table's spill — the fraction of keys that do not fit the home line of their minimizer group — by line layout.

    python tools/spill_model.py [--genomes 8] [--mb 2] [--d 0.01] [--k 21] [--points 15:1.19,16:1.19]   (m:keys per line)

numpy only, no GPU: N genomes of `mb` Mb at divergence d (tools/_synth.py), their distinct canonical k-mers, each
key's minimizer (the smallest of its w = k - m + 1 canonical m-mers in a multiplicative order), the group's home line by a hash,
keys / kpl lines.  A line (or half-line) takes its keys up to its capacity and the rest count as spilled: no chain effects — a
spilled key takes no room anywhere else, so the model under-reads dense tables (profiles/bytemask_ab.txt sets it against
pg_table_measure_spill).  Layouts: 8 slots (LAYOUT_SLOTS), two halves of 7 or 8 with the half chosen by the parity of the key or
by one key bit, 16 slots unsplit."""
import argparse

import numpy as np

from _synth import synth_genomes


def canonical_kmers(codes, k):
    """canonical k-mers (first base most significant, the smaller of the two strands) of a contig of 2-bit codes"""
    n = len(codes) - k + 1
    c = codes.astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    for i in range(k):
        fwd = (fwd << np.uint64(2)) | c[i:i + n]
    return np.minimum(fwd, revcomp(fwd, k))


def revcomp(keys, k):
    x = ~keys & np.uint64((1 << (2 * k)) - 1)
    out = np.zeros_like(keys)
    for _ in range(k):
        out = (out << np.uint64(2)) | (x & np.uint64(3))
        x >>= np.uint64(2)
    return out


def groups_of(keys, k, m):
    """minimizer group of every canonical key: min over its w m-mers of the canonical m-mer's scrambled rank"""
    w = k - m + 1
    rc = revcomp(keys, k)
    mm = np.uint64((1 << (2 * m)) - 1)
    best = np.full(len(keys), np.uint64(1 << 62))
    for i in range(w):
        f = (keys >> np.uint64(2 * (k - m - i))) & mm
        r = (rc >> np.uint64(2 * i)) & mm
        c = np.minimum(f, r)
        rank = ((c ^ (c >> np.uint64(32))) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        best = np.minimum(best, rank)
    return best


def mix(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def parity(keys):
    x = keys.copy()
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(s)
    return (x & np.uint64(1)).astype(np.int64)


def spilled(cells, ncells, cap):
    cnt = np.bincount(cells, minlength=ncells)
    return int(np.maximum(cnt - cap, 0).sum())


def model(keys, k, m, kpl):
    nlines = int(len(keys) / kpl) + 1
    with np.errstate(over="ignore"):
        line = (mix(groups_of(keys, k, m)) % np.uint64(nlines)).astype(np.int64)
        par, bit = parity(keys), ((keys >> np.uint64(7)) & np.uint64(1)).astype(np.int64)
    n = float(len(keys))
    return {"8 slots": spilled(line, nlines, 8) / n,
            "2 x 7, parity": spilled(2 * line + par, 2 * nlines, 7) / n,
            "2 x 7, key bit": spilled(2 * line + bit, 2 * nlines, 7) / n,
            "2 x 8, parity": spilled(2 * line + par, 2 * nlines, 8) / n,
            "16 slots": spilled(line, nlines, 16) / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--mb", type=float, default=2.0)
    ap.add_argument("--d", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--points", default="15:1.19,15:2.4,16:1.19,14:1.19", help="m:keys-per-line, comma-separated")
    a = ap.parse_args()
    gen = synth_genomes(a.genomes, [int(a.mb * 1e6)], a.d, a.seed)
    keys = np.unique(np.concatenate([canonical_kmers(c, a.k) for g in gen for c in g]))
    print(f"{a.genomes} x {a.mb:g} Mb, d = {a.d:g}, k = {a.k}: {len(keys)} distinct canonical k-mers")
    pts = [(int(p.split(":")[0]), float(p.split(":")[1])) for p in a.points.split(",")]
    res = [model(keys, a.k, m, kpl) for m, kpl in pts]
    print("layout".ljust(16) + "".join(f"m={m}, kpl {kpl:g}".rjust(18) for m, kpl in pts))
    for name in res[0]:
        print(name.ljust(16) + "".join(f"{r[name]:.3f}".rjust(18) for r in res))


if __name__ == "__main__":
    main()
