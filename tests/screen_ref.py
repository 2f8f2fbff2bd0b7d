"""What pg_screen.hip computes, restated in numpy the obvious way.  The table is a set — ``keys`` (distinct canonical k-mers) and
``M`` (len(keys) x N, 0/1: which genomes hold each), as in tests/kmerstats_ref.py; the sample is a list of sequence sets, each a list
of contigs (ASCII bytes), whose canonical keys come with counts from tests/copies_ref.py (np.unique).  No tests in here:
tests/test_screen_cpu.py ties the restatement to identities that follow by construction and holds the crafted sample to its
promises, tests/test_gpu_screen.py holds the kernels to it.  Oracle side only; never imported by the product.

  valid window   holds no non-ACGT byte; a contig shorter than k has none.  Lower case counts as upper.
  depth(key)     the valid windows of the sample, over every set, whose canonical key is ``key`` — saturating at DEPTH_MAX.
  windows, hits  the valid windows; those whose key the table holds."""
import functools

import numpy as np

from tests import copies_ref as cr
from tests import kmerstats_ref as KR

BINS = 64
DEPTH_MAX = 255
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s: bytes) -> bytes:
    return bytes(s).translate(_COMP)[::-1]


def spell(key: int, k: int) -> bytes:
    """the k bases of a key: first base most significant, A < C < G < T"""
    key = int(key)
    return _ACGT[[(key >> (2 * (k - 1 - i))) & 3 for i in range(k)]].tobytes()


def canonical(seq: bytes, k: int) -> int:
    """the canonical key of a sequence of exactly k ACGT bases"""
    assert len(seq) == k
    return int(cr.valid_keys([seq], k)[0])


def sample_counts(sets, k):
    """(windows, distinct keys [uint64, sorted], their counts [int64]) of the sample: every set's contigs"""
    ks = [cr.valid_keys(contigs, k) for contigs in sets]
    allk = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    u, c = np.unique(allk, return_counts=True)
    return int(len(allk)), u, c.astype(np.int64)


def depths(keys, sets, k):
    """(windows, hits, depth [int64] per table key, saturated)"""
    keys = np.asarray(keys, np.uint64)
    windows, u, c = sample_counts(sets, k)
    d = np.zeros(len(keys), np.int64)
    if len(u) and len(keys):
        at = np.minimum(np.searchsorted(u, keys), len(u) - 1)
        d = np.where(u[at] == keys, c[at], 0).astype(np.int64)
    return windows, int(d.sum()), np.minimum(d, DEPTH_MAX)


def screen(keys, M, depth, min_count) -> dict:
    """the counts of one pass over the table, as engine.TableScreen.result names them"""
    if not 1 <= int(min_count) <= DEPTH_MAX:
        raise ValueError(f"min_count {min_count} (1 to {DEPTH_MAX})")
    M = np.asarray(M, np.int64)
    n = M.shape[1]
    depth = np.asarray(depth, np.int64)
    assert len(keys) == len(M) == len(depth) and len(np.unique(keys)) == len(keys)
    held = M.sum(axis=1)
    got = depth >= int(min_count)
    alone = held == 1
    binned = np.minimum(depth, BINS - 1)
    return dict(distinct=M.sum(axis=0), seen=M[got].sum(axis=0), private=M[alone].sum(axis=0), private_seen=M[alone & got].sum(axis=0),
                occ=np.bincount(held, minlength=n + 1).astype(np.int64), seen_occ=np.bincount(held[got], minlength=n + 1).astype(np.int64),
                depth_hist=np.bincount(binned, minlength=BINS).astype(np.int64),
                core_depth_hist=np.bincount(binned[held == n], minlength=BINS).astype(np.int64), nkeys=int(len(keys)))


def screen_sets(keys, M, sets, k, min_count):
    """(counts, windows, hits) of a sample given as sequence sets"""
    windows, hits, d = depths(keys, sets, k)
    return screen(keys, M, d, min_count), windows, hits


# ---------------------------------------------------------------------------
# the crafted table keys and the crafted sample
# ---------------------------------------------------------------------------
SATELLITE = b"ACG"  # the period-3 satellite: its windows have three canonical keys
HOMOPOLYMER_RUN = 300
SATELLITE_BASES = 200


def special_keys(k):
    """(the homopolymer's key, the satellite's three keys) as the table must hold them for the crafted sample"""
    sat = (SATELLITE * (k // 3 + 2))
    return canonical(b"A" * k, k), sorted({canonical(sat[i:i + k], k) for i in range(3)})


def table_keys(rng, count, k):
    """``count`` distinct table keys: the homopolymer's and the satellite's first, random ones behind"""
    homo, sat = special_keys(k)
    first = np.array([homo] + sat, np.uint64)
    rest = KR.random_keys(rng, count, k)
    rest = rest[~np.isin(rest, first)][:count - len(first)]
    return np.concatenate([first, rest])


def crafted_sample(keys, k, min_count, rng, nplain=400):
    """(sets, promises) — a sample of two sequence sets spelled from the table's ``keys`` (``table_keys``: the special ones first).
    promises: ``below`` / ``at`` — a key at depth min_count - 1 and one at min_count; ``homo`` — the homopolymer's key (a run of
    HOMOPOLYMER_RUN: more than DEPTH_MAX windows on one key, which reads DEPTH_MAX); ``sat`` — the satellite's keys; ``absent`` —
    a key spelled into the sample that the table does not hold; ``short`` / ``exact`` — the contig shorter than k, the one of
    exactly k; ``broken`` — the contig whose windows an N breaks; ``lower`` — a contig in lower case."""
    keys = np.asarray(keys, np.uint64)
    nspecial = 1 + len(special_keys(k)[1])
    plain = keys[nspecial:]
    assert len(plain) >= nplain + 8

    def strand(s):
        return s if rng.random() < 0.5 else revcomp(s)
    below, at, brk, low, exact = (int(x) for x in plain[:5])
    a, b = [], []
    a += [strand(spell(below, k)) for _ in range(min_count - 1)]
    a += [strand(spell(at, k)) for _ in range(min_count - 1)]
    b += [strand(spell(at, k))]  # (the last of them in the second set: a depth that two calls make)
    # a key the table lacks: a random key outside it
    held = set(keys.tolist())
    absent = next(int(x) for x in KR.random_keys(rng, 64, k) if int(x) not in held)
    a += [spell(absent, k), revcomp(spell(absent, k))]
    # windows broken by N: the key's bases, an N in place of one of them, then the whole key behind it
    s = spell(brk, k)
    a += [s[:k // 2] + b"N" + s[k // 2 + 1:] + b"n" + strand(s)]
    short = b"ACGTACG"[:min(k - 1, 7)]
    a += [short, strand(spell(exact, k))]  # shorter than k; exactly k
    a += [strand(spell(low, k)).lower()]
    a += [b"A" * HOMOPOLYMER_RUN if rng.random() < 0.5 else b"T" * HOMOPOLYMER_RUN]
    b += [(SATELLITE * (SATELLITE_BASES // 3 + 1))[:SATELLITE_BASES]]
    # many keys back to back on either strand, a depth of 1 to 3 each (the junctions' windows are mostly no key of the table)
    body = plain[8:8 + nplain]
    for rep in range(3):
        chosen = body[rng.random(len(body)) < (1.0, 0.5, 0.25)[rep]]
        (a if rep != 1 else b).append(b"".join(strand(spell(int(x), k)) for x in rng.permutation(chosen)))
    promises = dict(below=below, at=at, homo=special_keys(k)[0], sat=special_keys(k)[1], absent=absent, short=short,
                    exact=exact, broken=brk, lower=low)
    return [a, b], promises


# ---------------------------------------------------------------------------
# screen end to end: the index and the reads of tests/place_ref.py (A, B, C; the sample a mosaic of B and C)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_table():
    """(keys, M) of the table of all three genomes' k-mers"""
    from oracle import pyoracle as po
    from tests import place_ref as pr
    genomes, _ = pr.e2e_genomes()
    return KR.from_groups(po.build_bitvec_dbs(genomes, pr.E2E["k"]), len(genomes))


@functools.lru_cache(maxsize=None)
def _e2e_reads_depths():
    from tests import place_ref as pr
    return depths(e2e_table()[0], [pr.joined_reads(pr.e2e_reads())], pr.E2E["k"])


def e2e_model(sample, min_count, genomes=None):
    """(main, occupancy, stats) as Index.screen returns them, from the model's counts and panagram_amd.screen.frames.  ``sample``:
    "reads" — place_ref.e2e_reads() — or the contigs of a FASTA"""
    from panagram_amd import screen as scr
    from tests import place_ref as pr
    keys, M = e2e_table()
    k = pr.E2E["k"]
    if isinstance(sample, str):
        assert sample == "reads"
        windows, hits, d = _e2e_reads_depths()
        nreads, bases = len(pr.e2e_reads()), sum(len(r) for r in pr.e2e_reads())
    else:
        windows, hits, d = depths(keys, [list(sample)], k)
        nreads, bases = len(sample), sum(len(c) for c in sample)
    return scr.frames(screen(keys, M, d, min_count), pr.E2E_NAMES, k, min_count, windows, hits, nreads, bases, genomes)
