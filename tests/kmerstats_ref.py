"""numpy reference of the pan table's shared distinct k-mer counts (engine.PanTable.kmer_stats): the input is the table as a
set — ``keys`` (distinct canonical k-mers) and ``M`` (len(keys) x N, 0/1: which genomes hold each) — the output what one pass
over it must give.  Oracle side only; never imported by the product."""
from typing import List, Sequence, Tuple

import numpy as np


def stats(keys: np.ndarray, M: np.ndarray) -> dict:
    M = np.asarray(M, np.int64)
    n = M.shape[1]
    assert len(keys) == len(M) and len(np.unique(keys)) == len(keys)
    held = M.sum(axis=1)
    alone = held == 1
    return dict(pairs=M.T @ M, occupancy=np.bincount(held, minlength=n + 1).astype(np.int64),
                private=M[alone].sum(axis=0).astype(np.int64), nkeys=int(len(keys)))


def from_groups(dbs: Sequence[Tuple[np.ndarray, np.ndarray]], ngenomes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(keys, M) of the oracle's ``build_bitvec_dbs`` groups: one (sorted keys, 32-bit masks) pair per 32 genomes"""
    keys = np.unique(np.concatenate([np.asarray(k, np.uint64) for k, _ in dbs])) if dbs else np.zeros(0, np.uint64)
    M = np.zeros((len(keys), ngenomes), np.uint8)
    for d, (k, m) in enumerate(dbs):
        at = np.searchsorted(keys, np.asarray(k, np.uint64))
        width = min(32, ngenomes - 32 * d)
        bits = (np.asarray(m, np.uint32)[:, None] >> np.arange(width, dtype=np.uint32)) & np.uint32(1)
        M[at, 32 * d: 32 * d + width] = bits
    return keys, M


def group_words(M: np.ndarray) -> List[np.ndarray]:
    """the 32-bit mask word of every key for each group of 32 genomes (what PanTable.insert_keys takes, group by group)"""
    M = np.asarray(M, np.uint32)
    out = []
    for g0 in range(0, M.shape[1], 32):
        blk = M[:, g0: g0 + 32]
        out.append((blk << np.arange(blk.shape[1], dtype=np.uint32)).sum(axis=1, dtype=np.uint32))
    return out


def random_keys(rng, count: int, k: int) -> np.ndarray:
    """``count`` distinct canonical k-mers as table keys: the smaller of a k-mer's and its reverse complement's 2k-bit value,
    first base most significant, A < C < G < T"""
    keys = np.zeros(0, np.uint64)
    while len(keys) < count:
        codes = rng.integers(0, 4, (count + count // 8 + 16, k), dtype=np.uint64)
        place = np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64)
        fwd = (codes * place).sum(axis=1, dtype=np.uint64)
        rev = ((np.uint64(3) - codes[:, ::-1]) * place).sum(axis=1, dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, np.minimum(fwd, rev)]))
    return rng.permutation(keys)[:count]
