"""numpy / plain-Python restatement of the genome distances panagram_amd writes to genome_dist.tsv (the reference
workflow's `mash sketch -r -s 10000` + `mash triangle -E`, panagram/workflow/Snakefile:124-149): what the GPU sketch,
pg_minhash_distances and Index.write_genome_dist are tested against.  Written from the specification, not from the
product's code:

* the k-mers of a sample: every 21 consecutive ACGT bases (either case) of one record; none spans a record
* canonical k-mer: the lexicographically smaller of the upper-case string and its reverse complement
* hash: h1 of MurmurHash3_x64_128 over the k ASCII bytes of the canonical k-mer, seed 42
* sketch: the s smallest distinct hashes (unsigned), ascending
* a pair: mash's merge (common / denom), distance -ln(2J / (1 + J)) / k, and a binomial p-value

The p-value and the distance use the same scalar arithmetic, in the same order, as the C++ host code, so that the
written file can be predicted byte for byte (both sides call the C library's log / exp / log1p)."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

K, S, SEED = 21, 10000, 42
_M = np.uint64(0xFFFFFFFFFFFFFFFF)
C1, C2 = np.uint64(0x87C37B91114253D5), np.uint64(0x4CF5AD432745937F)


def _rotl(x, r: int):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _fmix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def murmur3_x64_128(msgs: np.ndarray, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(h1, h2) of MurmurHash3_x64_128 for every row of ``msgs`` (n x length uint8; all rows of one length)."""
    msgs = np.ascontiguousarray(msgs, np.uint8)
    n, length = msgs.shape
    with np.errstate(over="ignore"):
        h1 = np.full(n, seed, np.uint64)
        h2 = np.full(n, seed, np.uint64)
        nblocks = length // 16
        words = msgs[:, :16 * nblocks].copy().view("<u8").reshape(n, 2 * nblocks) if nblocks else None
        for b in range(nblocks):
            k1, k2 = words[:, 2 * b].astype(np.uint64), words[:, 2 * b + 1].astype(np.uint64)
            k1 = _rotl(k1 * C1, 31) * C2
            h1 = h1 ^ k1
            h1 = _rotl(h1, 27) + h2
            h1 = h1 * np.uint64(5) + np.uint64(0x52DCE729)
            k2 = _rotl(k2 * C2, 33) * C1
            h2 = h2 ^ k2
            h2 = _rotl(h2, 31) + h1
            h2 = h2 * np.uint64(5) + np.uint64(0x38495AB5)
        tail = msgs[:, 16 * nblocks:]
        k1 = np.zeros(n, np.uint64)
        k2 = np.zeros(n, np.uint64)
        for i in range(tail.shape[1]):
            if i < 8:
                k1 |= tail[:, i].astype(np.uint64) << np.uint64(8 * i)
            else:
                k2 |= tail[:, i].astype(np.uint64) << np.uint64(8 * (i - 8))
        if tail.shape[1] > 8:
            h2 = h2 ^ (_rotl(k2 * C2, 33) * C1)
        if tail.shape[1] > 0:
            h1 = h1 ^ (_rotl(k1 * C1, 31) * C2)
        h1 = h1 ^ np.uint64(length)
        h2 = h2 ^ np.uint64(length)
        h1 = h1 + h2
        h2 = h2 + h1
        h1 = _fmix64(h1)
        h2 = _fmix64(h2)
        h1 = h1 + h2
        h2 = h2 + h1
    return h1, h2


_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i
_ASCII = np.frombuffer(b"ACGT", np.uint8)


def canonical_kmers(seq: bytes, k: int = K) -> np.ndarray:
    """The canonical k-mers of one record as an (n x k) array of upper-case ASCII bytes, in position order; k-mers
    holding a base other than ACGT are left out."""
    codes = _CODE[np.frombuffer(bytes(seq), np.uint8)]
    if len(codes) < k:
        return np.zeros((0, k), np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(codes, k)
    win = win[(win < 4).all(axis=1)].astype(np.uint64)
    rc = np.uint64(3) - win[:, ::-1]
    # strings of one length over A < C < G < T compare like their base-4 values, first base most significant
    place = np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64)
    fwd_first = (win * place).sum(axis=1) <= (rc * place).sum(axis=1)
    canon = np.where(fwd_first[:, None], win, rc)
    return _ASCII[canon.astype(np.intp)]


def kmer_hashes(records: Sequence[bytes], k: int = K, seed: int = SEED) -> np.ndarray:
    """h1 of every canonical k-mer occurrence of a sample (unsorted, with repeats)"""
    parts = [canonical_kmers(r, k) for r in records]
    msgs = np.concatenate(parts) if parts else np.zeros((0, k), np.uint8)
    return murmur3_x64_128(msgs, seed)[0]


def acgt_bases(records: Sequence[bytes]) -> int:
    return int(sum(int((_CODE[np.frombuffer(bytes(r), np.uint8)] < 4).sum()) for r in records))


def sketch(records: Sequence[bytes], s: int = S, k: int = K, seed: int = SEED) -> np.ndarray:
    """the s smallest distinct hashes of a sample, ascending (uint64)"""
    return np.unique(kmer_hashes(records, k, seed))[:s]


def compare(a: np.ndarray, b: np.ndarray, s: int = S) -> Tuple[int, int]:
    """mash's compareSketches merge over two sorted sketches: (common, denom)"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    i = j = common = denom = 0
    while denom < s and i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif a[i] > b[j]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
        denom += 1
    if denom < s:
        denom = min(s, denom + len(a) - i)
        denom = min(s, denom + len(b) - j)
    return common, denom


def distance(common: int, denom: int, k: int = K) -> float:
    if common == 0:
        return 1.0
    if common == denom:
        return 0.0
    j = common / denom
    return min(1.0, -math.log(2.0 * j / (1.0 + j)) / k)


def _log_factorials(n: int) -> List[float]:
    lf = [0.0] * (n + 1)
    for i in range(2, n + 1):
        lf[i] = lf[i - 1] + math.log(float(i))
    return lf


def pvalue(common: int, denom: int, len_a: int, len_b: int, k: int = K, _lf=None) -> float:
    """P[Binomial(denom, r) >= common], r from the two samples' ACGT base counts (mash's model; 1 when nothing is shared)"""
    if common == 0 or denom == 0 or len_a == 0 or len_b == 0:
        return 1.0
    space = float(4 ** k)
    px = 1.0 / (1.0 + space / float(len_a))
    py = 1.0 / (1.0 + space / float(len_b))
    r = px * py / (px + py - px * py)
    if r >= 1.0:
        return 1.0
    n, c = denom, common
    lf = _lf if _lf is not None else _log_factorials(n)
    lr, l1r = math.log(r), math.log1p(-r)
    step = lr - l1r

    def lterm(i):
        return lf[n] - lf[i] - lf[n - i] + float(i) * lr + float(n - i) * l1r

    acc, rel = 1.0, 0.0
    if float(c) > float(n) * r:  # the upper tail's terms fall from i = c on
        i = c
        while i < n:
            rel += math.log(float(n - i) / (float(i) + 1.0)) + step
            t = math.exp(rel)
            acc += t
            i += 1
            if t < 1e-17 * acc:
                break
        p = math.exp(lterm(c)) * acc
    else:  # 1 - P[X <= c - 1]: those terms fall from i = c - 1 down
        i = c - 1
        while i > 0:
            rel += math.log(float(i) / (float(n - i) + 1.0)) - step
            t = math.exp(rel)
            acc += t
            i -= 1
            if t < 1e-17 * acc:
                break
        p = 1.0 - math.exp(lterm(c - 1)) * acc
    return min(1.0, max(0.0, p))


def pairs(sketches: Sequence[np.ndarray], lengths: Sequence[int], s: int = S, k: int = K):
    """[(i, j, distance, p-value, common, denom)] for every i < j, in sample order"""
    lf = _log_factorials(s)
    out = []
    for i in range(len(sketches)):
        for j in range(i + 1, len(sketches)):
            c, d = compare(sketches[i], sketches[j], s)
            out.append((i, j, distance(c, d, k), pvalue(c, d, int(lengths[i]), int(lengths[j]), k, lf), c, d))
    return out


def genome_dist_text(names: Sequence[str], sketches, lengths, s: int = S, k: int = K) -> str:
    """the bytes of genome_dist.tsv: name_a, name_b, distance, p-value, common/denom; numbers as %.6g"""
    return "".join(f"{names[i]}\t{names[j]}\t{d:.6g}\t{p:.6g}\t{c}/{n}\n" for i, j, d, p, c, n in pairs(sketches, lengths, s, k))
