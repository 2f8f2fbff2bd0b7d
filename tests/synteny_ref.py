"""The mates and runs pg_synteny.hip computes, restated in numpy the obvious way: canonical keys of every window of both sides,
np.unique with counts per side, the mate word of every position of A, and np.diff per contig for the runs.  No tests in here:
tests/test_synteny_cpu.py ties the restatement to cases whose segments follow by construction, tests/test_gpu_synteny.py holds
the kernels to it.

A side is a list of contigs, each ASCII bytes.  A k-mer's position is the global base offset of its first base in the
concatenation of its side's contigs; its word is ``pos << 1 | rc`` with rc = 1 when the forward value is greater than the
reverse complement's; the mate of a position of A whose key is unique in both sides is ``posB << 1 | (rcA ^ rcB)``."""
import numpy as np

from oracle import pyoracle as po

NO_MATE = 0xFFFFFFFF


def forward_values(seq: bytes, k: int) -> np.ndarray:
    """value(forward strand) of every window, first base most significant (0 where the window is not valid: unused)"""
    codes = po.encode(bytes(seq))
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    c = np.where(codes == 255, 0, codes).astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    for j in range(k):
        fwd |= c[j:j + n] << np.uint64(2 * (k - 1 - j))
    return fwd


def side_kmers(contigs, k):
    """(keys, rc, pos) of the VALID windows of a side in position order, and the k-mer positions per contig (valid or not)"""
    keys, rcs, poss, nk = [], [], [], []
    off = 0
    for seq in contigs:
        key, valid = po.canonical_kmers(bytes(seq), k)
        rc = forward_values(seq, k) > key
        p = off + np.arange(len(key), dtype=np.int64)
        keys.append(key[valid])
        rcs.append(rc[valid].astype(np.int64))
        poss.append(p[valid])
        nk.append(len(key))
        off += len(seq)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return cat(keys, np.uint64), cat(rcs, np.int64), cat(poss, np.int64), nk


def unique_of(keys):
    """the keys that occur exactly once, sorted, and for each the index of its one occurrence"""
    u, first, counts = np.unique(keys, return_index=True, return_counts=True)
    return u[counts == 1], first[counts == 1]


def mates(contigs_a, contigs_b, k):
    """(mate word of every k-mer position of A, contigs back to back [uint32]; k-mer positions per contig of A)"""
    ka, rca, pa, nk = side_kmers(contigs_a, k)
    kb, rcb, pb, _ = side_kmers(contigs_b, k)
    out = np.full(int(sum(nk)), NO_MATE, np.int64)
    ua, ia = unique_of(ka)
    ub, ib = unique_of(kb)
    both, xa, xb = np.intersect1d(ua, ub, assume_unique=True, return_indices=True)
    ia, ib = ia[xa], ib[xb]
    # the index of A's position in the back-to-back array: its global base offset less (k - 1) per earlier contig that has k-mers
    starts = np.concatenate([[0], np.cumsum([len(s) for s in contigs_a])])[:-1]
    koff = np.concatenate([[0], np.cumsum(nk)])[:-1]
    contig = np.searchsorted(starts, pa[ia], side="right") - 1
    # (empty contigs share their start with the next one: side="right" lands on the last of them, the one that holds the base)
    idx = koff[contig] + (pa[ia] - starts[contig])
    out[idx] = (pb[ib] << 1) | (rca[ia] ^ rcb[ib])
    return out.astype(np.uint32), nk


def runs(mate_words, nkmers):
    """[n, 4] int64 = (contig, start, end, mate word of the start) of the maximal collinear runs, sorted by (contig, start)"""
    out = []
    off = 0
    for c, n in enumerate(nkmers):
        m = np.asarray(mate_words[off:off + n]).astype(np.int64)
        off += n
        if n == 0:
            continue
        mated = m != NO_MATE
        cont = np.zeros(n, bool)
        step = np.where(m & 1, -2, 2)
        cont[1:] = mated[1:] & mated[:-1] & (np.diff(m) == step[1:])
        before = np.concatenate([[False], mated[:-1]])
        s = np.flatnonzero(mated & ~cont)
        e = np.flatnonzero(before & ~cont)
        if mated[-1]:
            e = np.append(e, n)
        assert len(s) == len(e) and (s < e).all()
        out.append(np.stack([np.full(len(s), c, np.int64), s, e, m[s]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


def segments(contigs_a, contigs_b, k):
    """(runs [n, 4], mated positions of A)"""
    m, nk = mates(contigs_a, contigs_b, k)
    return runs(m, nk), int((m != NO_MATE).sum())


def segment_rows(run_rows, k, names_a, lens_b, names_b, min_len=1):
    """the segment table, one tuple (chrA, startA, endA, chrB, startB, endB, strand, kmers) per run, by a plain loop"""
    out = []
    offs = [0]
    for n in lens_b:
        offs.append(offs[-1] + int(n))
    for c, s, e, m in np.asarray(run_rows).tolist():
        n, pos, strand = e - s, m >> 1, m & 1
        if n < min_len:
            continue
        lo = pos if strand == 0 else pos - (n - 1)
        cb = max(i for i in range(len(lens_b)) if offs[i] <= lo and lens_b[i] > 0)
        out.append((names_a[c], s, e + k - 1, names_b[cb], lo - offs[cb], lo - offs[cb] + n + k - 1, "+-"[strand], n))
    return out


# ---------------------------------------------------------------------------
# planters, on code arrays 0..3
# ---------------------------------------------------------------------------
def revcomp(codes):
    return (3 - np.asarray(codes, np.uint8)[::-1]).astype(np.uint8)


def ascii_of(codes) -> bytes:
    return po.codes_to_ascii(np.asarray(codes, np.uint8))


def plant_inversion(codes, a, b):
    """bases [a, b) replaced by their reverse complement"""
    return np.concatenate([codes[:a], revcomp(codes[a:b]), codes[b:]])


def plant_translocation(contigs, src, a, b, dst, at):
    """bases [a, b) of contig src cut out and put in front of base ``at`` of contig dst (another contig)"""
    assert src != dst
    out = [np.asarray(c, np.uint8) for c in contigs]
    block = out[src][a:b]
    out[src] = np.concatenate([out[src][:a], out[src][b:]])
    out[dst] = np.concatenate([out[dst][:at], block, out[dst][at:]])
    return out


def plant_tandem_duplication(codes, a, b):
    """bases [a, b) twice in a row"""
    return np.concatenate([codes[:b], codes[a:b], codes[b:]])


def plant_snps(codes, positions):
    out = np.array(codes, np.uint8)
    for p in positions:
        out[p] = (out[p] + 1) & 3
    return out


def random_codes(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)


# ---------------------------------------------------------------------------
# the planted rearrangements, shared by tests/test_synteny_cpu.py, tests/test_gpu_synteny.py and tests/test_gpu_synteny_e2e.py
# ---------------------------------------------------------------------------
PLANTED_K = 15


def planted_contigs():
    """two random contigs of 900 and 700 bases whose bases at the breakpoints below are set so that no k-mer spanning a
    breakpoint survives a rearrangement by chance (callers assert that all their k-mers are distinct)"""
    x, y = random_codes(900, 9), random_codes(700, 10)
    x[199], x[499], y[299] = 0, 1, 2  # the base in front of every junction of the translocation ...
    x[200], x[500], y[300] = 0, 1, 2  # ... and the one behind it: the three differ
    y[100] = y[139] = 0               # just inside the inversion's breakpoints: A <-> T
    return x, y


def planted_rearranged(x, y):
    """bases [200, 500) of x moved in front of base 300 of y, and bases [100, 140) of y inverted"""
    return plant_translocation([x, plant_inversion(y, 100, 140)], 0, 200, 500, 1, 300)
