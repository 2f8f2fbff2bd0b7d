"""Sequence sets of thousands of short contigs, crafted: a fragmented draft assembly has 10^4 to 10^5 scaffolds, a query file
one record per transcript, and everything that is indexed by contig — k_tile0's shares, k_insert_tile's search in tile0,
the tile_contig look-aheads of the epilogues, the (contig, chunk) jobs, k_text_scan's blocks — does its work per contig.
No tests in here: tests/test_many_contigs_cpu.py holds the sets to what is promised below, tests/test_gpu_many_contigs.py
runs the kernels on them.

Contig lengths cycle through classes (``classes``): no k-mer (0, 1, k - 1 bases), a few (k, k + 1), around the rule that a
contig of fewer than 100 k-mers gets one bin per k-mer (k + 98, k + 99, k + 100 bases: 99, 100, 101 k-mers), around the tile
(T - 1, T, T + 1, 2T, 2T + 1, 4T + 1 k-mers) and a handful of LONG ones.  The order is fixed so that a set of at least
MIN_CRAFTED contigs
  starts with HEAD contigs without a k-mer,
  ends with TAIL of them (``ends_empty=False``: on one contig of 99 k-mers behind them),
  holds a run of MIDDLE contigs without a k-mer from contig n // 2 on — longer than any share of k_tile0 at these counts (one
  thread's share is ceil(n / 1024) contigs), so that whole shares sum to 0,
  carries N (a run across a tile edge, a single one) and lower case.
Smaller sets (the first of the regrowth sequence) only cycle through the classes."""
import numpy as np

from oracle import pyoracle as po

COUNTS = (1025, 2049, 3000)   # 1025: the smallest with two contigs per thread of k_tile0; 2049: with three; 3000: the general case
REGROWTH = (10, 1024, 2051)   # contig counts inserted into ONE table in this order: 11, 1025 and 2052 words of tile0
MIN_BASES, MAX_BASES = 150_000, 500_000
MIN_CRAFTED = 64
HEAD, TAIL, MIDDLE = 5, 5, 12
LONG = (5000, 9000, 13000, 17000, 20000)
TILE_EVERY = 32               # one contig in 32 is of a tile class: the bases stay few, the contigs many


def classes(k, tile):
    """name -> the lengths (bases) of the class"""
    return {"none": [0, 1, k - 1], "few": [k, k + 1], "bins": [k + 98, k + 99, k + 100],
            "tiles": [t + k - 1 for t in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 4 * tile + 1)], "long": list(LONG)}


def middle_run(n):
    """(first contig, count) of the run of empty contigs in the middle of a crafted set of n"""
    return n // 2, MIDDLE


def long_places(n):
    return [40 + j * (n - 80) // len(LONG) for j in range(len(LONG))]


def lengths(k, n, seed, tile, ends_empty=True):
    """the n contig lengths, in order"""
    cl = classes(k, tile)
    small = [0, k, 1, k + 98, k - 1, k + 1, k + 99, k + 100]  # (single empty contigs between the others: equal neighbours in tile0)
    if n < MIN_CRAFTED:
        every = [0, k, 1, tile + k, k - 1, k + 98, 2 * tile + k, k + 1, LONG[0], k + 99, k + 100, tile + k - 2, tile + k - 1, 0]
        return np.array([every[i % len(every)] for i in range(n)], np.int64)
    rng = np.random.default_rng(seed)
    lens = np.zeros(n, np.int64)
    j = 0
    for i in range(n):
        if i % TILE_EVERY == TILE_EVERY // 2:
            lens[i] = cl["tiles"][(i // TILE_EVERY) % len(cl["tiles"])]
        else:
            lens[i] = small[j % len(small)]
            j += 1
    for at, ln in zip(long_places(n), LONG):
        lens[at] = ln + int(rng.integers(0, 7))  # (5000 to 20006 bases)
    none = cl["none"]
    lens[:HEAD] = [none[i % 3] for i in range(HEAD)]
    m0, mn = middle_run(n)
    lens[m0:m0 + mn] = [none[i % 3] for i in range(mn)]
    if ends_empty:
        lens[n - TAIL:] = [none[(i + 1) % 3] for i in range(TAIL)]
    else:
        lens[n - TAIL - 1:n - 1] = [none[(i + 1) % 3] for i in range(TAIL)]
        lens[n - 1] = k + 98
    return lens


def marks(lens, k):
    """{contig: what it carries}: "nrun" (45 N across base 2 tile: the first long contig), "n" (one N in the middle: the first
    contig of 101 k-mers and the third long one), "lower" (lower case: the first contig of 100 k-mers and the second long one)"""
    lens = np.asarray(lens)
    long_ones = np.flatnonzero(lens >= LONG[0])
    out = {int(c): what for c, what in zip(long_ones, ("nrun", "lower", "n"))}
    for length, what in ((k + 100, "n"), (k + 99, "lower")):
        at = np.flatnonzero(lens == length)
        if len(at):
            out[int(at[0])] = what
    return out


def fragments(codes, k, n, seed, tile, ends_empty=True):
    """``codes`` (0..3) cut into exactly n contigs (ASCII bytes), back to back from its first base on; ``total_bases`` of them
    are used"""
    lens = lengths(k, n, seed, tile, ends_empty)
    total = int(lens.sum())
    if len(codes) < total:
        raise ValueError(f"{total} bases are needed, {len(codes)} given")
    offs = np.concatenate([[0], np.cumsum(lens)])
    text = po.codes_to_ascii(np.asarray(codes[:total], np.uint8))
    out = [text[offs[i]:offs[i + 1]] for i in range(n)]
    for c, what in marks(lens, k).items():
        s = bytearray(out[c])
        if what == "lower":
            s = bytearray(bytes(s).lower())
        elif what == "nrun" and len(s) > 2 * tile + 40:
            s[2 * tile - 10:2 * tile + 35] = b"N" * 45
        elif what == "n" and len(s) > 4:
            s[len(s) // 2] = ord("N")
        out[c] = bytes(s)
    return out


def total_bases(k, n, seed, tile, ends_empty=True):
    return int(lengths(k, n, seed, tile, ends_empty).sum())


def genomes(ngenomes, k, n, seed, tile, d=0.02, span=0, ends_empty=True):
    """[[contigs of g0: fragmented into n], [g1], ...]: g1.. are diverged copies (po.synth_genomes) of the sequence g0 was cut
    from — whole ones, or with ``span`` > 0 a window of ``span`` bases each, the windows spread evenly over the sequence (wide
    tables: rows of mixed bits everywhere at a fraction of the bases)"""
    total = total_bases(k, n, seed, tile, ends_empty)
    gen = po.synth_genomes(ngenomes, [total], d, seed)
    out = [fragments(gen[0][0], k, n, seed, tile, ends_empty)]
    for g in range(1, ngenomes):
        c = gen[g][0]
        if span and span < total:
            lo = (g - 1) * (total - span) // max(1, ngenomes - 2)
            c = c[lo:lo + span]
        out.append([po.codes_to_ascii(c)])
    return out


def norm(seq):
    """a contig as SeqSet.unpack shows it: upper case, N for every byte outside ACGT"""
    t = np.full(256, ord("N"), np.uint8)
    for c in b"ACGT":
        t[c] = t[c + 32] = c
    return t[np.frombuffer(bytes(seq), np.uint8)].tobytes()


# ---------------------------------------------------------------------------
# FASTA texts
# ---------------------------------------------------------------------------
def names_for(n):
    return [f"ctg{i}" for i in range(n)]


def fasta(contigs, width, crlf=False):
    """po.fasta_text of the contigs (an empty contig is a header alone), lines of ``width``; ``crlf``: CR LF line ends"""
    text = po.fasta_text(names_for(len(contigs)), contigs, width)
    return text.replace(b"\n", b"\r\n") if crlf else text


HEADER_COUNTS = (65535, 65536, 65537)  # around the 1 << 16 header positions SeqSet.from_fasta takes from the device
BIG_TEXT = 4 << 20                     # texts from this size on have their headers looked for on the device
EMPTY_EVERY, GT_EVERY, TWO_LINES_EVERY, DESCRIBED_EVERY = 97, 53, 11, 29


def header_text(nheaders, seed):
    """(text, names, sequences as written): ``nheaders`` records of 44 to 90 bytes, BIG_TEXT bytes at least — every
    EMPTY_EVERY-th record empty, every GT_EVERY-th with a '>' inside a sequence line (not at its start: a base like any other
    non-ACGT byte), every TWO_LINES_EVERY-th on two lines, every DESCRIBED_EVERY-th header with a description; the last record
    without a line end"""
    rng = np.random.default_rng(seed)
    pool = po.codes_to_ascii(rng.integers(0, 4, 1 << 16, dtype=np.uint8))
    sizes = rng.integers(44, 91, nheaders)
    starts = rng.integers(0, len(pool) - 100, nheaders)
    parts, names, seqs = [], [], []
    for i in range(nheaders):
        name = f"r{i}"
        head = b">" + name.encode() + (b" len=" + str(int(sizes[i])).encode() if i % DESCRIBED_EVERY == 3 else b"") + b"\n"
        room = int(sizes[i]) - len(head) - 1
        if i % EMPTY_EVERY == 5:
            seq, body = b"", b""
        else:
            seq = pool[starts[i]:starts[i] + max(4, room)]
            if i % GT_EVERY == 7:
                seq = seq[:3] + b">" + seq[4:]
            if i % TWO_LINES_EVERY == 2:
                cut = len(seq) // 2
                seq = seq[:-1]  # (the second line end takes its byte)
                body = seq[:cut] + b"\n" + seq[cut:] + b"\n"
            else:
                body = seq + b"\n"
        parts.append(head + body)
        names.append(name)
        seqs.append(seq)
    text = b"".join(parts)
    if text.endswith(b"\n") and seqs[-1]:
        text = text[:-1]
    return text, names, seqs


def header_text_picks(text, offs, lens, at_least=2000):
    """the records whose unpacked bases are compared: the first and the last, both neighbours of every empty one, the records
    that straddle a multiple of 4096 bytes of the text, and evenly spaced ones up to ``at_least``"""
    n = len(lens)
    pick = {0, n - 1}
    for e in np.flatnonzero(np.asarray(lens) == 0):
        pick.update(x for x in (int(e) - 1, int(e) + 1) if 0 <= x < n)
    offs = np.asarray(offs, np.int64)
    edges = np.arange(4096, len(text), 4096, dtype=np.int64)
    rec = np.searchsorted(offs, edges, side="right") - 1  # the record that holds byte ``edge``
    inside = (rec >= 0) & (offs[np.maximum(rec, 0)] < edges)   # ... and a byte before it
    pick.update(int(r) for r in rec[inside])
    if len(pick) < at_least:
        pick.update(int(x) for x in np.linspace(0, n - 1, at_least).astype(np.int64))
    return sorted(pick)
