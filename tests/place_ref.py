"""What pg_fastq.hip and pg_place.hip compute, and what `place` makes of it, restated the obvious way: Python's split for the FASTQ
text, np.unique over the reads' windows for the sample's depths, boolean masks for the four counts.  No tests in here:
tests/test_place_cpu.py ties the restatement to the oracle's rows and checks that the crafted cases hold what they promise,
tests/test_gpu_fastq.py, test_gpu_sample_agree.py and test_gpu_place_e2e.py hold the kernels and the command to it.

FASTQ (four lines per record; only the line count decides what a line is):
  nreads    = (line feeds in the text) // 4;  consumed = the offset just past line feed 4 * nreads
  joined    = b"N".join(sequence lines of the complete records, each without one trailing "\\r")
  malformed = a complete record whose line 0 does not begin with "@" or whose line 2 does not begin with "+"

sample_agree, for a window = rows [s, e) of contig c, row r being the k-mer at bases [r, r + k) of contig c of the anchor:
  valid row    that window of the anchor holds no non-ACGT base
  s(r)         the reads' valid windows with the row's canonical key number at least min_count (both strands through the key)
  valid, held  the valid rows, the valid rows with s(r);  col[g], both[g]  the valid rows with bit g, with bit g and s(r)"""
import functools
import gzip
import os

import numpy as np
import pandas as pd

from tests import copies_ref as cr
from tests import rows_craft as rc

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def rand(rng, n):
    return bytes(ACGT[rng.integers(0, 4, n)])


# ---------------------------------------------------------------------------
# FASTQ
# ---------------------------------------------------------------------------
def fastq_model(text):
    """(joined, nreads, consumed)"""
    text = bytes(text)
    nreads = text.count(b"\n") // 4
    lines = text.split(b"\n")[:4 * nreads]
    consumed = sum(len(line) + 1 for line in lines)
    return b"N".join(line[:-1] if line.endswith(b"\r") else line for line in lines[1::4]), nreads, consumed


def fastq_malformed(text):
    """the numbers of the malformed complete records"""
    text = bytes(text)
    lines = text.split(b"\n")[:4 * (text.count(b"\n") // 4)]
    return [r for r in range(len(lines) // 4) if not lines[4 * r].startswith(b"@") or not lines[4 * r + 2].startswith(b"+")]


def as_packed(seq):
    """a sequence as a packed seqset gives it back: lower case folded, every byte outside ACGT an N"""
    a = np.frombuffer(bytes(seq), np.uint8) & 0xDF
    return np.where(np.isin(a, ACGT), a, ord("N")).astype(np.uint8).tobytes()


def fastq_text(reads, eol=b"\n", quals=None, names=None):
    """four-line records of the sequences ``reads``; quals[i] / names[i] replace the default quality line / name"""
    out = []
    for i, r in enumerate(reads):
        q = quals[i] if quals and quals.get(i) is not None else b"I" * len(r)
        n = names[i] if names and names.get(i) is not None else b"r%d" % i
        out.append(b"@" + n + eol + bytes(r) + eol + b"+" + eol + q + eol)
    return b"".join(out)


FASTQ_K = 21
FASTQ_TILE = 4096  # bytes of text per workgroup (engine.FASTQ_TILE; tests/test_place_cpu.py holds the two together)


def fastq_texts():
    """{name: text}: the texts tests/test_gpu_fastq.py joins on the GPU (every one well-formed)"""
    rng = np.random.default_rng(77)
    k, T = FASTQ_K, FASTQ_TILE
    some = [rand(rng, int(n)) for n in rng.integers(30, 160, 40)]
    t = {}
    t["lf"] = fastq_text(some)
    t["crlf"] = fastq_text(some, eol=b"\r\n")
    t["no_final_lf"] = fastq_text(some)[:-1]                       # the last record is torn: consumed stops before it
    t["qual_at_plus"] = fastq_text(some[:6], quals={0: b"@" * len(some[0]), 1: b"+" * len(some[1]), 2: b"@+" + b"I" * (len(some[2]) - 2),
                                                    4: b"+@" + b"#" * (len(some[4]) - 2)})
    t["short_reads"] = fastq_text([some[0], b"", some[1], b"A", rand(rng, k - 1), rand(rng, k), b"", b"", some[2], b""])
    t["empty_first"] = fastq_text([b"", some[3]])
    t["all_empty"] = fastq_text([b"", b"", b""])
    t["alphabet"] = fastq_text([b"acgtACGTnNrRyYkKmMsSwWbBdDhHvV", some[4].lower(), b"ACGT.-*ACGT", b"NNNN" + some[5] + b"N"])
    t["cr_inside"] = fastq_text([b"AC\rGT", b"ACGT\r", some[6]], eol=b"\r\n")  # (only the "\r" right before the line feed goes)
    t["one_record"] = fastq_text(some[:1])
    t["zero_bytes"] = b""
    t["only_line_feeds"] = b"\n\n\n"
    # sequence lines whose last base / line feed falls at the tile's size - 1, + 0, + 1: header "@a\n" is 3 bytes
    for d in (-1, 0, 1):
        t[f"tile_edge{d:+d}"] = fastq_text([rand(rng, T - 3 + d), some[7], rand(rng, 2 * T - 3 + d)], names={0: b"a", 2: b"b"})
    t["long_read"] = fastq_text([some[8], rand(rng, 100_000), some[9]])
    t["many_short"] = fastq_text([rand(rng, 3) for _ in range(70_000)])
    whole = fastq_text(some[:5])
    r3 = len(fastq_text(some[:3]))  # records 0..2 complete; the cut falls in each of record 3's four lines
    hdr, seq = len(b"@r3\n"), len(some[3]) + 1
    for name, cut in (("cut_line0", r3 + 2), ("cut_line1", r3 + hdr + 10), ("cut_line2", r3 + hdr + seq + 1),
                      ("cut_line3", r3 + hdr + seq + 2 + 7), ("cut_after_line2", r3 + hdr + seq + 2)):
        t[name] = whole[:cut]
    return t


def fastq_malformed_texts():
    """{name: (text, the malformed records)}"""
    rng = np.random.default_rng(78)
    some = [rand(rng, 50) for _ in range(200)]
    good = fastq_text(some)
    t = {}
    t["no_at"] = good.replace(b"@r150\n", b"r150\n", 1)
    t["no_plus"] = good.replace(b"\n+\n", b"\n-\n", 1)
    t["empty_header"] = fastq_text(some[:3]) + b"\n" + some[3] + b"\n+\n" + b"I" * 50 + b"\n"
    t["shifted"] = good[good.index(b"\n") + 1:]  # (the first line lost: every record reads a sequence as its header)
    return {n: (x, fastq_malformed(x)) for n, x in t.items()}


# ---------------------------------------------------------------------------
# sample_agree
# ---------------------------------------------------------------------------
def sample_depths(anchor, reads, k):
    """per anchor contig (depth [int64] of every row — 0 where invalid —, valid [bool]); ``reads``: the contigs of the read set"""
    return cr.depths(anchor, reads, k)


def agree(depths, rows, n, min_count, contigs, starts, ends):
    """(valid, held [windows], col, both [windows, N]) uint64 — straight from the definitions"""
    nw = len(contigs)
    valid, held = np.zeros(nw, np.uint64), np.zeros(nw, np.uint64)
    col, both = np.zeros((nw, n), np.uint64), np.zeros((nw, n), np.uint64)
    for i, (c, s, e) in enumerate(zip(contigs, starts, ends)):
        c, s, e = int(c), int(s), int(e)
        d, v = depths[c]
        v = v[s:e]
        samp = v & (d[s:e] >= min_count)
        bits = rc.unpack(rows[c][s:e], n).astype(bool)
        valid[i], held[i] = v.sum(), samp.sum()
        col[i], both[i] = bits[v].sum(axis=0), bits[samp].sum(axis=0)
    return valid, held, col, both


AGREE_K = [6, 21, 31, 32]
AGREE_N = [1, 8, 9, 32, 33, 64, 65, 128, 129, 257, 512]
AGREE_MIN_COUNTS = [1, 2, 5]
DEEP = 70_000
CHUNK = 4096  # rows per workgroup of k_sample_agree (engine.PLACE_CHUNK)


def agree_case(k):
    """A crafted anchor, read set and windows for one k.  Returns dict(anchor=[three contigs: long, shorter than k, medium],
    reads=[the read set's contigs], windows=(contigs, starts, ends), special={name: (contig, row)}).

    The anchor's first contig: random, then planted, in order, P the reverse-complement palindrome (even k), a segment DUP that occurs
    again further on, and its reverse complement later still, two bases outside ACGT (an N and an R) that invalidate 2 k - 1 or
    fewer rows each, and lower-case bases (valid).  The reads: random pieces of the anchor of k to 3 k bases — few of them for k
    = 6, where every key occurs all over the anchor — then, as reads of exactly k bases, the k-mer at d0..d5 0, 1, 2, 4, 5 and DEEP
    times (depths min_count - 1 and min_count for min_count 1, 2 and 5), the k-mer at `rc_only` only as its reverse complement, the
    palindrome three times, the k-mer of DUP twice.  `never`: a row whose key no read holds."""
    rng = np.random.default_rng(1000 + k)
    n0 = 2 * CHUNK + 300 + k - 1          # rows: two whole chunks and 300
    a0 = bytearray(rand(rng, n0))
    half = k // 2
    pal = rand(rng, half)
    pal = pal + revcomp(pal) if k % 2 == 0 else None
    at = dict(pal=500, dup=900, dup2=5000, dup_rc=7000, d0=1500, d1=1600, d2=1700, d3=1800, d4=1900, d5=2000, rc_only=2200, never=2400)
    if pal:
        a0[at["pal"]:at["pal"] + k] = pal
    dup = bytes(a0[at["dup"]:at["dup"] + k])
    a0[at["dup2"]:at["dup2"] + k] = dup
    a0[at["dup_rc"]:at["dup_rc"] + k] = revcomp(dup)
    a0[3000] = ord("N")
    a0[CHUNK - 3] = ord("R")                # (invalid rows on both sides of a chunk edge)
    a0[6000:6200] = bytes(a0[6000:6200]).lower()
    a2 = bytearray(rand(rng, 700 + k - 1))
    a2[100] = ord("n")
    anchor = [bytes(a0), rand(rng, k - 1), bytes(a2)]
    special = {name: (0, p) for name, p in at.items() if name != "pal" or pal}
    keep_out = sorted(p for name, p in at.items() if name.startswith("d") and len(name) == 2 or name in ("rc_only", "never"))
    reads = []
    for _ in range(40 if k == 6 else 700):
        c = 0 if rng.random() < 0.8 else 2
        ln = int(rng.integers(k, 3 * k + 1))
        s = int(rng.integers(0, len(anchor[c]) - ln + 1))
        if c == 0 and any(s - k < p < s + ln for p in keep_out):
            continue  # (the rows with a planted depth stay clear of the random pieces)
        piece = anchor[c][s:s + ln]
        reads += [piece if rng.random() < 0.5 else revcomp(piece)] * int(rng.integers(1, 7))
    kmer = lambda p: bytes(a0[p:p + k])
    for name, depth in (("d0", 0), ("d1", 1), ("d2", 2), ("d3", 4), ("d4", 5), ("d5", DEEP)):
        reads += [kmer(at[name]) if i % 2 else revcomp(kmer(at[name])) for i in range(depth)]
    reads += [revcomp(kmer(at["rc_only"]))] * 3
    if pal:
        reads += [pal] * 3
    reads += [dup, revcomp(dup)]
    nk = [len(a) - k + 1 if len(a) >= k else 0 for a in anchor]
    w = [(0, 0, 0), (0, 7, 7), (0, 1500, 1501), (0, 3, 3 + CHUNK - 1), (0, 5, 5 + CHUNK), (0, 2, 2 + CHUNK + 1), (0, nk[0] - 200, nk[0]),
         (0, 1000, 6000), (0, 4000, 7500), (0, 0, nk[0]), (2, 0, nk[2]), (2, 50, 150), (2, nk[2] - 1, nk[2]), (1, 0, 0), (0, 1400, 2500)]
    c, s, e = (np.array(x) for x in zip(*w))
    return dict(anchor=anchor, reads=reads, windows=(c.astype(np.uint32), s.astype(np.uint64), e.astype(np.uint64)), special=special,
                nkmers=nk)


def joined_reads(reads):
    """the read set as pg_seqset_from_fastq leaves it: one contig"""
    return [b"N".join(reads)]


def agree_rows(nk, n, seed=0):
    """dense rows per contig with the bits past N set (they never count)"""
    return [rc.with_pad_bits(rc.dense(m, n, 100 + seed + i), n) for i, m in enumerate(nk)]


# ---------------------------------------------------------------------------
# place end to end: a planted mosaic sample
# ---------------------------------------------------------------------------
E2E = dict(k=21, bin_size=5000, contig_lens=(30000, 25000, 5000), divergence=0.01, private=0.002, read_len=100, coverage=12, error=0.005,
           min_count=2, seed=2026)
E2E_NAMES = ["A", "B", "C"]
E2E_CHROMS = ["chr1", "chr2", "chr3"]


def _substitute(rng, seq, rate):
    a = np.frombuffer(bytes(seq), np.uint8).copy()
    hit = np.flatnonzero(rng.random(len(a)) < rate)
    code = np.searchsorted(ACGT, a[hit])
    a[hit] = ACGT[(code + rng.integers(1, 4, len(hit))) % 4]
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def e2e_genomes():
    """([A, B, C] — each its three contigs —, the sample's contigs): B and C are A with independent substitutions; the sample holds
    B's sequence on the first half of each of the two long contigs and C's on the second half (the short contig: B's), with
    private substitutions of its own"""
    p = E2E
    rng = np.random.default_rng(p["seed"])
    A = [rand(rng, n) for n in p["contig_lens"]]
    B = [_substitute(rng, c, p["divergence"]) for c in A]
    C = [_substitute(rng, c, p["divergence"]) for c in A]
    sample = []
    for i, n in enumerate(p["contig_lens"]):
        h = n // 2 if i < 2 else n
        sample.append(_substitute(rng, B[i][:h] + C[i][h:], p["private"]))
    return [A, B, C], sample


@functools.lru_cache(maxsize=None)
def e2e_reads():
    """the sample's reads: read_len bases, both strands, `coverage` fold, substitution errors, fixed seed"""
    p = E2E
    _, sample = e2e_genomes()
    rng = np.random.default_rng(p["seed"] + 1)
    reads = []
    for c in sample:
        for s in rng.integers(0, len(c) - p["read_len"] + 1, p["coverage"] * len(c) // p["read_len"]):
            r = _substitute(rng, c[int(s):int(s) + p["read_len"]], p["error"])
            reads.append(r if rng.random() < 0.5 else revcomp(r))
    return reads


def e2e_write_reads(tmp):
    """the reads as two FASTQ files under ``tmp``, the second gzipped and without a final line feed; their paths"""
    reads = e2e_reads()
    h = len(reads) // 2
    p1, p2 = os.path.join(str(tmp), "reads_1.fq"), os.path.join(str(tmp), "reads_2.fq.gz")
    with open(p1, "wb") as f:
        f.write(fastq_text(reads[:h]))
    with gzip.open(p2, "wb") as f:
        f.write(fastq_text(reads[h:])[:-1])
    return [p1, p2]


def model_rows(anchor, genomes, k):
    """per anchor contig the (rows, N) bits: bit g = genome g holds the row's canonical key (zeros at an invalid row)"""
    sets = [np.unique(cr.valid_keys(g, k)) for g in genomes]
    out = []
    for key, valid in cr.keys_of(anchor, k):
        out.append(np.stack([valid & np.isin(key, s) for s in sets], axis=1).astype(np.uint8) if len(key) else
                   np.zeros((0, len(genomes)), np.uint8))
    return out


def bin_geometry(size, bin_size):
    """(bin numbers, first row, end row) of the bins of a contig of ``size`` rows at step 1"""
    b = np.arange((size + bin_size - 1) // bin_size, dtype=np.int64)
    return b, b * bin_size, np.minimum(size, (b + 1) * bin_size)


@functools.lru_cache(maxsize=None)
def _e2e_depths_rows():
    gs, _ = e2e_genomes()
    k = E2E["k"]
    return sample_depths(gs[0], joined_reads(e2e_reads()), k), [rc.pack(r) for r in model_rows(gs[0], gs, k)]


def e2e_model(chroms=None, genomes=None, min_count=None, bin_size=None, batches=None):
    """(main, matrix, summary, stats) as Index.place returns them, from the model's counts and panagram_amd.place.frames.
    ``batches``: the chromosome batches the GPU side walks (lists of contig numbers; None: one batch of all) — ``hits`` is summed
    over them, a key of two batches counting in both."""
    from panagram_amd import place as pl
    p = E2E
    k = p["k"]
    min_count = p["min_count"] if min_count is None else min_count
    bin_size = p["bin_size"] if bin_size is None else bin_size
    gs, _ = e2e_genomes()
    anchor = gs[0]
    reads = e2e_reads()
    take = [i for i, c in enumerate(E2E_CHROMS) if chroms is None or c in chroms]
    depths, rows = _e2e_depths_rows()
    frames, ci, st, en = [], [], [], []
    for i in take:
        size = len(anchor[i]) - k + 1
        b, s, e = bin_geometry(size, bin_size)
        frames.append(pd.DataFrame({"chrom": E2E_CHROMS[i], "start": b * bin_size, "end": e}))
        ci += [i] * len(b)
        st += list(s)
        en += list(e)
    valid, held, col, both = agree(depths, rows, len(gs), min_count, ci, st, en)
    dh = np.zeros(cr.BINS, np.uint64)
    for i in take:
        d, v = depths[i]
        dh += np.bincount(np.minimum(d[v], cr.BINS - 1), minlength=cr.BINS).astype(np.uint64)
    hits = sum(cr.hits([anchor[i] for i in b], joined_reads(reads), k) for b in (batches if batches is not None else [take]))
    stats = dict(reads=len(reads), read_bases=sum(len(r) for r in reads), hits=hits, depth_hist=dh, depth_mode=pl.depth_mode(dh),
                 min_count=min_count)
    bins = pd.concat(frames, ignore_index=True)
    return (*pl.frames(bins, valid, held, col, both, E2E_NAMES, genomes), stats)


def e2e_donor_bins():
    """[(chrom, bin start, donor)] of the bins that lie wholly inside one donor's segment with at least one bin between them and a
    breakpoint (a contig's ends are no breakpoints)"""
    p = E2E
    out = []
    for i, n in enumerate(p["contig_lens"]):
        size, bs = n - p["k"] + 1, p["bin_size"]
        brk = n // 2 if i < 2 else None
        for b in range((size + bs - 1) // bs):
            s, e = b * bs, min(size, (b + 1) * bs) + p["k"] - 1  # the bases the bin's rows span
            if brk is None:
                out.append((E2E_CHROMS[i], s, "B"))
            elif e + bs <= brk:
                out.append((E2E_CHROMS[i], s, "B"))
            elif s - bs >= brk:
                out.append((E2E_CHROMS[i], s, "C"))
    return out
