"""Host side of `synteny`: the runs of unique k-mer matches the GPU returns (engine.synteny_segments: per run the contig of A,
its first k-mer position and exclusive end, and the mate word ``posB << 1 | strand`` of the first position) as a table of
segments with base coordinates on both genomes, and its summary; the blocks the GPU chains from those runs
(engine.synteny_blocks) as the same table with their runs and shifted links, and as PAF lines; the variants the GPU reads off
the blocks' links (engine.synteny_variants) as a table with both alleles, and as VCF lines.  No device code here.

A run of n k-mers covers n + k - 1 bases on either genome.  On strand ``+`` the run's first k-mer lies at ``posB`` and B's range
is ``[posB, posB + n + k - 1)``; on ``-`` the positions of B descend from ``posB``, the range is ``[posB - n + 1, posB + k)``.
Global positions of B become (contig, offset) by a search in the contigs' cumulative lengths: a run never crosses a contig edge
of B, since the last k-mer of one contig and the first of the next lie k bases apart."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import pandas as pd

NO_MATE = 0xFFFFFFFF
COLUMNS = ["chrA", "startA", "endA", "chrB", "startB", "endB", "strand", "kmers"]
BLOCK_COLUMNS = COLUMNS + ["runs", "shifted"]
SUMMARY_COLUMNS = ["chrA", "chrB", "strand", "segments", "kmers"]
TOTALS_COLUMNS = ["side", "genome", "unique", "mated"]
VARIANT_COLUMNS = ["chrA", "posA", "refLen", "chrB", "posB", "altLen", "strand", "class", "mismatches", "ref", "alt"]
VARIANT_CLASSES = ("same", "snp", "mnp", "ins", "del", "complex")
VARIANT_SUMMARY_COLUMNS = ["class", "count", "basesA", "basesB"]
ALL = "*"  # a summary line's chromosome: every chromosome of that side


def contig_offsets(lens: Sequence[int]) -> np.ndarray:
    """[n + 1] int64: the global base offset of every contig of a side, and the side's bases"""
    out = np.zeros(len(lens) + 1, np.int64)
    out[1:] = np.cumsum(np.asarray(lens, np.int64))
    return out


def locate(pos, offsets: np.ndarray):
    """(contig, offset inside it) of global base positions (an empty contig shares its offset with the next one: the search
    from the right lands on the one that holds the base)"""
    pos = np.asarray(pos, np.int64)
    c = np.searchsorted(offsets[:-1], pos, side="right") - 1
    return c, pos - offsets[c]


def segment_frame(run_contig, run_start, run_end, run_mate, k: int, names_a: Sequence[str], lens_b: Sequence[int],
                  names_b: Sequence[str], min_len: int = 1) -> pd.DataFrame:
    """one line per run of at least ``min_len`` k-mers, in the order of the runs: sorted by (contig of A, startA).  Base ranges
    are half-open and ``kmers + k - 1`` long on both genomes."""
    if min_len < 1:
        raise ValueError("min_len must be at least 1")
    c = np.asarray(run_contig, np.int64)
    s, e, m = (np.asarray(x, np.int64) for x in (run_start, run_end, run_mate))
    if not (len(c) == len(s) == len(e) == len(m)):
        raise ValueError("the run arrays differ in length")
    n = e - s
    if len(n) and (n.min() < 1 or (m == NO_MATE).any()):
        raise ValueError("a run without positions or without a mate")
    keep = n >= min_len
    c, s, e, m, n = c[keep], s[keep], e[keep], m[keep], n[keep]
    pos, strand = m >> 1, m & 1
    lo = np.where(strand == 0, pos, pos - (n - 1))
    offs = contig_offsets(lens_b)
    if len(lo) and (lo.min() < 0 or (lo + n + k - 1).max() > offs[-1]):
        raise ValueError("a run outside genome B")
    cb, ob = locate(lo, offs)
    if len(lo) and (ob + n + k - 1 > np.asarray(lens_b, np.int64)[cb]).any():
        raise ValueError("a run across a contig edge of genome B")
    na, nb = np.asarray(list(names_a), object), np.asarray(list(names_b), object)
    return pd.DataFrame({"chrA": na[c] if len(c) else np.zeros(0, object), "startA": s, "endA": e + k - 1,
                         "chrB": nb[cb] if len(c) else np.zeros(0, object), "startB": ob, "endB": ob + n + k - 1,
                         "strand": np.where(strand == 0, "+", "-").astype(object), "kmers": n}, columns=COLUMNS)


def block_frame(blk_contig, blk_start, blk_end, blk_mate_first, blk_mate_last, blk_kmers, blk_runs, blk_shifted, k: int,
                names_a: Sequence[str], lens_b: Sequence[int], names_b: Sequence[str], min_len: int = 1) -> pd.DataFrame:
    """one line per block (engine.synteny_blocks) of at least ``min_len`` k-mers, in the order of the blocks: sorted by (contig of
    A, startA).  Base ranges are half-open: ``endA = end + k - 1``; B's positions are monotone inside a block, so its range is
    ``[mate_first >> 1, (mate_last >> 1) + k)`` on ``+`` and ``[mate_last >> 1, (mate_first >> 1) + k)`` on ``-``.  The two
    ranges differ in length by the insertions and deletions the block bridges."""
    if min_len < 1:
        raise ValueError("min_len must be at least 1")
    cols = [np.asarray(x, np.int64) for x in (blk_contig, blk_start, blk_end, blk_mate_first, blk_mate_last, blk_kmers, blk_runs,
                                              blk_shifted)]
    if len({len(x) for x in cols}) != 1:
        raise ValueError("the block arrays differ in length")
    keep = cols[5] >= min_len
    c, s, e, mf, ml, km, nr, sh = (x[keep] for x in cols)
    if len(c) and ((e <= s).any() or (mf == NO_MATE).any() or (ml == NO_MATE).any() or ((mf ^ ml) & 1).any()):
        raise ValueError("a block without positions, without a mate or of two strands")
    strand = mf & 1
    lo = np.where(strand == 0, mf >> 1, ml >> 1)
    hi = np.where(strand == 0, ml >> 1, mf >> 1) + k
    offs = contig_offsets(lens_b)
    if len(lo) and ((lo > hi - k).any() or lo.min() < 0 or hi.max() > offs[-1]):  # (first k-mer of B behind the last: no block)
        raise ValueError("a block outside genome B")
    cb, ob = locate(lo, offs)
    if len(lo) and (ob + (hi - lo) > np.asarray(lens_b, np.int64)[cb]).any():
        raise ValueError("a block across a contig edge of genome B")
    na, nb = np.asarray(list(names_a), object), np.asarray(list(names_b), object)
    return pd.DataFrame({"chrA": na[c] if len(c) else np.zeros(0, object), "startA": s, "endA": e + k - 1,
                         "chrB": nb[cb] if len(c) else np.zeros(0, object), "startB": ob, "endB": ob + (hi - lo),
                         "strand": np.where(strand == 0, "+", "-").astype(object), "kmers": km, "runs": nr, "shifted": sh},
                        columns=BLOCK_COLUMNS)


def paf_lines(blocks: pd.DataFrame, lens_a, lens_b) -> list:
    """the blocks of ``block_frame`` as PAF lines, query = A, target = B: the 12 mandatory columns — name, length, start, end of
    the query, strand, name, length, start, end of the target, matches = ``kmers``, alignment length = the longer of the two
    ranges, mapping quality 255 (not available) — and the tags ``rn:i:<runs>`` and ``sh:i:<shifted>``.  ``lens_a`` / ``lens_b``:
    chromosome name -> length."""
    out = []
    for r in blocks.itertuples(index=False):
        aln = max(int(r.endA) - int(r.startA), int(r.endB) - int(r.startB))
        out.append("\t".join(str(v) for v in (r.chrA, int(lens_a[r.chrA]), int(r.startA), int(r.endA), r.strand, r.chrB, int(lens_b[r.chrB]),
                                              int(r.startB), int(r.endB), int(r.kmers), aln, 255, f"rn:i:{int(r.runs)}",
                                              f"sh:i:{int(r.shifted)}")))
    return out


_COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")


def _decode(word: int, n: int) -> str:
    """the first n <= 32 bases of an allele word: 2 bits per base, base i at bits 2i and 2i + 1"""
    return "".join("ACGT"[(word >> (2 * i)) & 3] for i in range(n))


def variant_frame(var_contig, var_pos_a, var_len_a, var_pos_b, var_len_b, var_info, var_mismatches, var_allele_a, var_allele_b,
                  names_a: Sequence[str], lens_b: Sequence[int], names_b: Sequence[str], seqs_a=None, seqs_b=None) -> pd.DataFrame:
    """one line per variant (engine.synteny_variants), in the order of the records: sorted by (contig of A, posA).  ``posA`` /
    ``posB`` are 0-based offsets inside the chromosome, ``refLen`` / ``altLen`` the alleles' lengths, ``ref`` A's allele and
    ``alt`` B's in A's orientation (reverse-complemented on strand ``-``; ``posB`` is the lowest base of B's range either way).
    Alleles of up to 32 bases are decoded from the GPU's words; a longer one, or one flagged as holding a base outside ACGT
    (shown as ``N``), is cut from ``seqs_a.unpack(contig)`` / ``seqs_b.unpack(contig)`` — each contig unpacked at most once, and
    only when such an allele needs it.  The anchor bases (the base of A in front of every variant, for ``vcf_lines``) ride in
    ``frame.attrs["anchor"]``."""
    cols = [np.asarray(x, np.int64) for x in (var_contig, var_pos_a, var_len_a, var_pos_b, var_len_b, var_info, var_mismatches)]
    words = [np.asarray(x, np.uint64) for x in (var_allele_a, var_allele_b)]
    if len({len(x) for x in cols + words}) != 1:
        raise ValueError("the variant arrays differ in length")
    c, pa, la, pb, lb, info, mism = cols
    strand, cls, anchor, nflag = info & 1, (info >> 1) & 7, (info >> 4) & 3, (info >> 6) & 1
    if len(c) and (cls.min() < 1 or cls.max() > 5 or (info >> 7).any()):
        raise ValueError("a variant of no class")
    offs = contig_offsets(lens_b)
    if len(c) and (pb.min() < 0 or (pb + lb).max() > offs[-1]):
        raise ValueError("a variant outside genome B")
    cb, ob = locate(pb, offs)
    if len(c) and (ob + lb > np.asarray(lens_b, np.int64)[cb]).any():
        raise ValueError("a variant across a contig edge of genome B")
    unpacked = {}

    def cut(side, seqs, contig, pos, n):
        if seqs is None:
            raise ValueError("an allele of more than 32 bases, or one with a base outside ACGT, needs the sequence sets")
        if (side, contig) not in unpacked:
            unpacked[(side, contig)] = bytes(seqs.unpack(contig))
        return unpacked[(side, contig)][pos:pos + n]
    ref, alt = [], []
    for i in range(len(c)):
        whole = nflag[i] == 0
        if la[i] <= 32 and whole:
            ref.append(_decode(int(words[0][i]), int(la[i])))
        else:
            ref.append(cut(0, seqs_a, int(c[i]), int(pa[i]), int(la[i])).decode())
        if lb[i] <= 32 and whole:
            alt.append(_decode(int(words[1][i]), int(lb[i])))
        else:
            s = cut(1, seqs_b, int(cb[i]), int(ob[i]), int(lb[i]))
            alt.append((s.translate(_COMPLEMENT)[::-1] if strand[i] else s).decode())
    na, nb = np.asarray(list(names_a), object), np.asarray(list(names_b), object)
    empty = np.zeros(0, object)
    out = pd.DataFrame({"chrA": na[c] if len(c) else empty, "posA": pa, "refLen": la, "chrB": nb[cb] if len(c) else empty, "posB": ob,
                        "altLen": lb, "strand": np.where(strand == 0, "+", "-").astype(object),
                        "class": np.asarray(VARIANT_CLASSES, object)[cls] if len(c) else empty, "mismatches": mism,
                        "ref": np.asarray(ref, object), "alt": np.asarray(alt, object)}, columns=VARIANT_COLUMNS)
    out.attrs["anchor"] = ["ACGT"[x] for x in anchor.tolist()]
    return out


def vcf_lines(variants: pd.DataFrame, lens_a, sample: str) -> list:
    """the variants of ``variant_frame`` as VCF 4.2 lines of B (the one sample, genotype ``1``) against A: a snp or mnp stands at
    POS = posA + 1 with the two alleles; an ins, del or complex one at POS = posA with both alleles behind the anchor base (the
    base of A in front of it, the same in B).  FILTER is ``PASS``, or ``N`` when an allele holds a base outside ACGT.  INFO:
    ``CLASS``, ``BCHR`` / ``BPOS`` (the chromosome of B and the 1-based place of the B allele's lowest base there; of the base
    behind it when the allele is empty), ``STRAND`` and ``MISM``.  ``lens_a``: chromosome of A -> length, in file order."""
    anchor = variants.attrs.get("anchor")
    if anchor is None or len(anchor) != len(variants):
        raise ValueError("vcf_lines takes variant_frame's own frame: the anchor bases ride in its attrs")
    out = ["##fileformat=VCFv4.2"]
    out += [f"##contig=<ID={name},length={int(n)}>" for name, n in lens_a.items()]
    out += ['##INFO=<ID=CLASS,Number=1,Type=String,Description="snp, mnp, ins, del or complex">',
            '##INFO=<ID=BCHR,Number=1,Type=String,Description="chromosome of the sample that holds the allele">',
            '##INFO=<ID=BPOS,Number=1,Type=Integer,Description="1-based position of the allele\'s lowest base there">',
            '##INFO=<ID=STRAND,Number=1,Type=String,Description="+ or -: the strand of the sample that matches the reference">',
            '##INFO=<ID=MISM,Number=1,Type=Integer,Description="mismatching bases of a snp or mnp">',
            '##FILTER=<ID=N,Description="an allele holds a base outside ACGT">',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + str(sample)]
    for r, base in zip(variants.itertuples(index=False), anchor):
        cls = r[7]
        if cls in ("snp", "mnp"):
            pos, ref, alt = int(r.posA) + 1, r.ref, r.alt
        else:
            pos, ref, alt = int(r.posA), base + r.ref, base + r.alt
        flt = "N" if "N" in r.ref or "N" in r.alt else "PASS"
        info = f"CLASS={cls};BCHR={r.chrB};BPOS={int(r.posB) + 1};STRAND={r.strand};MISM={int(r.mismatches)}"
        out.append("\t".join(str(v) for v in (r.chrA, pos, ".", ref, alt, ".", flt, info, "GT", 1)))
    return out


def apply_variants(seq, variants: pd.DataFrame, start: int = 0, end=None, chrom=None) -> bytes:
    """bases [start, end) of a chromosome of A with every variant of ``variants`` that lies inside them carried out: ``ref``
    replaced by ``alt``.  Over a block's range of A — its first run's start to its last run's end + k - 1 — the result is B's
    range of the block, reverse-complemented on strand ``-``.  ``chrom``: only the variants of this chromosome."""
    seq = bytes(seq)
    end = len(seq) if end is None else int(end)
    rows = variants if chrom is None else variants[variants["chrA"] == chrom]
    out, at = [], int(start)
    for pos, n, ref, alt in zip(rows["posA"].tolist(), rows["refLen"].tolist(), rows["ref"].tolist(), rows["alt"].tolist()):
        if pos < start or pos + n > end:
            continue
        if pos < at:
            raise ValueError("variants that overlap, or are not sorted by posA")
        out += [seq[at:pos], alt.encode()]
        at = pos + n
    return b"".join(out + [seq[at:end]])


def variant_summary_frame(variants: pd.DataFrame, class_counts, links: int) -> pd.DataFrame:
    """class, count, bases on A and on B: one line per class of variant, then the ``same`` links (no difference: no bases) and
    all ``links`` — the counts are the GPU's (``class_counts``: the six of engine.synteny_variants), the bases the table's"""
    counts = [int(x) for x in class_counts]
    if len(counts) != 6 or sum(counts) != int(links):
        raise ValueError("six class counts that add up to the links")
    rows = []
    for i, name in enumerate(VARIANT_CLASSES[1:], 1):
        mine = variants[variants["class"] == name]
        if len(mine) != counts[i]:
            raise ValueError(f"{len(mine)} {name} variants in the table, {counts[i]} counted")
        rows.append([name, counts[i], int(mine["refLen"].sum()), int(mine["altLen"].sum())])
    rows.append(["same", counts[0], 0, 0])
    rows.append(["links", int(links), sum(r[2] for r in rows), sum(r[3] for r in rows)])
    return pd.DataFrame(rows, columns=VARIANT_SUMMARY_COLUMNS)


def summary_frame(segments: pd.DataFrame) -> pd.DataFrame:
    """the segments and the shared unique k-mers of every (chrA, chrB, strand) that has a segment, in order of first appearance;
    then per side: one line per chromosome of A over all of B (chrB ``*``, strand ``*``), one per chromosome of B over all of A,
    and the total (``* * *``).  With ``min_len`` 1 the total's k-mers are the mated positions of A.  Works on any frame whose
    leading columns are ``segment_frame``'s — ``block_frame``'s too: the count column reads ``segments`` for either kind, and
    counts blocks there."""
    def lines(keys, a, b, strand):
        g = segments.groupby(keys, sort=False)["kmers"].agg(["size", "sum"]).reset_index()
        return pd.DataFrame({"chrA": g["chrA"] if a is None else a, "chrB": g["chrB"] if b is None else b,
                             "strand": g["strand"] if strand is None else strand, "segments": g["size"].astype(np.int64),
                             "kmers": g["sum"].astype(np.int64)}, columns=SUMMARY_COLUMNS)
    total = pd.DataFrame([[ALL, ALL, ALL, len(segments), int(segments["kmers"].sum())]], columns=SUMMARY_COLUMNS)
    if not len(segments):
        return total
    return pd.concat([lines(["chrA", "chrB", "strand"], None, None, None), lines(["chrA"], None, ALL, ALL),
                      lines(["chrB"], ALL, None, ALL), total], ignore_index=True)


def totals_frame(name_a: str, name_b: str, unique_a: int, unique_b: int, mated: int) -> pd.DataFrame:
    """per side: the positions whose k-mer is unique in that genome, and those of them that have a mate in the other — the
    same number on both sides, a mate being a pair"""
    return pd.DataFrame({"side": ["A", "B"], "genome": [name_a, name_b], "unique": [int(unique_a), int(unique_b)],
                         "mated": [int(mated), int(mated)]}, columns=TOTALS_COLUMNS)


def write_summary(path, summary: pd.DataFrame, totals: pd.DataFrame) -> None:
    """the summary table, tab-separated under its header, behind the totals as ``#`` lines (``side genome unique mated``)"""
    with open(path, "w") as f:
        f.write("# " + "\t".join(TOTALS_COLUMNS) + "\n")
        for row in totals.values.tolist():
            f.write("# " + "\t".join(str(v) for v in row) + "\n")
        summary.to_csv(f, sep="\t", index=False)


def chromosome_map(segments: pd.DataFrame) -> pd.DataFrame:
    """which chromosome of B corresponds to each chromosome of A: per chrA the chrB that holds most of its shared unique
    k-mers, with those k-mers, all of chrA's, and the share on strand ``-``.  Takes ``segment_frame``'s lines or
    ``block_frame``'s: it reads ``chrA``, ``chrB``, ``strand`` and ``kmers``."""
    rows = []
    for a, g in segments.groupby("chrA", sort=False):
        per = g.groupby("chrB", sort=False)["kmers"].sum()
        b = per.idxmax()
        best = g[g["chrB"] == b]
        rows.append([a, b, int(per.max()), int(per.sum()), float(best.loc[best["strand"] == "-", "kmers"].sum()) / float(per.max())])
    return pd.DataFrame(rows, columns=["chrA", "chrB", "kmers", "kmers_all", "minus_frac"])


def pick_contigs(names: Sequence[str], chosen) -> list:
    """the indices of the chromosomes ``chosen`` (None: all) in the order of ``names``' sequence set"""
    names = list(names)
    if chosen is None:
        return list(range(len(names)))
    chosen = list(chosen)
    unknown = [c for c in chosen if c not in names]
    if unknown:
        raise ValueError(f"unknown chromosome {unknown[0]!r} (there are {', '.join(map(str, names))})")
    if len(set(chosen)) != len(chosen):
        raise ValueError("a chromosome is named twice")
    want = set(chosen)
    return [i for i, n in enumerate(names) if n in want]
