"""Host side of `genotype`: which allele a sample carries at every variant of genome B against genome A.  The variants are those of
``synteny --variants`` (synteny.variant_frame); per variant the GPU returns, for A's allele and for B's, the allele windows whose
k-mer is informative — once in the allele's own genome, nowhere in the other — and how many of those the sample holds
(engine.CopyTable.allele_support; include/panagram_hip.h has the definitions).  Here: the variants as the two range lists, the
call rule, the table, the VCF lines with a sample column, and the summary.  No device code.

A's range of a variant is ``(contig of chrA, posA, refLen)``, B's ``(contig of chrB, posB, altLen)`` — variant_frame has mapped B's
global position to chromosome and offset (synteny.contig_offsets / locate) — both in the genomes' WHOLE assemblies: a side narrowed
to some chromosomes took them whole, so offsets inside a chromosome are the same.

Call rule, with ``min_frac`` F in (0, 1]: an allele is present when ``inf > 0 and seen >= F * inf``.  ``GT`` is ``./.`` with flag
``uninformative`` when either side has ``inf == 0``; otherwise ``0/1`` when both alleles are present, ``0/0`` when only A's, ``1/1``
when only B's, and ``./.`` with flag ``neither`` when neither is (no coverage, or a third allele)."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import pandas as pd

from . import synteny

CALL_COLUMNS = ["ref_kmers", "ref_seen", "ref_depth", "alt_kmers", "alt_seen", "alt_depth", "GT", "flag"]
FRAME_COLUMNS = synteny.VARIANT_COLUMNS + CALL_COLUMNS
TABLE_COLUMNS = [c for c in synteny.VARIANT_COLUMNS if c != "mismatches"] + CALL_COLUMNS  # what the command prints
SUMMARY_COLUMNS = ["class", "GT", "count"]
GENOTYPES = ("0/0", "0/1", "1/1", "./.")
STAT_NAMES = ["reads", "windows", "hits", "sites", "callable", "min_count", "min_frac"]
FORMAT_LINES = ['##FORMAT=<ID=RK,Number=2,Type=Integer,Description="informative k-mers of the reference allele the sample holds, and all of them">',
                '##FORMAT=<ID=AK,Number=2,Type=Integer,Description="informative k-mers of the alternate allele the sample holds, and all of them">']


def check_min_frac(min_frac) -> float:
    f = float(min_frac)
    if not 0.0 < f <= 1.0:
        raise ValueError(f"genotype: min_frac={min_frac} (above 0, at most 1)")
    return f


def check_min_count(min_count) -> int:
    m = int(min_count)
    if not 1 <= m <= 0xFFFFFFFF:
        raise ValueError(f"genotype: min_count={min_count} (1 to 2^32 - 1)")
    return m


def allele_ranges(variants: pd.DataFrame, names_a: Sequence[str], names_b: Sequence[str]):
    """((contig, start, len) of A's alleles, the same of B's) as uint32 / uint64 / uint64 arrays: the contig numbers are those of
    ``names_a`` / ``names_b``, the chromosomes of the whole assemblies in file order"""
    out = []
    for names, chrom, pos, length in ((names_a, "chrA", "posA", "refLen"), (names_b, "chrB", "posB", "altLen")):
        number = {}
        for i, n in enumerate(names):
            number.setdefault(n, i)
        unknown = [c for c in variants[chrom].unique() if c not in number]
        if unknown:
            raise ValueError(f"genotype: a variant on chromosome {unknown[0]!r}, which the assembly does not name")
        out.append((np.asarray([number[c] for c in variants[chrom]], np.uint32), variants[pos].to_numpy(np.uint64),
                    variants[length].to_numpy(np.uint64)))
    return tuple(out)


def present(inf, seen, min_frac: float) -> np.ndarray:
    inf, seen = np.asarray(inf, np.int64), np.asarray(seen, np.int64)
    return (inf > 0) & (seen >= float(min_frac) * inf)


def call(ref_inf, ref_seen, alt_inf, alt_seen, min_frac: float):
    """(GT [object], flag [object]) per site, by the call rule above; an empty flag is ``""``"""
    ri, ai = np.asarray(ref_inf, np.int64), np.asarray(alt_inf, np.int64)
    pr, pa = present(ri, ref_seen, min_frac), present(ai, alt_seen, min_frac)
    blind = (ri == 0) | (ai == 0)
    gt = np.where(blind, "./.", np.where(pr & pa, "0/1", np.where(pr, "0/0", np.where(pa, "1/1", "./.")))).astype(object)
    flag = np.where(blind, "uninformative", np.where(~pr & ~pa, "neither", "")).astype(object)
    return gt, flag


def mean_depth(depth, inf) -> np.ndarray:
    """``depth / inf`` to two decimals as text, ``.`` where ``inf == 0``"""
    return np.asarray(["." if int(n) == 0 else f"{int(d) / int(n):.2f}" for d, n in zip(depth, inf)], object)


def frames(variants: pd.DataFrame, ref_support, alt_support, min_frac: float):
    """(table, summary) of the variants of ``synteny.variant_frame`` (chromosomes named) and the two sides' ``(windows, inf, seen,
    depth)`` of ``CopyTable.allele_support``.  table: FRAME_COLUMNS — ``*_kmers`` = inf, ``*_depth`` = the mean depth of the
    informative k-mers — with the variants' anchor bases in its attrs, for ``vcf_lines``; summary: SUMMARY_COLUMNS, the sites of
    every class and genotype that occurs, classes in synteny.VARIANT_CLASSES' order, genotypes in GENOTYPES'."""
    min_frac = check_min_frac(min_frac)
    n = len(variants)
    if any(len(x) != n for x in tuple(ref_support) + tuple(alt_support)):
        raise ValueError("genotype: the support arrays need one entry per variant")
    (_, ri, rs, rd), (_, ai, as_, ad) = ([np.asarray(x, np.uint64) for x in side] for side in (ref_support, alt_support))
    gt, flag = call(ri, rs, ai, as_, min_frac)
    table = variants.copy()
    table.attrs = dict(variants.attrs)
    for name, col in zip(CALL_COLUMNS, (ri.astype(np.int64), rs.astype(np.int64), mean_depth(rd, ri), ai.astype(np.int64),
                                        as_.astype(np.int64), mean_depth(ad, ai), gt, flag)):
        table[name] = col
    table = table[FRAME_COLUMNS]
    rows = []
    for cls in synteny.VARIANT_CLASSES[1:]:
        mine = gt[(table["class"] == cls).to_numpy(bool)] if n else gt
        for g in GENOTYPES:
            count = int((mine == g).sum())
            if count:
                rows.append([cls, g, count])
    return table, pd.DataFrame(rows, columns=SUMMARY_COLUMNS)


def stats(table: pd.DataFrame, ref_support, alt_support, reads: int, hits: int, min_count: int, min_frac: float) -> dict:
    """STAT_NAMES: the sample's reads (the records of a FASTA), the allele windows of both sides, the sample's windows whose k-mer
    is an allele k-mer, the sites, those with informative k-mers on both sides, and the two thresholds"""
    windows = int(np.asarray(ref_support[0], np.uint64).sum()) + int(np.asarray(alt_support[0], np.uint64).sum())
    return {"reads": int(reads), "windows": windows, "hits": int(hits), "sites": len(table),
            "callable": int((table["flag"] != "uninformative").sum()), "min_count": int(min_count), "min_frac": float(min_frac)}


def table_text(table: pd.DataFrame) -> str:
    """the table as the command prints it: TABLE_COLUMNS, tab-separated with a header, ``-`` for an empty allele or flag"""
    out = table[TABLE_COLUMNS].replace({"ref": {"": "-"}, "alt": {"": "-"}, "flag": {"": "-"}})
    return out.to_csv(sep="\t", index=False)


def vcf_lines(table: pd.DataFrame, lens_a, sample: str) -> list:
    """``synteny.vcf_lines`` of the variants with the sample's call in place of B's column: FORMAT ``GT:RK:AK``, RK = ref_seen,
    ref_kmers and AK = alt_seen, alt_kmers"""
    lines = synteny.vcf_lines(table, lens_a, sample)
    head = [ln for ln in lines if ln.startswith("#")]
    body = lines[len(head):]
    if len(body) != len(table):
        raise ValueError("genotype: one VCF line per variant")
    out = head[:-1] + FORMAT_LINES + head[-1:]
    for ln, gt, rs, rk, as_, ak in zip(body, table["GT"], table["ref_seen"], table["ref_kmers"], table["alt_seen"], table["alt_kmers"]):
        out.append("\t".join(ln.split("\t")[:8] + ["GT:RK:AK", f"{gt}:{int(rs)},{int(rk)}:{int(as_)},{int(ak)}"]))
    return out


def summary_text(summary: pd.DataFrame, st: dict) -> str:
    """the statistics as ``#`` lines (``min_frac`` to six places), then ``class GT count``"""
    head = [f"# {n}\t{st[n]:.6f}" if isinstance(st[n], float) else f"# {n}\t{int(st[n])}" for n in STAT_NAMES]
    return "\n".join(head) + "\n" + summary.to_csv(sep="\t", index=False)


def write_main(table: pd.DataFrame, out) -> None:
    if hasattr(out, "write"):
        out.write(table_text(table))
    else:
        with open(out, "w") as f:
            f.write(table_text(table))


def write_summary(summary: pd.DataFrame, st: dict, path) -> None:
    with open(path, "w") as f:
        f.write(summary_text(summary, st))
