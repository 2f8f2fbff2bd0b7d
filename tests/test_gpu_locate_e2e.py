"""GPU: Index.locate, Genome.gene_loci and the `locate` subcommand on an index written by Index.run() — three small genomes with
genes planted at known places (tests/locate_ref.py: e2e_genomes; tests/test_locate_cpu.py holds them to their truth) — against
``locate.frames`` of the numpy model's arrays, exactly."""
import os
import subprocess
import sys

import pytest

from oracle import pyoracle as po
from panagram_amd import locate as loc
from tests import locate_ref as lr

pytestmark = pytest.mark.gpu

K = lr.E2E_K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, CHROMS = lr.E2E_NAMES, lr.E2E_CHROMS


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("locate")
    genomes, _, genes, _ = lr.e2e_genomes()
    gff = tmp / "g0.gff"
    with open(gff, "w") as fh:
        fh.write("##gff-version 3\n")
        for i, (c, s, e) in enumerate(genes):
            fh.write(f"{c}\tsrc\tgene\t{s}\t{e}\t.\t+\t.\tID=g{i}\n")
            fh.write(f"{c}\tsrc\texon\t{s}\t{e}\t.\t+\t.\tParent=g{i}\n")
    lines = ["name\tfasta\tgff"]
    for i, contigs in enumerate(genomes):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(CHROMS, contigs))
        lines.append(f"g{i}\t{fa}\t" + (str(gff) if i == 0 else ""))
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def queries():
    return [(n, s) for n, s, _ in lr.e2e_queries()]


def fasta(width=60):
    out = []
    for i, (name, seq) in enumerate(queries()):
        out.append(b">" + name.encode() + (b" a description" if i == 1 else b"") + b"\n")
        out += [seq[j:j + width] + b"\n" for j in range(0, len(seq), width)]
    return b"".join(out)


def reference(named, cols=(0, 1, 2), k=K, **kw):
    genomes = lr.e2e_genomes()[0]
    return lr.loci_frames([n for n, _ in named], [s for _, s in named], [(NAMES[c], CHROMS, genomes[c]) for c in cols], k, **kw)


def chrom_lens():
    return {n: dict(zip(CHROMS, map(len, g))) for n, g in zip(NAMES, lr.e2e_genomes()[0])}


def _same(got, want, tag):
    for g, w, what in zip(got, want, ("loci", "matrix", "summary")):
        assert g.to_csv(sep="\t") == w.to_csv(sep="\t"), (tag, what)


def test_locate_equals_the_model(built):
    from panagram_amd import index as pidx
    want = reference(queries())
    idx = pidx.Index(built, mode="r")
    try:
        got = idx.locate(fasta())
        _same(got, want, "fasta")
        loci, matrix, summary = got
        assert matrix.index.tolist() == [n for n, _ in queries()]
        assert matrix.to_numpy().tolist() == [[1, 3, 0], [1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1], [1, 0, 0]]
        a1 = loci[(loci["query"] == "geneA") & (loci["genome"] == "g1")]
        assert a1[["chrom", "start", "end", "strand"]].to_numpy().tolist() == [["chr1", 700, 2200, "+"], ["chr1", 2900, 4400, "-"],
                                                                              ["chr1", 5100, 6600, "+"]]
        assert loci.attrs["chrom_lens"] == chrom_lens() and loc.paf_lines(loci, loci.attrs["chrom_lens"]) == loc.paf_lines(want[0], chrom_lens())
        assert not idx._seqsets  # (what the call loaded it dropped again)
        # a list of (name, sequence); a selection, another k and other parameters; the filters
        _same(idx.locate(queries()), want, "pairs")
        sub = idx.locate(queries(), ["g2", "g1"], k=15, min_run=3, max_gap=40, max_shift=2)
        _same(sub, reference(queries(), (1, 2), 15, min_run=3, max_gap=40, max_shift=2), "selection")
        assert sub[1].columns.tolist() == ["g1", "g2"]
        _same(idx.locate(queries(), min_kmers=400, min_frac=0.99), reference(queries(), min_kmers=400, min_frac=0.99), "filters")
        held = idx.seqset_for("g1")  # a sequence set that was loaded before stays
        idx.locate(queries()[:1], ["g1"])
        assert idx._seqsets.get("g1") is held
        with pytest.raises(KeyError, match="nobody"):
            idx.locate(queries(), ["nobody"])
        with pytest.raises(ValueError, match="k=33"):
            idx.locate(queries(), k=33)
        with pytest.raises(ValueError, match="max_gap"):
            idx.locate(queries(), max_gap=0)
        with pytest.raises(ValueError, match="min_frac"):
            idx.locate(queries(), min_frac=2.0)
        empty = idx.locate(b"")
        assert len(empty[0]) == 0 and empty[1].shape == (0, 3)
        short = idx.locate([("short", b"ACGT")])
        assert len(short[0]) == 0 and short[2].to_numpy().tolist() == [["short", 4, 0, 0, 0, 0, "-", 0.0]]
    finally:
        idx.close()


def test_gene_loci_on_a_small_gff(built):
    from panagram_amd import index as pidx
    genomes, _, genes, _ = lr.e2e_genomes()
    chrom = dict(zip(CHROMS, genomes[0]))
    order = sorted(range(len(genes)), key=lambda i: (genes[i][0], genes[i][1]))  # (load_genes sorts by chromosome and start)
    named = [(f"{genes[i][0]}:{genes[i][1]}-{genes[i][2]}", chrom.get(genes[i][0], b"")[genes[i][1]:max(genes[i][1], genes[i][2])]) for i in order]
    idx = pidx.Index(built, mode="r")
    try:
        got = idx["g0"].gene_loci()
        _same(got, reference(named), "genes")
        m = got[1]
        assert m.loc["chr1:613-2113"].tolist() == [1, 3, 0] and m.loc["chr2:77-477"].tolist() == [1, 0, 0]
        assert m.loc["chrZ:10-500"].tolist() == [0, 0, 0] and m.loc["chr1:900-880"].tolist() == [0, 0, 0]
        _same(idx["g0"].gene_loci(["g1"], min_frac=0.99), reference(named, (1,), min_frac=0.99), "genes, filtered")
        with pytest.raises(ValueError, match="GFF"):
            idx["g1"].gene_loci()
        # gene_copies goes through the same cut of the genes
        assert idx["g0"].gene_copies()[1].index.tolist() == [n for n, _ in named]
    finally:
        idx.close()


def test_locate_subcommand_in_a_child_process(built, tmp_path):
    want_loci, want_matrix, want_summary = reference(queries())
    qfa = tmp_path / "queries.fa"
    qfa.write_bytes(fasta(70))
    out, mx, su, paf, flt = (tmp_path / n for n in ("loci.tsv", "matrix.tsv", "summary.tsv", "loci.paf", "filtered.tsv"))
    run = ["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "locate", built]
    p = subprocess.run(run + [str(qfa), "-o", str(out), "--matrix", str(mx), "--summary", str(su)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_text() == want_loci.to_csv(sep="\t", index=False)
    assert mx.read_text() == want_matrix.to_csv(sep="\t", index_label="query")
    assert su.read_text() == want_summary.to_csv(sep="\t", index=False)
    # PAF of a selection with a filter, to a file and to stdout
    sel = reference(queries(), (0, 1), min_frac=0.99)
    p = subprocess.run(run + [str(qfa), "--paf", "--genomes", "g1,g0", "--min-frac", "0.99", "-o", str(paf)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = loc.paf_lines(sel[0], chrom_lens())
    assert paf.read_text().split("\n")[:-1] == lines and len(lines) == 7 and all(len(x.split("\t")) == 15 for x in lines)
    # the genes of g0 as the queries, the table on stdout
    p = subprocess.run(run + ["--genes", "g0", "--genomes", "g1", "--min-kmers", "100"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [x.split("\t") for x in p.stdout.split("\n")[:-1]]
    assert rows[0] == loc.LOCI_COLUMNS and [r[:6] for r in rows[1:]] == [
        ["chr1:613-2113", "g1", "chr1", "700", "2200", "+"], ["chr1:613-2113", "g1", "chr1", "2900", "4400", "-"],
        ["chr1:613-2113", "g1", "chr1", "5100", "6600", "+"], ["chr1:2813-3713", "g1", "chr2", "0", "900", "+"]]
    # an unknown genome name, both kinds of queries at once: argparse errors that say so
    p = subprocess.run([sys.executable, "-m", "panagram_amd", "locate", built, str(qfa), "--genomes", "g1,nobody"], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 2 and "nobody" in p.stderr
    p = subprocess.run([sys.executable, "-m", "panagram_amd", "locate", built, str(qfa), "--genes", "g0"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 2 and "exactly one" in p.stderr
