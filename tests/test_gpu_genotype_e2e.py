"""GPU: `python -m panagram_amd genotype` on an index written by Index.run() from the planted genomes of tests/genotype_ref.py, at
k = 21 and k = 31: reads of A, reads of B, both, and a mosaic of the two — the table, the VCF and the summary byte for byte the
numpy model's, the genotypes the planted truth on every site but the two named hard ones; the same sample as an assembly; a run
narrowed to one chromosome of A; and every refusal of the command."""
import gzip
import os

import pytest

from oracle import pyoracle as po
from tests import genotype_ref as gr

pytestmark = pytest.mark.gpu

NAMES = ["A", "B"]
FLAGS = ["--max-shift", str(gr.E2E_PARAMS["max_shift"]), "--max-gap", str(gr.E2E_PARAMS["max_gap"])]


@pytest.fixture(scope="module", params=[21, 31])
def built(request, tmp_path_factory):
    """(k, index directory, sample name -> its files): reads_ab is two FASTQ files, one of them gzipped"""
    from panagram_amd import index as pidx
    k = request.param
    tmp = tmp_path_factory.mktemp(f"genotype{k}")
    a, b, _ = gr.planted()
    lines = ["name\tfasta"]
    for name, contigs in zip(NAMES, (a, b)):
        fa = tmp / f"{name}.fa"
        fa.write_bytes(po.fasta_text(gr.E2E_CHROMS, contigs))
        lines.append(f"{name}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=k, anchor_genomes=["A"], lowres_step=100).run()
    files = {}
    for name, (genomes, _) in gr.samples().items():
        files[name] = []
        for i, g in enumerate(genomes):
            gz = name == "reads_ab" and i == 1
            path = tmp / f"{name}_{i}.fq{'.gz' if gz else ''}"
            (gzip.open if gz else open)(path, "wb").write(gr.fastq_text(gr.reads_of(g)))
            files[name].append(str(path))
    mosaic = tmp / "mosaic.fa"
    mosaic.write_bytes(po.fasta_text(gr.E2E_CHROMS, gr.samples()["mosaic"][0][0]))
    files["mosaic_fa"] = [str(mosaic)]
    return k, out, files


def _run(args):
    from panagram_amd.__main__ import main
    assert main(["genotype"] + args) == 0


@pytest.mark.parametrize("sample", sorted(gr.samples()))
def test_table_and_summary_are_the_models_and_the_truth(built, tmp_path, sample):
    k, out, files = built
    m = gr.e2e_model(k, sample)
    assert not [r for r in m["rows"] if r[16] == "./."]  # (tests/test_genotype_cpu.py: the model leaves out no site)
    table, summ = tmp_path / "table.tsv", tmp_path / "summary.tsv"
    batch = ["--batch-bytes", str(300000)] if sample == "reads_a" else []  # (about 1 MB of FASTQ text: four batches)
    _run([out, "A", "B", *files[sample], "-o", str(table), "--summary", str(summ)] + FLAGS + batch)
    assert table.read_text() == gr.table_text(m["rows"])
    assert summ.read_text() == gr.summary_text(m["rows"], m["reads"], m["hits"], *m["support"], 2, gr.E2E_MIN_FRAC)
    got = [ln.split("\t") for ln in table.read_text().splitlines()[1:]]
    truth = gr.samples()[sample][1]
    checked = 0
    for f in got:
        c = gr.E2E_CHROMS.index(f[0])
        if not gr.is_hard(c, int(f[1])):
            assert f[16] == truth(c) and f[17] == "-", f
            checked += 1
    assert checked == len(got) - 2 >= 140


def test_vcf_is_the_models(built, capsys):
    from panagram_amd import genotype as gt
    from panagram_amd import synteny
    k, out, files = built
    m = gr.e2e_model(k, "mosaic")
    a, _, _ = gr.planted()
    lens_a = dict(zip(gr.E2E_CHROMS, (len(c) for c in a)))
    capsys.readouterr()
    _run([out, "A", "B", *files["mosaic"], "--vcf", "--sample", "mine"] + FLAGS)
    lines = capsys.readouterr().out.splitlines()
    base = synteny.vcf_lines(m["frame"], lens_a, "mine")  # (the variants' own fields: `synteny --variants --vcf`'s)
    head = [ln for ln in base if ln.startswith("#")]
    want = head[:-1] + gt.FORMAT_LINES + head[-1:]
    for ln, f in zip(base[len(head):], gr.vcf_body(m["rows"], m["anchors"])):
        v = ln.split("\t")
        assert (v[0], v[1], v[3], v[4]) == f[:4]
        want.append("\t".join(v[:8] + [f[4], f[5]]))
    assert lines == want and len(lines) == len(head) + 2 + len(m["rows"])
    # the default name of the sample column: the first file's base name
    _run([out, "A", "B", *files["mosaic"], "--vcf"] + FLAGS)
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines if ln.startswith("#CHROM")][0].split("\t")[-1] == os.path.basename(files["mosaic"][0])
    assert lines[len(want) - len(m["rows"]):] == want[len(want) - len(m["rows"]):]


def test_an_assembly_gives_the_same_genotypes(built, tmp_path):
    k, out, files = built
    m = gr.e2e_model(k, "mosaic", fasta=True)
    table, summ = tmp_path / "table.tsv", tmp_path / "summary.tsv"
    _run([out, "A", "B", *files["mosaic_fa"], "-o", str(table), "--summary", str(summ)] + FLAGS)
    assert table.read_text() == gr.table_text(m["rows"])
    assert summ.read_text() == gr.summary_text(m["rows"], 3, m["hits"], *m["support"], 1, gr.E2E_MIN_FRAC)
    assert [r[16] for r in m["rows"]] == [r[16] for r in gr.e2e_model(k, "mosaic")["rows"]]
    # min_count and min_frac reach the kernel and the rule: the model at 3 and 1.0
    m3 = gr.e2e_model(k, "reads_ab", min_count=3, min_frac=1.0)
    _run([out, "A", "B", *files["reads_ab"], "-o", str(table), "--min-count", "3", "--min-frac", "1"] + FLAGS)
    assert table.read_text() == gr.table_text(m3["rows"])


def test_a_narrowed_side_is_judged_against_the_whole_assemblies(built, tmp_path):
    k, out, files = built
    m = gr.e2e_model(k, "mosaic")
    table = tmp_path / "table.tsv"
    _run([out, "A", "B", *files["mosaic"], "-o", str(table), "--chroms-a", "chr2"] + FLAGS)
    full = gr.table_text(m["rows"]).splitlines()
    assert table.read_text().splitlines() == full[:1] + [ln for ln in full[1:] if ln.startswith("chr2\t")]
    assert len(table.read_text().splitlines()) > 30


def test_the_index_call_returns_frames(built):
    from panagram_amd import genotype as gt
    from panagram_amd import index as pidx
    k, out, files = built
    m = gr.e2e_model(k, "reads_b")
    idx = pidx.Index(out, mode="r")
    try:
        table, summary, stats = idx.genotype("A", "B", files["reads_b"], **gr.E2E_PARAMS)
        assert gt.table_text(table) == gr.table_text(m["rows"])
        assert list(summary.columns) == gt.SUMMARY_COLUMNS and int(summary["count"].sum()) == len(m["rows"]) == stats["sites"]
        assert stats["reads"] == m["reads"] and stats["hits"] == m["hits"] and stats["min_count"] == 2 and stats["callable"] == len(m["rows"])
        with pytest.raises(KeyError, match="nobody"):
            idx.genotype("A", "nobody", files["reads_b"])
        with pytest.raises(ValueError, match="itself"):
            idx.genotype("A", "A", files["reads_b"])
        with pytest.raises(ValueError, match="no sample file"):
            idx.genotype("A", "B", ["/nowhere/reads.fq"])
        with pytest.raises(ValueError, match="min_frac"):
            idx.genotype("A", "B", files["reads_b"], min_frac=0)
        with pytest.raises(ValueError, match="min_count"):
            idx.genotype("A", "B", files["reads_b"], min_count=0)
    finally:
        idx.close()


def test_refusals_come_before_a_context_is_made(built, tmp_path, capsys, monkeypatch):
    from panagram_amd import engine
    from panagram_amd.__main__ import main
    k, out, files = built

    def no_context(*a, **kw):
        raise AssertionError("a context was made")
    monkeypatch.setattr(engine, "Context", no_context)
    reads = files["reads_a"]
    cases = [([out, "A", "nobody", *reads], "nobody"), ([out, "A", "A", *reads], "itself"), ([out, "A", "B", "/nowhere/reads.fq"], "no sample file"),
             ([out, "A", "B", *reads, "--min-frac", "0"], "--min-frac"), ([out, "A", "B", *reads, "--min-frac", "1.5"], "--min-frac"),
             ([out, "A", "B", *reads, "--min-count", "0"], "--min-count"), ([out, "A", "B", *reads, "-k", "0"], "-k"),
             ([out, "A", "B", *reads, "-k", "33"], "-k"), ([out, "A", "B", *reads, "--sample", "mine"], "--sample")]
    for args, word in cases:
        with pytest.raises(SystemExit) as ei:
            main(["genotype"] + args)
        assert ei.value.code == 2 and word in capsys.readouterr().err, args


def test_a_genome_without_an_assembly_is_refused(built, tmp_path, capsys, monkeypatch):
    """the index's copy of the samples table names B's FASTA; with that file gone the command refuses, before a context is made"""
    import shutil
    from panagram_amd import engine
    from panagram_amd import index as pidx
    from panagram_amd.__main__ import main
    k, out, files = built
    idx = pidx.Index(out, mode="r")
    fasta = str(idx["B"].fasta)
    idx.close()
    moved = str(tmp_path / "B.fa")
    shutil.move(fasta, moved)
    try:
        monkeypatch.setattr(engine, "Context", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a context was made")))
        with pytest.raises(SystemExit) as ei:
            main(["genotype", out, "A", "B", *files["reads_a"]])
        assert ei.value.code == 2 and "no assembly FASTA" in capsys.readouterr().err
    finally:
        shutil.move(moved, fasta)
