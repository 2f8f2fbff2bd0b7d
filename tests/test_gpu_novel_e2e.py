"""GPU: Index.novel and the `novel` subcommand on an index written by Index.run(): A, B and C (tests/place_ref.py: E2E), and as the
sample genome B with a planted 500-base insertion, a substitution, a deletion and a wholly novel contig — as a FASTA, and as
error-free reads of it with errors planted once each (tests/novel_ref.py).  The statistics, the spectrum, the k-mers and the
regions are exactly the numpy model's; the insertion's region has 500 bases at the planted place; of the reads at min_count 2 every
solid k-mer lies in a planted region and no planted error's k-mer is solid; the command writes the same files."""
import gzip
import os
import subprocess
import sys

import pytest

from oracle import pyoracle as po
from panagram_amd import novel as nov
from tests import novel_ref as NR
from tests import place_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = pr.E2E["k"]


def same(got, want, tag):
    assert list(got[0]) == nov.STAT_NAMES
    for key in nov.STAT_NAMES:
        assert got[0][key] == want[0][key], (tag, key, got[0][key], want[0][key])
    for g, w, what in zip(got[1:], want[1:], ("spectrum", "kmers", "regions")):
        assert (g is None) == (w is None), (tag, what)
        if w is not None:
            assert g.to_csv(sep="\t") == w.to_csv(sep="\t"), (tag, what, g.to_csv(sep="\t")[:2000], w.to_csv(sep="\t")[:2000])


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("novel")
    genomes, _ = pr.e2e_genomes()
    lines = ["name\tfasta\tgff"]
    for name, contigs in zip(pr.E2E_NAMES, genomes):
        fa = tmp / f"{name}.fa"
        fa.write_bytes(po.fasta_text(pr.E2E_CHROMS, contigs))
        lines.append(f"{name}\t{fa}\t")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["A"], lowres_step=100).run()
    sample = tmp / "sample.fa"
    sample.write_bytes(po.fasta_text(NR.E2E_SAMPLE_NAMES, NR.e2e_sample()))
    reads = NR.e2e_reads()[0]
    h = len(reads) // 2
    r1, r2 = str(tmp / "reads_1.fq"), str(tmp / "reads_2.fq.gz")
    with open(r1, "wb") as f:
        f.write(pr.fastq_text(reads[:h]))
    with gzip.open(r2, "wb") as f:
        f.write(pr.fastq_text(reads[h:])[:-1])  # (no final line feed)
    return out, str(sample), [r1, r2]


def test_novel_equals_the_model_on_the_assembly_and_on_its_reads(built):
    from panagram_amd import index as pidx
    out, sample, reads = built
    idx = pidx.Index(out, mode="r")
    try:
        table = idx._full_table()
        seqsets, stats_before = dict(idx._seqsets), table.stats()
        got = idx.novel(sample, kmers=True, regions=True)  # (min_count: the default of a FASTA sample)
        want = NR.e2e_model("fasta", 1, file=sample)
        same(got, want, "the assembly")
        st, _, kmers, regions = got
        assert st["min_count"] == 1 and st["regions"] == 4 and st["error_windows"] == 0 and st["reads"] == 4
        ins = regions.iloc[0]
        assert (ins["contig"], ins["start"], ins["bases"], ins["left_held"], ins["right_held"]) == ("s1", NR.E2E_INS_AT - K + 1, 500, 1, 1)
        assert ins["end"] == NR.E2E_INS_AT + NR.E2E_INSERTION + K - 1 and regions["bases"].tolist() == [500, 1, 0, NR.E2E_NOVEL_CONTIG]
        m = NR.e2e_model("fasta", 1, 2, file=sample)
        got = idx.novel([sample], min_bases=2, regions=True)
        same(got, (m[0], m[1], None, m[3]), "min_bases")
        assert got[0]["regions"] == 2 and got[0]["region_bases"] == 500 + NR.E2E_NOVEL_CONTIG
        planted = set(kmers["kmer"])
        # the reads, each file in three batches or more: the solid k-mers are the planted regions', no error among them
        sizes = [len((gzip.open if p.endswith(".gz") else open)(p, "rb").read()) for p in reads]
        got = idx.novel(reads, batch_bytes=max(sizes) // 3 + 1000, kmers=True)  # (min_count: the default of a FASTQ sample)
        want = NR.e2e_model("reads", 2)
        same(got, want, "the reads")
        st, _, kmers, none = got
        errors = set(nov.spell(sorted(NR.e2e_reads()[1]), K))
        assert none is None and st["min_count"] == 2 and st["solid_kmers"] == len(kmers) == want[0]["solid_kmers"]
        assert set(kmers["kmer"]) <= planted and not set(kmers["kmer"]) & errors and st["error_windows"] == len(errors)
        # one batch per file, another threshold: the errors are k-mers like any other at min_count 1
        got = idx.novel(reads[::-1], min_count=1, kmers=True)
        same(got, NR.e2e_model("reads", 1), "min_count 1")
        assert errors <= set(got[2]["kmer"])
        # B's own assembly holds nothing novel
        st = idx.novel(os.path.join(os.path.dirname(sample), "B.fa"), regions=True)
        assert st[0]["novel_kmers"] == 0 and st[0]["novel_windows"] == 0 and len(st[3]) == 0 and st[2] is None
        # FASTQ and FASTA in one sample: the default threshold is the reads'; regions need an assembly
        assert idx.novel([sample, reads[0]])[0]["min_count"] == 2
        with pytest.raises(ValueError, match="regions need an assembly"):
            idx.novel([sample, reads[0]], regions=True)
        with pytest.raises(ValueError, match="min_count"):
            idx.novel(reads, min_count=0)
        with pytest.raises(ValueError, match="no sample file"):
            idx.novel(["/nowhere/reads.fq"])
        with pytest.raises(ValueError, match="min_bases"):
            idx.novel(sample, regions=True, min_bases=-1)
        # the table and the packed genomes are as before
        assert idx._table is table and idx._seqsets == seqsets and table.stats() == stats_before
    finally:
        idx.close()


def test_novel_subcommand_in_a_child_process(built, tmp_path):
    out, sample, reads = built
    want = NR.e2e_model("fasta", 1, file=sample)
    files = {n: tmp_path / f"{n}.tsv" for n in ("spectrum", "kmers", "regions", "summary")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "novel", out, sample, "--spectrum", str(files["spectrum"]),
                        "--kmers", str(files["kmers"]), "--regions", str(files["regions"]), "--summary", str(files["summary"])], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    w = {n: tmp_path / f"w{n}.tsv" for n in files}
    nov.write_spectrum(want[1], str(w["spectrum"]))
    nov.write_kmers(want[2], str(w["kmers"]))
    nov.write_regions(want[3], str(w["regions"]))
    nov.write_summary(want[0], str(w["summary"]))
    for n in files:
        assert files[n].read_text() == w[n].read_text(), n
    assert r.stdout == w["summary"].read_text() and r.stdout.startswith("reads\t4\n")
    assert files["regions"].read_text().split("\n")[1].split("\t")[1:6] == ["s1", str(NR.E2E_INS_AT - K + 1), str(NR.E2E_INS_AT + 500 + K - 1), str(500 + K - 1), "500"]
    # the reads at --min-count 2, in batches
    want = NR.e2e_model("reads", 2)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "novel", out, *reads, "--min-count", "2", "--kmers",
                        str(files["kmers"]), "--batch-bytes", "300000"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    nov.write_kmers(want[2], str(w["kmers"]))
    nov.write_summary(want[0], str(w["summary"]))
    assert files["kmers"].read_text() == w["kmers"].read_text() and r.stdout == w["summary"].read_text()
    # regions of reads: an argparse error before any work
    r = subprocess.run([sys.executable, "-m", "panagram_amd", "novel", out, reads[0], "--regions", str(tmp_path / "no.tsv")], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "needs an assembly" in r.stderr and not (tmp_path / "no.tsv").exists()
