"""GPU: Index.place and the `place` subcommand on an index written by Index.run(): anchor A, B and C with independent
substitutions, and the reads of a mosaic sample — B's sequence on the first half of each long contig, C's on the second
(tests/place_ref.py: E2E) — in two FASTQ files, one gzipped.  The main table, the matrix and the summary are exactly the numpy
model's, every bin well inside one donor's segment names its donor, and the command writes the same files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import place as pl
from tests import place_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [[0], [1, 2]]  # the chromosome batches PLACE_BUDGET forces: chr1 alone (29 980 one-byte rows), chr2 and chr3 together
PLACE_BUDGET = 30000


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("place")
    genomes, _ = pr.e2e_genomes()
    lines = ["name\tfasta\tgff"]
    for name, contigs in zip(pr.E2E_NAMES, genomes):
        fa = tmp / f"{name}.fa"
        fa.write_bytes(po.fasta_text(pr.E2E_CHROMS, contigs))
        lines.append(f"{name}\t{fa}\t")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=pr.E2E["k"], anchor_genomes=["A"], lowres_step=100).run()
    return out, pr.e2e_write_reads(tmp)


def _batch_bytes(reads):
    """a third of the larger file's text and a little: three FASTQ batches per file"""
    import gzip
    sizes = [len((gzip.open if p.endswith(".gz") else open)(p, "rb").read()) for p in reads]
    return max(sizes) // 3 + 1000


def _same(got, want, tag):
    for g, w, what in zip(got[:3], want[:3], ("main", "matrix", "summary")):
        assert g.to_csv(sep="\t") == w.to_csv(sep="\t"), (tag, what)
    for key in ("reads", "read_bases", "hits", "depth_mode", "min_count"):
        assert int(got[3][key]) == int(want[3][key]), (tag, key, got[3][key], want[3][key])
    assert np.array_equal(got[3]["depth_hist"], want[3]["depth_hist"]), tag


def test_place_equals_the_model_and_names_the_donors(built, monkeypatch):
    from panagram_amd import index as pidx
    out, reads = built
    p = pr.E2E
    idx = pidx.Index(out, mode="r")
    try:
        batches = []
        orig = pidx.Genome._place_batches
        monkeypatch.setattr(pidx.Genome, "_place_batches", lambda self, chroms: batches.append(orig(self, chroms)) or batches[-1])
        monkeypatch.setattr(pidx.Genome, "place_budget", PLACE_BUDGET)
        nbatches = []
        orig_iter = pl.FastqBatches.__iter__

        def counted(self):
            n = 0
            for buf in orig_iter(self):
                n += 1
                yield buf
            nbatches.append(n)
        monkeypatch.setattr(pl.FastqBatches, "__iter__", counted)
        got = idx.place("A", reads, bin_size=p["bin_size"], min_count=p["min_count"], batch_bytes=_batch_bytes(reads))
        assert batches == [[[pr.E2E_CHROMS[i] for i in b] for b in BATCHES]]
        assert len(nbatches) == 2 * len(reads) and min(nbatches) >= 3  # each file in three batches or more, once per chromosome batch
        _same(got, pr.e2e_model(batches=BATCHES), "two chromosome batches, three FASTQ batches")
        main = got[0]
        best = {(c, s): b for c, s, b in zip(main["chrom"], main["start"], main["best"])}
        for chrom, start, donor in pr.e2e_donor_bins():
            assert best[(chrom, start)] == donor, (chrom, start, donor)
        assert not idx._seqsets  # (what the call loaded it dropped again)
        monkeypatch.undo()
        # one chromosome batch, one FASTQ batch per file, a selection of chromosomes and genomes, another min_count and bin size
        got = idx.place("A", reads[::-1], chroms=["chr3", "chr1"], bin_size=7000, min_count=3, genomes=["C", "A"])
        want = pr.e2e_model(chroms=["chr1", "chr3"], genomes=["C", "A"], min_count=3, bin_size=7000, batches=[[0], [2]])
        _same(got, want, "selection")  # (chr1 and chr3 are no neighbours in the file: two batches)
        assert got[1].columns.tolist() == ["A", "C"] and set(got[0]["chrom"]) == {"chr1", "chr3"}
        with pytest.raises(KeyError, match="nobody"):
            idx.place("A", reads, genomes=["nobody"])
        with pytest.raises(KeyError, match="chrZ"):
            idx.place("A", reads, chroms=["chrZ"])
        with pytest.raises(KeyError, match="Z"):
            idx.place("Z", reads)
        with pytest.raises(ValueError, match="bitmap"):
            idx.place("B", reads)  # (no anchor: it has no rows)
        with pytest.raises(ValueError, match="min_count"):
            idx.place("A", reads, min_count=0)
        with pytest.raises(ValueError, match="no read file"):
            idx.place("A", ["/nowhere/reads.fq"])
    finally:
        idx.close()


def test_a_torn_last_record_raises(built, tmp_path):
    from panagram_amd import index as pidx
    out, reads = built
    torn = tmp_path / "torn.fq"
    text = open(reads[0], "rb").read()
    torn.write_bytes(text[:text.rindex(b"\n+\n")])
    idx = pidx.Index(out, mode="r")
    try:
        with pytest.raises(ValueError, match="not a whole FASTQ record"):
            idx.place("A", [str(torn)], chroms=["chr3"])
    finally:
        idx.close()


def test_place_subcommand_in_a_child_process(built, tmp_path):
    out, reads = built
    p = pr.E2E
    want = pr.e2e_model()
    main, mx, su = (tmp_path / n for n in ("main.tsv", "matrix.tsv", "summary.tsv"))
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "place", out, "A", *reads, "--bin-size",
                        str(p["bin_size"]), "--min-count", str(p["min_count"]), "-o", str(main), "--matrix", str(mx), "--summary", str(su),
                        "--batch-bytes", str(_batch_bytes(reads))], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    wm, wx, ws = (tmp_path / n for n in ("wmain.tsv", "wmatrix.tsv", "wsummary.tsv"))
    pl.write_main(want[0], str(wm))
    pl.write_matrix(want[1], str(wx))
    pl.write_summary(want[2], want[3], str(ws))
    assert main.read_text() == wm.read_text() and mx.read_text() == wx.read_text() and su.read_text() == ws.read_text()
    best = {(l.split("\t")[0], int(l.split("\t")[1])): l.split("\t")[5] for l in main.read_text().split("\n")[1:-1]}
    for chrom, start, donor in pr.e2e_donor_bins():
        assert best[(chrom, start)] == donor
    assert su.read_text().startswith(f"# reads\t{len(pr.e2e_reads())}\n")
    # an unknown genome name: an argparse error that names it
    r = subprocess.run([sys.executable, "-m", "panagram_amd", "place", out, "A", reads[0], "--genomes", "B,nobody"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "nobody" in r.stderr
