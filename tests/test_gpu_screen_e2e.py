"""GPU: Index.screen and the `screen` subcommand on an index written by Index.run(): A, B and C with independent substitutions
(tests/place_ref.py: E2E), and as the sample the reads of a mosaic of B and C in two FASTQ files, one gzipped — or B's own FASTA.
The main table, the occupancy table and the statistics are exactly the numpy model's (tests/screen_ref.py); the donors rank above
the genome that gave nothing; an assembly recovers itself whole; the command writes the same files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import screen as scr
from tests import place_ref as pr
from tests import screen_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = pr.E2E["k"]


model = SR.e2e_model


def same(got, want, tag):
    for g, w, what in zip(got[:2], want[:2], ("main", "occupancy")):
        assert g.to_csv(sep="\t") == w.to_csv(sep="\t"), (tag, what, g.to_csv(sep="\t"), w.to_csv(sep="\t"))
    assert list(got[2]) == scr.STAT_NAMES
    for key in scr.STAT_NAMES:
        assert got[2][key] == want[2][key], (tag, key, got[2][key], want[2][key])


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("screen")
    genomes, _ = pr.e2e_genomes()
    lines = ["name\tfasta\tgff"]
    for name, contigs in zip(pr.E2E_NAMES, genomes):
        fa = tmp / f"{name}.fa"
        fa.write_bytes(po.fasta_text(pr.E2E_CHROMS, contigs))
        lines.append(f"{name}\t{fa}\t")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["A"], lowres_step=100).run()
    return out, pr.e2e_write_reads(tmp), str(tmp / "B.fa")


def _batch_bytes(reads):
    """a third of the larger file's text and a little: three FASTQ batches per file"""
    import gzip
    sizes = [len((gzip.open if p.endswith(".gz") else open)(p, "rb").read()) for p in reads]
    return max(sizes) // 3 + 1000


def test_screen_equals_the_model_and_ranks_the_donors(built, monkeypatch):
    from panagram_amd import index as pidx, place as pl
    out, reads, b_fasta = built
    idx = pidx.Index(out, mode="r")
    try:
        table = idx._full_table()
        seqsets, stats_before = dict(idx._seqsets), table.stats()
        nbatches = []
        orig_iter = pl.FastqBatches.__iter__

        def counted(self):
            n = 0
            for buf in orig_iter(self):
                n += 1
                yield buf
            nbatches.append(n)
        monkeypatch.setattr(pl.FastqBatches, "__iter__", counted)
        got = idx.screen(reads, batch_bytes=_batch_bytes(reads))  # (min_count: the default of a FASTQ sample)
        monkeypatch.undo()
        assert len(nbatches) == len(reads) and min(nbatches) >= 3  # each file once, in three batches or more
        same(got, model("reads", 2), "reads, three batches per file")
        main = got[0].set_index("genome")
        assert got[2]["min_count"] == 2 and main.loc["A", "rank"] == 3
        assert 100 * main.loc["A", "private_seen"] <= main.loc["A", "private"]
        # the table and the packed genomes are as before
        assert idx._table is table and idx._seqsets == seqsets and table.stats() == stats_before
        # one batch per file, another threshold, a selection of genomes
        got = idx.screen(reads[::-1], min_count=3, genomes=["C", "A"])
        same(got, model("reads", 3, ["C", "A"]), "selection")
        assert got[0]["genome"].tolist() == ["A", "C"]
        # B's own assembly: every k-mer of B, no private k-mer of another genome
        got = idx.screen(b_fasta)
        same(got, model(pr.e2e_genomes()[0][1], 1), "B's FASTA")
        main = got[0].set_index("genome")
        assert got[2]["min_count"] == 1 and main.loc["B", "containment"] == 1.0 and main.loc["B", "rank"] == 1
        assert main.loc["B", "private_seen"] == main.loc["B", "private"] > 0
        assert main.loc["A", "private_seen"] == 0 and main.loc["C", "private_seen"] == 0
        assert got[2]["novel_frac"] == 0.0 and got[2]["reads"] == 3
        # FASTQ and FASTA in one sample: the default threshold is the reads'
        got = idx.screen([b_fasta, reads[0]])
        assert got[2]["min_count"] == 2
        with pytest.raises(KeyError, match="nobody"):
            idx.screen(reads, genomes=["nobody"])
        with pytest.raises(ValueError, match="min_count"):
            idx.screen(reads, min_count=0)
        with pytest.raises(ValueError, match="min_count"):
            idx.screen(reads, min_count=256)
        with pytest.raises(ValueError, match="no sample file"):
            idx.screen(["/nowhere/reads.fq"])
        assert idx._table is table and idx._seqsets == seqsets and table.stats() == stats_before
    finally:
        idx.close()


def test_a_torn_last_record_raises(built, tmp_path):
    from panagram_amd import index as pidx
    out, reads, _ = built
    torn = tmp_path / "torn.fq"
    text = open(reads[0], "rb").read()
    torn.write_bytes(text[:text.rindex(b"\n+\n")])
    idx = pidx.Index(out, mode="r")
    try:
        with pytest.raises(ValueError, match="not a whole FASTQ record"):
            idx.screen([str(torn)])
    finally:
        idx.close()


def test_a_table_of_some_anchors_only_cannot_answer(built):
    from panagram_amd import index as pidx
    out, reads, _ = built
    idx = pidx.Index(out, mode="r")
    try:
        idx._table, idx._table_scope = object(), frozenset(["A"])
        with pytest.raises(RuntimeError, match="anchors"):
            idx.screen(reads)
        idx._table, idx._table_scope = None, "all"
    finally:
        idx.close()


def test_screen_subcommand_in_a_child_process(built, tmp_path):
    out, reads, _ = built
    want = model("reads", 2)
    main, occ, su = (tmp_path / n for n in ("main.tsv", "occupancy.tsv", "summary.tsv"))
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "screen", out, *reads, "-o", str(main),
                        "--occupancy", str(occ), "--summary", str(su), "--batch-bytes", str(_batch_bytes(reads))], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    wm, wo, ws = (tmp_path / n for n in ("wmain.tsv", "woccupancy.tsv", "wsummary.tsv"))
    scr.write_main(want[0], str(wm))
    scr.write_occupancy(want[1], str(wo))
    scr.write_summary(want[2], str(ws))
    assert main.read_text() == wm.read_text() and occ.read_text() == wo.read_text() and su.read_text() == ws.read_text()
    assert su.read_text().startswith(f"# reads\t{len(pr.e2e_reads())}\n")
    # the main table goes to stdout by default; a selection and a threshold
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "screen", out, *reads, "--min-count", "3",
                        "--genomes", "C,A"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    scr.write_main(model("reads", 3, ["C", "A"])[0], str(wm))
    assert r.stdout == wm.read_text()
    # an unknown genome name: an argparse error that names it
    r = subprocess.run([sys.executable, "-m", "panagram_amd", "screen", out, reads[0], "--genomes", "B,nobody"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "nobody" in r.stderr
