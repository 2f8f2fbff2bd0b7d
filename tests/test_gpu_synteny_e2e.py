"""GPU: Index.synteny and the `synteny` subcommand on an index written by Index.run() — the planted genomes of
tests/synteny_ref.py (a translocation to the other chromosome and an inversion) and a third, unrelated one — against the numpy
model's segments; the chromosome lists, --min-len and --summary against the unrestricted run."""
import os
import subprocess
import sys

import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import synteny
from tests import synteny_ref as sr

pytestmark = pytest.mark.gpu

K = sr.PLANTED_K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROMS = ["chr1", "chr2"]


def _genomes():
    x, y = sr.planted_contigs()
    other = [sr.random_codes(800, 98), sr.random_codes(500, 99)]
    return [[sr.ascii_of(c) for c in g] for g in ([x, y], sr.planted_rearranged(x, y), other)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("synteny")
    lines = ["name\tfasta"]
    for i, contigs in enumerate(_genomes()):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(CHROMS, contigs))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def _want(a, b, k, pick_a=(0, 1), pick_b=(0, 1), min_len=1):
    """the model's segment table of genomes a and b restricted to some chromosomes"""
    g = _genomes()
    ca, cb = [g[a][i] for i in pick_a], [g[b][i] for i in pick_b]
    runs, mated = sr.segments(ca, cb, k)
    return sr.segment_rows(runs, k, [CHROMS[i] for i in pick_a], [len(c) for c in cb], [CHROMS[i] for i in pick_b], min_len), mated


def _unique(g, k, pick=(0, 1)):
    """the positions of a genome whose k-mer occurs once in it, both strands counted, by the model"""
    keys = sr.side_kmers([_genomes()[g][i] for i in pick], k)[0]
    return len(sr.unique_of(keys)[0])


def _rows(frame):
    assert list(frame.columns) == synteny.COLUMNS
    return [tuple(r) for r in frame.values.tolist()]


def test_index_synteny_equals_the_model(built):
    from panagram_amd import index as pidx
    idx = pidx.Index(built, mode="r")
    try:
        want, mated = _want(0, 1, K)
        assert want[1] == ("chr1", 200, 500, "chr2", 300, 600, "+", 300 - K + 1) and ("chr2", 100, 140, "chr2", 100, 140, "-", 40 - K + 1) in want
        full = idx.synteny("g0", "g1")
        assert _rows(full) == want
        seg, summary, totals = idx.synteny_tables("g0", "g1")
        assert _rows(seg) == want and summary.iloc[-1].tolist() == ["*", "*", "*", len(want), mated]
        assert list(totals.columns) == synteny.TOTALS_COLUMNS
        assert totals.values.tolist() == [["A", "g0", _unique(0, K), mated], ["B", "g1", _unique(1, K), mated]]
        assert mated < _unique(1, K) < sum(len(c) - K + 1 for c in _genomes()[1]) + 1
        t = idx.synteny_tables("g0", "g1", chroms_a=["chr2"], k=8)[2]
        assert t.values.tolist() == [["A", "g0", _unique(0, 8, (1,)), _want(0, 1, 8, pick_a=(1,))[1]],
                                     ["B", "g1", _unique(1, 8), _want(0, 1, 8, pick_a=(1,))[1]]] and t["unique"][0] < 700 - 8 + 1
        assert summary.equals(synteny.summary_frame(full))
        # the other direction, another k (the table of the index's k-mers is not read), and a pair that shares nothing
        assert _rows(idx.synteny("g1", "g0")) == _want(1, 0, K)[0]
        assert _rows(idx.synteny("g0", "g1", k=21)) == _want(0, 1, 21)[0]
        assert _rows(idx.synteny("g0", "g1", k=8)) == _want(0, 1, 8)[0]
        assert len(idx.synteny("g0", "g2")) == 0
        # chromosome lists: every k-mer of these genomes is unique, so a restricted run is the unrestricted one's lines
        only_a = idx.synteny("g0", "g1", chroms_a=["chr2"])
        assert _rows(only_a) == _want(0, 1, K, pick_a=(1,))[0] == [r for r in want if r[0] == "chr2"]
        only_b = idx.synteny("g0", "g1", chroms_b=["chr1"])
        assert _rows(only_b) == _want(0, 1, K, pick_b=(0,))[0] == [r for r in want if r[3] == "chr1"]
        both = idx.synteny("g0", "g1", chroms_a=["chr1"], chroms_b=["chr2"], min_len=1)
        assert _rows(both) == [r for r in want if r[0] == "chr1" and r[3] == "chr2"]
        assert _rows(idx.synteny("g0", "g1", min_len=100)) == [r for r in want if r[7] >= 100] == _want(0, 1, K, min_len=100)[0]
        with pytest.raises(ValueError, match="chr9"):
            idx.synteny("g0", "g1", chroms_a=["chr9"])
        with pytest.raises(KeyError):
            idx.synteny("g0", "nobody")
        with pytest.raises(ValueError):
            idx.synteny("g0", "g1", k=33)
    finally:
        idx.close()


def test_synteny_subcommand_in_a_child_process(built, tmp_path):
    want, mated = _want(0, 1, K)
    seg, summ = tmp_path / "seg.tsv", tmp_path / "summary.tsv"
    base = ["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "synteny", built, "g0", "g1"]
    p = subprocess.run(base + ["-o", str(seg), "--summary", str(summ)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = pd.read_csv(seg, sep="\t", header=None, names=synteny.COLUMNS)
    assert _rows(got) == want
    assert [tuple(r) for r in got.sort_values(["chrA", "startA"], kind="stable").values.tolist()] == want  # sorted by (chrA, startA)
    s = pd.read_csv(summ, sep="\t", comment="#")
    assert list(s.columns) == synteny.SUMMARY_COLUMNS
    head = [ln[2:].split("\t") for ln in open(summ).read().splitlines() if ln.startswith("# ")]
    assert head == [synteny.TOTALS_COLUMNS, ["A", "g0", str(_unique(0, K)), str(mated)], ["B", "g1", str(_unique(1, K)), str(mated)]]
    assert s.values.tolist() == synteny.summary_frame(got).values.tolist() and s.iloc[-1].tolist() == ["*", "*", "*", len(want), mated]
    # the chromosome lists and --min-len together, to stdout: the lines of the unrestricted run that they leave
    p = subprocess.run(base + ["--chroms-a", "chr1,chr2", "--chroms-b", "chr2", "--min-len", "30", "--summary", str(summ)], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [tuple(int(v) if v.isdigit() else v for v in ln.split("\t")) for ln in p.stdout.splitlines()]
    left = [r for r in want if r[3] == "chr2" and r[7] >= 30]
    assert lines == left and 0 < len(left) < len(want)
    s = pd.read_csv(summ, sep="\t", comment="#")
    assert s.iloc[-1].tolist() == ["*", "*", "*", len(left), sum(r[7] for r in left)]
    # an unknown genome: an argparse error that names it
    p = subprocess.run([sys.executable, "-m", "panagram_amd", "synteny", built, "g0", "nobody"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "nobody" in p.stderr
