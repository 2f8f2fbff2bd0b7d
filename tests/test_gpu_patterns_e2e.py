"""GPU: Genome.pattern_spectrum / pattern_counts and the `patterns` subcommand on indexes written by Index.run(), against
DataFrame.value_counts() of the frames Index.query_bitmap returns, and against two tables the index already holds."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import patterns

pytestmark = pytest.mark.gpu

K = 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [6000, 2500]
COLUMNS = ["pattern", "n", "rows", "frac"]


@pytest.fixture(scope="module", params=[9, 33], ids=["N9", "N33"])
def built(request, tmp_path_factory):
    from panagram_amd import index as pidx
    n = request.param
    tmp = tmp_path_factory.mktemp(f"patterns_n{n}")
    chroms = [f"chr{i + 1}" for i in range(len(LENS))]
    lines = ["name\tfasta"]
    for i, g in enumerate(po.synth_genomes(n, LENS, 0.02, 57 + n)):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(chroms, [po.codes_to_ascii(c) for c in g]))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out, n


def _want(idx, genomes, chrom, start, end, step, top=None, min_rows=1):
    """value_counts() of the queried frames' selected columns, as spectrum_frame lays it out"""
    names = list(idx.genome_names)
    cols = names if genomes is None else [g for g in names if g in genomes]
    chroms = list(idx["g0"].chrs.index) if chrom is None else [chrom]
    frame = pd.concat([idx.query_bitmap("g0", c, start, end, step)[cols] for c in chroms], ignore_index=True)
    vc = frame.astype(np.int64).value_counts()
    total = len(frame)
    rows = [("".join(str(int(b)) for b in pat), int(sum(pat)), int(v), int(v) / total) for pat, v in vc.items()]
    want = pd.DataFrame(rows, columns=COLUMNS).astype({"n": np.int64, "rows": np.int64, "frac": np.float64})
    want = want[want["rows"] >= min_rows].sort_values(["rows", "pattern"], ascending=[False, True]).reset_index(drop=True)
    return want if top is None else want.iloc[:top]


def _same(got, want, tag):
    assert list(got.columns) == COLUMNS, tag
    assert len(got) == len(want), (tag, len(got), len(want))
    assert got["pattern"].tolist() == want["pattern"].tolist(), tag
    for col in ("n", "rows"):
        assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy()), (tag, col)
    assert np.allclose(got["frac"].to_numpy(), want["frac"].to_numpy(), rtol=1e-12, atol=0), tag


def _regions(g):
    return [("chr1", 1234, 5678), ("chr2", 77, int(g.chrs.loc["chr2", "size"])), (None, None, None)]


def test_pattern_spectrum_equals_value_counts_of_the_queried_bitmap(built):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        some = ["g3", "g1", f"g{n - 1}"]
        want = _want(idx, None, None, None, None, 1)
        print(f"N = {n}: {len(want)} patterns in {want['rows'].sum()} rows of the whole genome at step 1")
        assert len(want) >= 20  # the input stays non-trivial
        for genomes in (None, some):
            for step in (1, 7, 100):
                for chrom, start, end in _regions(g):
                    got = idx.pattern_spectrum("g0", genomes, chrom, start, end, step)
                    _same(got, _want(idx, genomes, chrom, start, end, step), (genomes, chrom, start, end, step))
        _same(g.pattern_spectrum(None, "chr1", top=5, min_rows=3), _want(idx, None, "chr1", None, None, 1, 5, 3), "top, min_rows")
        # cut into pieces of a few rows: the same
        for chrom, start, end, step in [("chr1", 1234, 5678, 1), ("chr1", 1234, 5678, 7), ("chr2", 77, None, 100), (None, None, None, 1)]:
            whole = g.pattern_spectrum(some, chrom, start, end, step)
            g.similarity_budget = 1000 * g.nbytes
            try:
                _same(g.pattern_spectrum(some, chrom, start, end, step), whole, ("pieces", chrom, start, end, step))
                _same(g.pattern_spectrum(None, chrom, start, end, step), _want(idx, None, chrom, start, end, step),
                      ("pieces, all", chrom, start, end, step))
            finally:
                del g.similarity_budget
        with pytest.raises(ValueError, match="nobody"):
            g.pattern_spectrum(["nobody"])
        with pytest.raises(ValueError, match="twice"):
            g.pattern_spectrum(["g1", "g1"])
        with pytest.raises(KeyError):
            g.pattern_spectrum(chrom="chr9")
        with pytest.raises(ValueError):
            g.pattern_spectrum(top=-1)
    finally:
        idx.close()


def test_spectrum_agrees_with_the_bins_and_the_pair_counts(built):
    """two invariants that need no model, at step 1 over the whole genome and all genomes: the rows by number of genomes are
    the column sums of bitsum.bins.tsv, and the rows of the patterns that hold genome g are the pair counts' diagonal"""
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        keys, counts, selected = idx.pattern_counts("g0")
        assert selected == list(idx.genome_names) and len(selected) == n
        bins = pd.read_table(g.bins_fname)
        want_occ = bins[[str(i) for i in range(n + 1)]].to_numpy().astype(np.int64).sum(axis=0)
        assert np.array_equal(patterns.occupancy(keys, counts, n), want_occ)
        frame = patterns.spectrum_frame(keys, counts, selected)
        assert np.array_equal(frame.groupby("n")["rows"].sum().reindex(range(n + 1), fill_value=0).to_numpy(), want_occ)
        diag = np.diag(idx.pair_counts("g0").to_numpy()).astype(np.int64)
        held = np.array([int(counts[(keys >> np.uint64(i)) & np.uint64(1) == 1].sum()) for i in range(n)], np.int64)
        assert np.array_equal(held, diag) and held[0] == int(counts.sum())  # (the anchor genome holds every row)
    finally:
        idx.close()


def _run(args):
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "patterns"] + args, cwd=ROOT,
                          capture_output=True, text=True)


def test_patterns_subcommand_in_a_child_process(built, tmp_path):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        names = list(idx.genome_names)
        want = idx.pattern_spectrum("g0", None, "chr2", 100, 2400, 7)
        want_cut = idx.pattern_spectrum("g0", ["g1", "g2", "g5"], None, None, None, 1, top=4, min_rows=2)
        keys, counts, selected = idx.pattern_counts("g0", ["g1", "g2", "g5"])
    finally:
        idx.close()
    assert len(want) > 3 and len(want_cut) == 4
    f = tmp_path / "spectrum.tsv"
    p = _run([out, "g0", "chr2", "100", "2400", "7", "-o", str(f)])
    assert p.returncode == 0, p.stderr[-2000:]
    assert f.read_text().splitlines()[0] == "pattern\tn\trows\tfrac\tgenomes"
    got = pd.read_csv(f, sep="\t", dtype={"pattern": str, "genomes": str})
    _same(got[COLUMNS], want, "-o")
    for pat, present in zip(got["pattern"], got["genomes"]):
        assert present == (",".join(g for g, b in zip(names, pat) if b == "1") or "-")
    # stdout, the whole genome, a selection, --top and --min-rows
    p = _run([out, "g0", "--whole", "--genomes", "g5,g1,g2", "--top", "4", "--min-rows", "2"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln.split("\t") for ln in p.stdout.splitlines() if ln.count("\t") == 4]
    assert lines[0] == COLUMNS + ["genomes"]
    got = pd.DataFrame(lines[1:], columns=lines[0]).astype({"n": np.int64, "rows": np.int64, "frac": np.float64})
    _same(got[COLUMNS], want_cut, "stdout")
    # --occupancy
    p = _run([out, "g0", "--whole", "--genomes", "g1,g2,g5", "--occupancy", "-o", str(f)])
    assert p.returncode == 0, p.stderr[-2000:]
    got = pd.read_csv(f, sep="\t")
    assert list(got.columns) == ["n", "rows"] and got["n"].tolist() == [0, 1, 2, 3]
    assert np.array_equal(got["rows"].to_numpy(), patterns.occupancy(keys, counts, 3))
    # an unknown genome name: an argparse error that names it and lists the index's
    p = _run([out, "g0", "chr1", "--genomes", "g1,nobody"])
    assert p.returncode != 0 and "nobody" in p.stderr and "g0, g1" in p.stderr
