"""GPU: Genome.absence_runs / absence_spectrum and the `gaps` subcommand on an index written by Index.run() — the planted-variant
genomes of tests/test_gaps_cpu.py and a third, unrelated one — against tests/gaps_ref.py on the frame Index.query_bitmap
returns: labels, classes and sites included, with a budget so small that the region is cut into pieces inside the runs."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import gaps
from tests import gaps_ref as gr

pytestmark = pytest.mark.gpu

K = gr.PLANTED_K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ["chr", "start", "end", "genome", "rows", "class", "site"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("gaps")
    a, b = gr.planted_genomes()
    other = np.random.default_rng(99).integers(0, 4, gr.PLANTED_LEN, dtype=np.uint8)
    lines = ["name\tfasta"]
    for i, codes in enumerate((a, b, other)):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(["chr1"], [po.codes_to_ascii(codes)]))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def _want(idx, genomes, start, end, step, min_len, max_len, maxlen):
    """(runs frame, hist, absent, edges, rows) by the reference on query_bitmap's frame"""
    frame = idx.query_bitmap("g0", "chr1", start, end, step)
    labels = frame.index.to_numpy().astype(np.int64)
    names = list(frame.columns)
    cols = None if genomes is None else [names.index(g) for g in genomes]
    runs, hist, absent, edges = gr.ref_window(frame.to_numpy(), maxlen, cols)
    runs = runs[(runs[:, 2] >= min_len) & ((runs[:, 2] <= max_len) if max_len else True)]
    runs = runs[np.lexsort((runs[:, 0], runs[:, 1]))]
    first = labels[runs[:, 1]] if len(runs) else np.zeros(0, np.int64)
    cls, site, _ = gaps.classify(runs[:, 2], K, first)
    out = pd.DataFrame({"chr": np.full(len(runs), "chr1", object), "start": first,
                        "end": (labels[runs[:, 1] + runs[:, 2] - 1] + 1) if len(runs) else first, "genome": [names[i] for i in runs[:, 0]],
                        "rows": runs[:, 2], "class": cls if step == 1 else np.full(len(runs), "", object),
                        "site": site if step == 1 else np.full(len(runs), -1, np.int64)})
    return out, hist, absent, edges, len(frame)


def _same(got, want, tag):
    assert list(got.columns) == COLUMNS and len(got) == len(want), (tag, len(got), len(want))
    for col in ("chr", "genome", "class"):
        assert got[col].fillna("").tolist() == want[col].tolist(), (tag, col)
    for col in ("start", "end", "rows", "site"):
        assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy().astype(np.int64)), (tag, col)


def test_absence_runs_equal_the_reference_on_the_queried_bitmap(built):
    from panagram_amd import index as pidx
    idx = pidx.Index(built, mode="r")
    try:
        g = idx["g0"]
        # the planted variants, as tests/test_gaps_cpu.py pins them on the oracle's rows
        got = idx.absence_runs("g0", ["g1"])
        assert got[["start", "rows", "class", "site"]].values.tolist() == [[s, n, c, site] for s, n, c, site, _ in gr.PLANTED_RUNS]
        assert got["end"].tolist() == [s + n for s, n, *_ in gr.PLANTED_RUNS] and set(got["genome"]) == {"g1"}
        assert len(idx.absence_runs("g0", ["g0"])) == 0
        cases = [(None, None, None, 1, 1, 0), (None, 400, 2100, 1, K - 1, 0), (["g1", "g2"], 490, 1990, 1, 1, 30), (None, None, None, 7, 1, 0),
                 (["g2"], 77, None, 100, 1, 0)]
        for genomes, start, end, step, min_len, max_len in cases:
            want = _want(idx, genomes, start, end, step, min_len, max_len, 4 * K)
            tag = (genomes, start, end, step, min_len, max_len)
            _same(g.absence_runs(genomes, "chr1", start, end, step, min_len, max_len), want[0], tag)
            names = idx.genome_names if genomes is None else genomes
            cols = [list(idx.genome_names).index(x) for x in names]
            sp = gaps.spectrum_frame(want[1][cols], names)
            assert g.absence_spectrum(genomes, "chr1", start, end, step).equals(sp), tag
            # cut into pieces of 99 and of 13 rows, inside the runs (a run of 28 rows holds whole pieces of 13): the same
            for per in (99, 13):
                if per == 13 and (start is None or step != 1):
                    continue
                g.similarity_budget = per * g.nbytes * (100 if step % 100 == 0 else 1)
                try:
                    runs, spectrum, summary = g.absence_tables(genomes, "chr1", start, end, step, min_len, max_len)
                finally:
                    del g.similarity_budget
                _same(runs, want[0], tag + (per,))
                assert spectrum.equals(sp), tag + (per,)
                if step == 1:
                    su = gaps.summary_frame(want[1][cols], want[2][cols], gaps.open_rows(want[3], want[4])[cols], want[4], names, K)
                    assert summary.equals(su), tag + (per,)
    finally:
        idx.close()


def test_gaps_subcommand_in_a_child_process(built, tmp_path):
    from panagram_amd import index as pidx
    idx = pidx.Index(built, mode="r")
    try:
        want = _want(idx, None, None, None, 1, K - 1, 0, 4 * K)
        names = list(idx.genome_names)
    finally:
        idx.close()
    assert len(want[0]) >= 4
    runs, sp, su = tmp_path / "runs.tsv", tmp_path / "spectrum.tsv", tmp_path / "summary.tsv"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "gaps", built, "g0", "chr1", "-o", str(runs),
                        "--spectrum", str(sp), "--summary", str(su)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    _same(pd.read_csv(runs, sep="\t", header=None, names=COLUMNS), want[0], "-o")
    want_sp = gaps.spectrum_frame(want[1], names)
    got = pd.read_csv(sp, sep="\t")
    assert list(got.columns) == ["genome", "rows", "runs"] and got.values.tolist() == want_sp.values.tolist()
    want_su = gaps.summary_frame(want[1], want[2], gaps.open_rows(want[3], want[4]), want[4], names, K)
    got = pd.read_csv(su, sep="\t")
    assert list(got.columns) == list(want_su.columns) and got["genome"].tolist() == names
    assert np.allclose(got.iloc[:, 1:].to_numpy().astype(float), want_su.iloc[:, 1:].to_numpy().astype(float))
    assert got.loc[1, ["sub", "ins", "del_or_multi"]].tolist() == [1, 1, 2]
    # an unknown genome name: an argparse error that names it
    p = subprocess.run([sys.executable, "-m", "panagram_amd", "gaps", built, "g0", "chr1", "--genomes", "g1,nobody"], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode != 0 and "nobody" in p.stderr
