"""GPU: Genome.find_pattern / pattern_density and the `find` subcommand on indexes written by Index.run(), against the same
rule evaluated in numpy on the frame Index.query_bitmap returns — labels included."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import find

pytestmark = pytest.mark.gpu

K = 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [6000, 2500]
# (have, lack, min_have, max_lack): the reference's exact expression, and a quorum rule
RULES = {"exact": (["g1"], ["g2"], None, 0),
         "quorum": (["g1", "g2", "g3", "g4"], ["g5", "g6", "g7", "g8"], 3, 1)}


@pytest.fixture(scope="module", params=[9, 33], ids=["N9", "N33"])
def built(request, tmp_path_factory):
    from panagram_amd import index as pidx
    n = request.param
    tmp = tmp_path_factory.mktemp(f"find_n{n}")
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


def _match(frame, have, lack, min_have, max_lack):
    """the rule on a query_bitmap frame -> one bool per row"""
    nh = frame[list(have)].to_numpy().astype(np.int64).sum(axis=1)
    nl = frame[list(lack)].to_numpy().astype(np.int64).sum(axis=1) if len(lack) else np.zeros(len(frame), np.int64)
    return (nh >= (len(have) if min_have is None else min_have)) & (nl <= max_lack)


def _runs_frame(chrom, frame, m):
    """chr, start, end, rows of the maximal runs of m, labelled as the frame's index labels its rows"""
    d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
    a, b = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    labels = frame.index.to_numpy().astype(np.int64)
    return pd.DataFrame({"chr": np.full(len(a), chrom, object), "start": labels[a], "end": labels[b - 1] + 1, "rows": b - a})


def _want(idx, rule, chrom, start, end, step):
    chroms = list(idx["g0"].chrs.index) if chrom is None else [chrom]
    parts, rows, matched = [], 0, 0
    for c in chroms:
        frame = idx.query_bitmap("g0", c, start, end, step)
        m = _match(frame, *rule)
        parts.append(_runs_frame(c, frame, m))
        rows += len(m)
        matched += int(m.sum())
    return pd.concat(parts, ignore_index=True), rows, matched


def _same(got, want, tag):
    assert list(got.columns) == ["chr", "start", "end", "rows"], tag
    assert len(got) == len(want), (tag, len(got), len(want))
    assert got["chr"].tolist() == want["chr"].tolist(), tag
    for col in ("start", "end", "rows"):
        assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy().astype(np.int64)), (tag, col)


def _regions(g):
    size, size2 = int(g.chrs.loc["chr1", "size"]), int(g.chrs.loc["chr2", "size"])
    return [("chr1", None, None), ("chr1", 1234, 5678), ("chr2", 77, size2), ("chr1", size - 1, size), (None, None, None)]


def test_find_pattern_equals_the_rule_on_the_queried_bitmap(built):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        for name, rule in RULES.items():
            # the inputs stay non-trivial: many runs, neither every row nor none
            want, rows, matched = _want(idx, rule, "chr1", None, None, 1)
            print(f"N = {n}, {name}: {len(want)} runs, {matched} of {rows} rows match on chr1 at step 1")
            assert len(want) >= 20 and 0 < matched < rows, (name, len(want), matched, rows)
            for step in (1, 7, 100, 300):
                for chrom, start, end in _regions(g):
                    want, _, _ = _want(idx, rule, chrom, start, end, step)
                    got = idx.find_pattern("g0", rule[0], rule[1], rule[2], rule[3], chrom, start, end, step)
                    _same(got, want, (name, chrom, start, end, step))
        # cut into pieces of a few rows: the same (runs joined across the pieces' edges)
        rule = RULES["quorum"]
        for chrom, start, end, step in [("chr1", 1234, 5678, 1), ("chr1", 1234, 5678, 7), ("chr2", 77, None, 300), (None, None, None, 1)]:
            whole = g.find_pattern(*rule, chrom, start, end, step)
            g.similarity_budget = 1000 * g.nbytes
            try:
                _same(g.find_pattern(*rule, chrom, start, end, step), whole, ("pieces", chrom, start, end, step))
            finally:
                del g.similarity_budget
    finally:
        idx.close()


def test_min_len_and_max_gap_equal_merge_runs_of_the_plain_result(built):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        rule = RULES["exact"]
        for step in (1, 7):
            plain = g.find_pattern(*rule, "chr1", 100, None, step)
            for min_len, max_gap in [(1, 1), (3, 0), (5, 2), (40, 10)]:
                got = g.find_pattern(*rule, "chr1", 100, None, step, min_len, max_gap)
                # the plain runs back in sampled rows (label = 100 + j * step)
                a = (plain["start"].to_numpy() - 100) // step
                b = (plain["end"].to_numpy() - 1 - 100) // step + 1
                s, e, rows = find.merge_runs(a, b, min_len, max_gap)
                want = pd.DataFrame({"chr": np.full(len(s), "chr1", object), "start": 100 + s * step, "end": 100 + (e - 1) * step + 1,
                                     "rows": rows})
                _same(got, want, (step, min_len, max_gap))
        with pytest.raises(ValueError):
            g.find_pattern(["g1"], ["g1"])
        with pytest.raises(ValueError):
            g.find_pattern(["nobody"])
        with pytest.raises(KeyError):
            g.find_pattern(["g1"], chrom="chr9")
    finally:
        idx.close()


def test_pattern_density_equals_binned_sums_of_the_match_vector(built):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        for name, rule in RULES.items():
            for step in (1, 100):
                got = idx.pattern_density("g0", rule[0], rule[1], rule[2], rule[3], None, step, 1000)
                assert list(got.columns) == ["chr", "start", "matched", "rows"]
                parts = []
                for c in g.chrs.index:
                    frame = idx.query_bitmap("g0", c, None, None, step)
                    m = _match(frame, *rule)
                    b = frame.index.to_numpy().astype(np.int64) // 1000
                    ub = np.unique(b)
                    parts.append(pd.DataFrame({"chr": np.full(len(ub), c, object), "start": ub * 1000,
                                               "matched": np.bincount(b, weights=m)[ub].astype(np.int64),
                                               "rows": np.bincount(b)[ub]}))
                want = pd.concat(parts, ignore_index=True)
                assert got["chr"].tolist() == want["chr"].tolist(), (name, step)
                for col in ("start", "matched", "rows"):
                    assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy().astype(np.int64)), (name, step, col)
                assert 0 < got["matched"].sum() < got["rows"].sum()
        one = g.pattern_density(["g1"], ["g2"], chroms=["chr2"], step=1, bin_size=1000)
        assert set(one["chr"]) == {"chr2"} and len(one) == -(-int(g.chrs.loc["chr2", "size"]) // 1000)
    finally:
        idx.close()


def _run(args):
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "find"] + args, cwd=ROOT,
                          capture_output=True, text=True)


def test_find_subcommand_in_a_child_process(built, tmp_path):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        want = idx.find_pattern("g0", *RULES["quorum"], "chr2", 100, 2400, 1, 2, 1)
        want_all = idx.find_pattern("g0", *RULES["exact"])
        want_density = idx.pattern_density("g0", *RULES["exact"], None, 1, 1000)
    finally:
        idx.close()
    assert len(want) > 0
    f = tmp_path / "runs.tsv"
    quorum = ["--have", "g1,g2,g3,g4", "--lack", "g5,g6,g7,g8", "--min-have", "3", "--max-lack", "1"]
    p = _run([out, "g0", "chr2", "100", "2400", "1"] + quorum + ["--min-len", "2", "--max-gap", "1", "-o", str(f)])
    assert p.returncode == 0, p.stderr[-2000:]
    got = pd.read_csv(f, sep="\t", header=None, names=["chr", "start", "end", "rows"])
    _same(got, want, "-o")
    # stdout, the whole genome
    p = _run([out, "g0", "--whole", "--have", "g1", "--lack", "g2"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln.split("\t") for ln in p.stdout.splitlines() if ln.count("\t") == 3 and ln.startswith("chr")]
    got = pd.DataFrame(lines, columns=["chr", "start", "end", "rows"]).astype({"start": np.int64, "end": np.int64, "rows": np.int64})
    _same(got, want_all, "stdout")
    # --density
    p = _run([out, "g0", "--whole", "--have", "g1", "--lack", "g2", "--density", "1000", "-o", str(f)])
    assert p.returncode == 0, p.stderr[-2000:]
    got = pd.read_csv(f, sep="\t", header=None, names=["chr", "start", "matched", "rows"])
    assert len(want_density) > 0 and got["chr"].tolist() == want_density["chr"].tolist()
    for col in ("start", "matched", "rows"):
        assert np.array_equal(got[col].to_numpy(), want_density[col].to_numpy()), col
    # an unknown genome name: an argparse error that names it
    p = _run([out, "g0", "chr1", "--have", "g1,nobody"])
    assert p.returncode != 0 and "nobody" in p.stderr
