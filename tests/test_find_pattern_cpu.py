"""CPU: the host side of Genome.find_pattern / pattern_density — which rows they hand to the engine (exactly query()'s), the
labels, the budgeted pieces and their join, chromosomes kept apart — with a numpy stand-in for the rows container
(tests/find_ref.py computes what k_find_runs would) and test_pair_counts_cpu.py's in-memory index."""
import numpy as np
import pandas as pd
import pytest

from panagram_amd import find
from tests import rows_craft as rc
from tests.find_ref import ref_find_runs
from tests.test_pair_counts_cpu import LOW, REGIONS, SIZES, _scene


def _cols(n, words):
    return np.flatnonzero(rc.keep_bits(n, words)).tolist()


class _Rows:
    """stands in for a rows container: contig c = rows[c]"""

    def __init__(self, rows, n, bstep):
        self.rows, self.n, self.bstep = rows, n, bstep

    def find_runs(self, contigs, starts, ends, have_words, lack_words, min_have, max_lack, step=1, stride=1):
        assert step == self.bstep
        out, matched = [], []
        for i, (c, s, e) in enumerate(zip(contigs, starts, ends)):
            assert e == 0 or (int(e) - 1) * stride < len(self.rows[c])  # every sampled row inside the contig
            a, b, m = ref_find_runs(self.rows[c], self.n, s, e, stride, _cols(self.n, have_words), _cols(self.n, lack_words),
                                    min_have, max_lack)
            out.append(np.stack([np.full(len(a), i, np.int64), a, b], axis=1))
            matched.append(m)
        return np.concatenate(out).reshape(-1, 3), np.array(matched, np.uint64)

    def find_counts(self, *args, **kw):
        runs, matched = self.find_runs(*args, **kw)
        return np.bincount(runs[:, 0], minlength=len(matched)).astype(np.uint64), matched

    def close(self):
        pass


def _find_scene(monkeypatch, n):
    idx, g, log = _scene(monkeypatch, n)
    region = g._rows_region

    def rows_region(bstep, row0, nrows):
        r = region(bstep, row0, nrows)  # (checks that the region stays inside the file, and logs it)
        return _Rows([r.rows], n, bstep)

    def rows_from_disk(chroms, step=1):
        return _Rows([rc.pack(g.query(c, None, None, step).to_numpy()) for c in chroms], n, step)
    g._rows_region, g._rows_from_disk = rows_region, rows_from_disk
    return idx, g, log


RULES = [(["g1"], ["g2"], None, 0), (["g1", "g2", "g3", "g4"], ["g5", "g6", "g7", "g8"], 2, 2), ([1, 10], (), 1, 0)]


def _match(frame, have, lack, min_have, max_lack):
    cols = lambda gs: [g if isinstance(g, str) else frame.columns[g] for g in gs]
    nh = frame[cols(have)].to_numpy().astype(np.int64).sum(axis=1)
    nl = frame[cols(lack)].to_numpy().astype(np.int64).sum(axis=1)
    return (nh >= (len(have) if min_have is None else min_have)) & (nl <= max_lack)


def _want(g, rule, chrom, start, end, step):
    parts = []
    for c in (list(SIZES) if chrom is None else [chrom]):
        frame = g.query(c, start, end, step)
        d = np.diff(np.concatenate([[0], _match(frame, *rule).astype(np.int8), [0]]))
        a, b = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
        labels = frame.index.to_numpy().astype(np.int64)
        parts.append(pd.DataFrame({"chr": np.full(len(a), c, object), "start": labels[a], "end": labels[b - 1] + 1, "rows": b - a}))
    return pd.concat(parts, ignore_index=True)


def _same(got, want, tag):
    assert list(got.columns) == ["chr", "start", "end", "rows"] and len(got) == len(want), (tag, len(got), len(want))
    assert got["chr"].tolist() == want["chr"].tolist(), tag
    for col in ("start", "end", "rows"):
        assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy().astype(np.int64)), (tag, col)


@pytest.mark.parametrize("step", [1, 7, 100, 300])
def test_find_pattern_selects_and_labels_querys_rows(monkeypatch, step):
    idx, g, log = _find_scene(monkeypatch, 11)
    total = 0
    for rule in RULES:
        for chrom, start, end in REGIONS + [(None, None, None)]:
            got = g.find_pattern(*rule, chrom, start, end, step)
            _same(got, _want(g, rule, chrom, start, end, step), (rule, chrom, start, end, step))
            _same(idx.find_pattern("g0", *rule, chrom, start, end, step), got, "Index.find_pattern")
            total += len(got)
    assert total > 20


@pytest.mark.parametrize("step,rows_per_piece", [(7, 50), (1, 97), (300, 5), (300, 4), (1, 1)])
def test_tiny_budget_joins_runs_across_pieces(monkeypatch, step, rows_per_piece):
    idx, g, log = _find_scene(monkeypatch, 11)
    bstep = LOW if step % LOW == 0 else 1
    rule = ([1, 10], (), 1, 0)  # (three rows in four match: long runs, many across a piece's edge)
    want = g.find_pattern(*rule, "c1", 3, 1230, step)
    n0 = len(log)
    g.similarity_budget = rows_per_piece * g.nbytes * bstep
    got = g.find_pattern(*rule, "c1", 3, 1230, step)
    assert len(log) - n0 >= 3 and all(nrows <= rows_per_piece for _, _, nrows in log[n0:])
    _same(got, want, (step, rows_per_piece))
    _same(want, _want(g, rule, "c1", 3, 1230, step), "uncut")
    # some run crosses a piece's edge (a piece begins at the first sampled row at or behind a multiple of rows_per_piece)
    stride = step // bstep
    a, b = (want["start"].to_numpy() - 3) // step, (want["end"].to_numpy() - 1 - 3) // step + 1
    edges = -(-np.arange(rows_per_piece, stride * int(b.max()), rows_per_piece) // stride)
    assert any(((a < x) & (x < b)).any() for x in edges)
    # every chromosome, still in pieces: no run joins two chromosomes
    _same(g.find_pattern(*rule, step=step), _want(g, rule, None, None, None, step), "whole genome in pieces")


def test_min_len_and_max_gap(monkeypatch):
    idx, g, log = _find_scene(monkeypatch, 11)
    rule = RULES[0]
    plain = g.find_pattern(*rule, "c1", 5, None, 7)
    a, b = (plain["start"].to_numpy() - 5) // 7, (plain["end"].to_numpy() - 1 - 5) // 7 + 1
    for min_len, max_gap in [(1, 1), (2, 0), (4, 2)]:
        s, e, rows = find.merge_runs(a, b, min_len, max_gap)
        want = pd.DataFrame({"chr": np.full(len(s), "c1", object), "start": 5 + s * 7, "end": 5 + (e - 1) * 7 + 1, "rows": rows})
        _same(g.find_pattern(*rule, "c1", 5, None, 7, min_len, max_gap), want, (min_len, max_gap))
        assert len(want) < len(plain)


def test_find_pattern_input_errors(monkeypatch):
    idx, g, log = _find_scene(monkeypatch, 3)
    with pytest.raises(KeyError, match="no chromosome"):
        g.find_pattern(["g1"], chrom="nope")
    with pytest.raises(ValueError, match="step"):
        g.find_pattern(["g1"], chrom="c1", step=0)
    with pytest.raises(ValueError, match="need a chromosome"):
        g.find_pattern(["g1"], start=5, end=10)
    with pytest.raises(ValueError, match="'nobody'"):
        g.find_pattern(["nobody"])
    with pytest.raises(ValueError, match="both"):
        g.find_pattern(["g1"], ["g1"])
    with pytest.raises(ValueError):
        g.find_pattern(["g1"], min_len=0)
    assert log == []  # nothing was read


@pytest.mark.parametrize("step", [1, 100])
def test_pattern_density(monkeypatch, step):
    idx, g, log = _find_scene(monkeypatch, 11)
    rule = RULES[1]
    got = idx.pattern_density("g0", *rule, None, step, 100)
    assert list(got.columns) == ["chr", "start", "matched", "rows"]
    parts = []
    for c in SIZES:
        frame = g.query(c, None, None, step)
        m = _match(frame, *rule)
        b = frame.index.to_numpy().astype(np.int64) // 100
        ub = np.unique(b)
        parts.append(pd.DataFrame({"chr": np.full(len(ub), c, object), "start": ub * 100,
                                   "matched": np.bincount(b, weights=m)[ub].astype(np.int64), "rows": np.bincount(b)[ub]}))
    want = pd.concat(parts, ignore_index=True)
    assert got["chr"].tolist() == want["chr"].tolist()
    for col in ("start", "matched", "rows"):
        assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy().astype(np.int64)), col
    assert 0 < got["matched"].sum() < got["rows"].sum()
    assert g.pattern_density(*rule, chroms=["c2"], step=step, bin_size=100)["chr"].unique().tolist() == ["c2"]
